"""Writes tests/golden/pil_bilinear.npz: Pillow's own `Image.resize(BILINEAR)` bytes for the shapes of the weak-view tests.

Inputs are not stored: `make_input(h, w, seed, binary)` regenerates them.  Stored per case: the row of `cases`
(h, w, new_h, new_w, seed, binary) and the output `out_<i>`.  Run with Pillow installed:  python tests/golden/make_pil_golden.py"""
import os

import numpy as np

# (h, w) -> (new_h, new_w): the shapes tests/test_weak_aug_gpu.py runs, see its table for the reason of each
SHAPES = [
    ((37, 53), (80, 115)), ((64, 128), (25, 50)), ((50, 70), (50, 35)), ((33, 47), (99, 47)), ((50, 70), (50, 70)),
    ((100, 201), (7, 13)), ((5, 3), (64, 64)), ((1, 9), (4, 36)), ((9, 1), (27, 3)), ((240, 480), (100, 200)),
    ((37, 53), (1, 1)), ((1, 1), (1, 1)), ((3, 200), (1, 1)),
]


def make_input(h: int, w: int, seed: int, binary: bool) -> np.ndarray:
    """(h, w, 3) uint8: random bytes, or only 0 and 255 when `binary`"""
    rs = np.random.RandomState(seed)
    if binary:
        return (rs.randint(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)
    return rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8)


def main():
    from PIL import Image
    import PIL
    cases, outs = [], {}
    for i, ((h, w), (nh, nw)) in enumerate(SHAPES):
        for binary in (False, True):
            seed = 100 + 2 * i + int(binary)
            img = make_input(h, w, seed, binary)
            out = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))
            assert out.shape == (nh, nw, 3) and out.dtype == np.uint8
            outs[f"out_{len(cases)}"] = out
            cases.append((h, w, nh, nw, seed, int(binary)))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pil_bilinear.npz")
    np.savez_compressed(path, cases=np.array(cases, dtype=np.int64), pillow_version=np.array(PIL.__version__), **outs)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
