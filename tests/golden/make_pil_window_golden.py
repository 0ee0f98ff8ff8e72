"""Writes tests/golden/pil_window.npz: Pillow's own `Image.resize(BILINEAR)` bytes of a WINDOW of a raw image, for the cases of the
windowed-view tests (tests/test_view_window_cpu.py, tests/test_view_window_gpu.py).

detectron2's RandomCrop slices the decoded array before ResizeShortestEdge, so the expected bytes of a cropped view are
`Image.fromarray(raw[y0:y0+h, x0:x0+w]).resize((new_w, new_h), BILINEAR)`.  Raw images are not stored: `make_raw(raw_h, raw_w, seed)`
regenerates them.  Stored per case: the row of `cases` (raw_h, raw_w, y0, x0, h, w, new_h, new_w, seed) and the output `out_<i>`.
Flips and the channel exchange are index permutations the tests apply to the expected array themselves.
Run with Pillow installed:  python tests/golden/make_pil_window_golden.py"""
import os

import numpy as np

# (raw_h, raw_w), (y0, x0), (h, w), (new_h, new_w)
CASES = [
    ((40, 50), (9, 7), (23, 37), (45, 71)),          # 1  upscale, odd origin, partial tiles
    ((120, 230), (11, 20), (100, 201), (7, 13)),     # 2  33 taps; row window over the LDS budget, so always two-pass
    ((64, 128), (0, 0), (64, 128), (25, 50)),        # 3  window = image; must also equal launch_weak_views byte for byte
    ((70, 90), (20, 20), (50, 70), (50, 70)),        # 4  no resampling: pure crop
    ((60, 80), (27, 27), (33, 53), (80, 128)),       # 5  window ends at the image's last row and column
    ((9, 9), (4, 4), (1, 1), (1, 1)),                # 6  one-pixel window
    ((9, 9), (8, 8), (1, 1), (4, 4)),                # 7  one-pixel window in the last corner, upscaled
    ((5, 40), (2, 0), (1, 40), (3, 120)),            # 8  one-row window across the full width
    ((50, 90), (3, 10), (33, 47), (99, 47)),         # 9  width kept, height changes
    ((260, 500), (10, 10), (240, 480), (100, 200)),  # 10 fused downscale over several tiles
]


def make_raw(raw_h: int, raw_w: int, seed: int) -> np.ndarray:
    """(raw_h, raw_w, 3) uint8 random bytes"""
    return np.random.RandomState(seed).randint(0, 256, size=(raw_h, raw_w, 3)).astype(np.uint8)


def seed_of(i: int) -> int:
    return 700 + i


def main():
    from PIL import Image
    import PIL
    cases, outs = [], {}
    for i, ((rh, rw), (y0, x0), (h, w), (nh, nw)) in enumerate(CASES):
        raw = make_raw(rh, rw, seed_of(i))
        win = np.ascontiguousarray(raw[y0:y0 + h, x0:x0 + w])
        assert win.shape == (h, w, 3)
        out = np.asarray(Image.fromarray(win).resize((nw, nh), Image.BILINEAR))
        assert out.shape == (nh, nw, 3) and out.dtype == np.uint8
        outs[f"out_{i}"] = out
        cases.append((rh, rw, y0, x0, h, w, nh, nw, seed_of(i)))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pil_window.npz")
    np.savez_compressed(path, cases=np.array(cases, dtype=np.int64), pillow_version=np.array(PIL.__version__), **outs)
    print(path, os.path.getsize(path), "bytes,", len(cases), "cases")


if __name__ == "__main__":
    main()
