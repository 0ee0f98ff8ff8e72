"""Inference API on the device: aldi_detector_postprocess and aldi_tta_merge (csrc/infer.hip) against the CPU restatements of
tests/infer_refs.py, then `inference(do_postprocess=True)`, `Predictor` and `GeneralizedRCNNWithTTA` on tiny synthetic models.
Every comparison is exact: the device does the same float32 operations in the same order."""
import os

import numpy as np
import pytest
import torch

import infer_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
GUARD = 64


# ------------------------------------------------------------------------------------------------ helpers
def upload_descs(descs):
    """restated descriptors -> device bytes of aldi_box_tfm structs"""
    from aldi_amd import _lib as L
    arr = (L.BoxTfm * len(descs))()
    for t, d in zip(arr, descs):
        for k, v in d.items():
            setattr(t, k, float(v))
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)


class Carved:
    """outputs carved out of one buffer filled with 0xA5, GUARD bytes between them, at offsets that are multiples of 4 only"""

    def __init__(self, specs):
        self.spans, off = [], GUARD + 4
        for shape, dtype in specs:
            nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            self.spans.append((off, nbytes, shape, dtype))
            off += nbytes + GUARD + 4
        self.buf = torch.full((off,), 0xA5, dtype=torch.uint8, device=DEV)
        self.tensors = [self.buf[o:o + n].view(dt).view(sh) for o, n, sh, dt in self.spans]

    def guards_untouched(self):
        host = self.buf.cpu().numpy().copy()
        for o, n, _, _ in self.spans:
            host[o:o + n] = 0xA5
        return bool((host == 0xA5).all())


# ------------------------------------------------------------------------------------------------ aldi_detector_postprocess alone
@pytest.mark.parametrize("D", [7, 130])                       # one partial round; three rounds of 64, the last one partial
def test_postprocess_kernel_equals_the_restatement(D):
    from aldi_amd import ops
    rng = np.random.RandomState(D)
    N, counts = 3, [D, 3, 0]
    # network space 100 x 80; per image: scales above and below 1, different per axis / exactly 1.0 / below and above 1
    descs = [R.desc((150, 60), (150 / 100, 60 / 80)), R.desc((100, 80)), R.desc((37, 106), (37 / 100, 106 / 80))]
    x1 = rng.uniform(-20, 110, (N, D)).astype(F)
    y1 = rng.uniform(-20, 90, (N, D)).astype(F)
    boxes = np.stack([x1, y1, x1 + rng.uniform(0, 40, (N, D)).astype(F), y1 + rng.uniform(0, 40, (N, D)).astype(F)], -1).astype(F)
    directed = np.array([[10, 10, np.nextafter(F(10), F(11)), 20],      # only just survives: one ulp wide
                         [105, 10, 130, 20],                           # right of the clip: zero width after the clamp
                         [12, 10, 12, 20],                             # x1 == x2 before scaling
                         [-30, 10, -5, 20]], dtype=F)                  # entirely left of 0
    boxes[:, :4] = directed
    for n, c in enumerate(counts):
        boxes[n, c:] = 1e6                                             # rows past the count are never read into the output
    scores = rng.uniform(0.01, 1, (N, D)).astype(F)
    classes = rng.randint(0, 3, (N, D)).astype(np.int32)
    ref = R.postprocess(torch.from_numpy(boxes), torch.from_numpy(scores), torch.from_numpy(classes), counts, descs)
    assert ref[3][1] >= 1 and ref[0][1, 0].tolist() == directed[0].tolist()          # the one-ulp box is kept at scale 1.0
    assert ref[3].tolist()[2] == 0 and 0 < ref[3].tolist()[0] < D                    # an empty image; some rows dropped, some kept
    out = Carved([((N, D, 4), torch.float32), ((N, D), torch.float32), ((N, D), torch.int32), ((N,), torch.int32)])
    ob, os_, oc, on = out.tensors
    ops.detector_postprocess(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), torch.from_numpy(classes).to(DEV),
                             torch.tensor(counts, dtype=torch.int32, device=DEV), upload_descs(descs), ob, os_, oc, on)
    torch.cuda.synchronize()
    assert on.cpu().tolist() == ref[3].tolist()
    assert torch.equal(ob.cpu(), ref[0]) and torch.equal(os_.cpu(), ref[1]) and torch.equal(oc.cpu(), ref[2])       # fill rows included
    assert out.guards_untouched()


# ------------------------------------------------------------------------------------------------ aldi_tta_merge alone
def _run_merge(boxes, scores, classes, count, descs, K, floor, thr, topk):
    """boxes [B][A][D][4] ... numpy -> the kernel's outputs (carved, guards checked) as CPU tensors"""
    from aldi_amd import ops
    B, A, D = scores.shape
    out = Carved([((B, topk, 4), torch.float32), ((B, topk), torch.float32), ((B, topk), torch.int32), ((B,), torch.int32)])
    ob, os_, oc, on = out.tensors
    ws = torch.empty(ops.tta_merge_workspace(B, A, D), dtype=torch.uint8, device=DEV)
    ops.tta_merge(torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV), torch.from_numpy(classes).to(DEV),
                  torch.from_numpy(np.asarray(count, np.int32)).to(DEV), upload_descs([d for row in descs for d in row]),
                  K, floor, thr, topk, ws, ob, os_, oc, on)
    torch.cuda.synchronize()
    assert out.guards_untouched()
    return ob.cpu(), os_.cpu(), oc.cpu(), on.cpu()


@pytest.mark.parametrize("B,A,D,topk", [(2, 3, 5, 100), (1, 6, 100, 100), (1, 11, 100, 100)])   # 1100 rows: past the sort's 1024 padding, 18 mask words
def test_merge_kernel_equals_the_restatement(B, A, D, topk):
    rng = np.random.RandomState(A * D)
    K, Wo, Ho = 3, 120, 90
    # view a of image b: its two scale stages and its flip; view 1 is flipped, view 2 has both stages different from 1
    descs, fwd = [], []
    for b in range(B):
        row, f = [], []
        for a in range(A):
            s0 = (1.0, 1.0) if a == 0 else (60 / (40 + 7 * a), 45 / (31 + 5 * a))
            s1 = (120 / 60, 90 / 45) if a == 2 else (1.0, 1.0)
            vw = Wo / (s0[0] * s1[0])                                     # the view's width in its own pixels
            row.append(R.desc((Wo, Ho), s0, s1, vw if a == 1 else None))
            f.append((s0[0] * s1[0], s0[1] * s1[1], vw if a == 1 else None))
        descs.append(row)
        fwd.append(f)
    # D / 2 base boxes per image in original pixels; every view sees each of them jittered, so suppression has work to do
    M = max(D // 2, 1)
    bx, by = rng.uniform(-5, Wo - 10, (B, M)), rng.uniform(-5, Ho - 10, (B, M))
    bw, bh = rng.uniform(4, 50, (B, M)), rng.uniform(4, 40, (B, M))
    boxes = np.zeros((B, A, D, 4), F)
    for b in range(B):
        for a in range(A):
            which = rng.randint(0, M, D)
            j = rng.uniform(-2, 2, (D, 4))
            o = np.stack([bx[b, which], by[b, which], bx[b, which] + bw[b, which], by[b, which] + bh[b, which]], 1) + j
            sx, sy, fw = fwd[b][a]
            v = o / np.array([sx, sy, sx, sy])
            if fw is not None:
                v[:, [0, 2]] = fw - v[:, [2, 0]]
            boxes[b, a] = v.astype(F)
    n = B * A * D
    scores = (0.05 + 0.9 * (rng.permutation(n) + 0.5) / n).astype(F).reshape(B, A, D)
    assert len(np.unique(scores)) == n                                   # distinct after the rounding to float32
    classes = rng.randint(0, K, (B, A, D)).astype(np.int32)
    count = np.full((B, A), D, np.int32)
    if B == 2:
        count[:] = [[5, 3, 0], [2, 5, 4]]
    ob, os_, oc, on = _run_merge(boxes, scores, classes, count, descs, K, 1e-8, 0.5, topk)
    kept = 0
    for b in range(B):
        rb, rs, rc, rn = R.merge(boxes[b], scores[b], classes[b], count[b], descs[b], K, 1e-8, 0.5, topk)
        assert int(on[b]) == rn
        assert torch.equal(ob[b], torch.from_numpy(rb)) and torch.equal(os_[b], torch.from_numpy(rs)) and torch.equal(oc[b], torch.from_numpy(rc))
        kept += rn
    assert 0 < kept < int(count.sum())                                   # something was suppressed, something survived
    if A * D >= 600:
        assert kept == topk                                              # more survivors than topk: the output is cut


def test_merge_kernel_directed_rules():
    boxes, scores, classes, count, exp = R.directed_merge_case()
    descs = [[R.desc((100, 100))] * 3]
    for topk in (100, 4):                                                # 4: more survivors than topk
        ob, os_, oc, on = _run_merge(boxes[None], scores[None], classes[None], count[None], descs, 3, 1e-8, 0.5, topk)
        want = exp[:topk]
        n = int(on[0])
        assert n == len(want)
        assert ob[0, :n].tolist() == [[float(x) for x in r[0]] for r in want]
        assert os_[0, :n].tolist() == [float(F(r[1])) for r in want] and oc[0, :n].tolist() == [r[2] for r in want]
        assert not ob[0, n:].any() and not os_[0, n:].any() and bool((oc[0, n:] == -1).all())
        rb, rs, rc, rn = R.merge(boxes, scores, classes, count, descs[0], 3, 1e-8, 0.5, topk)
        assert rn == n and torch.equal(ob[0], torch.from_numpy(rb)) and torch.equal(os_[0], torch.from_numpy(rs)) and torch.equal(oc[0], torch.from_numpy(rc))
    ob, os_, oc, on = _run_merge(boxes[None], scores[None], classes[None], np.zeros((1, 3), np.int32), descs, 3, 1e-8, 0.5, 10)
    assert on.tolist() == [0] and not ob.any() and not os_.any() and bool((oc == -1).all())        # all views empty


# ------------------------------------------------------------------------------------------------ end to end, tiny synthetic models
H, W, K = 64, 96, 3
_models = {}


def _rcnn_cfg(*opts):
    from aldi_amd.config import add_aldi_config, get_cfg
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_list(["MODEL.ROI_HEADS.NUM_CLASSES", K, "SEED", 1, "TEST.DETECTIONS_PER_IMAGE", 20, "MODEL.ROI_HEADS.SCORE_THRESH_TEST", 0.0,
                         "MODEL.RPN.POST_NMS_TOPK_TEST", 300, "INPUT.MIN_SIZE_TEST", 64, "INPUT.MAX_SIZE_TEST", 96,
                         "TEST.AUG.MIN_SIZES", (48, 64), "TEST.AUG.MAX_SIZE", 96, "SYNTHETIC.HEIGHT", 96, "SYNTHETIC.WIDTH", 128,
                         "SYNTHETIC.VAL_IMAGES", 3] + list(opts))
    return cfg


def _detr_cfg():
    from aldi_amd.config import add_aldi_config, get_cfg
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(os.path.join(ROOT, "configs", "Base-DETR.yaml"))
    cfg.merge_from_list(["MODEL.DEFORMABLE_DETR.NUM_CLASSES", K, "MODEL.DEFORMABLE_DETR.TRANSFORMER.NUM_QUERIES", 40,
                         "MODEL.DEFORMABLE_DETR.TRANSFORMER.ENC_LAYERS", 2, "MODEL.DEFORMABLE_DETR.TRANSFORMER.DEC_LAYERS", 2, "SEED", 3])
    return cfg


def _model(kind):
    """one tiny model per kind for the whole module, in eval mode"""
    if kind not in _models:
        from aldi_amd.model import build_aldi
        torch.manual_seed(0)
        _models[kind] = build_aldi(_rcnn_cfg() if kind == "r50" else _detr_cfg()).eval()
    return _models[kind]


def _images(n, sizes=None, seed=0):
    g = torch.Generator().manual_seed(seed)
    from aldi_amd import synthetic as syn
    return [syn.make_image(h, w, 4, K, g)[0] for h, w in (sizes or [(H, W)] * n)]


def _restated(insts, out_sizes):
    """the restated postprocess of a list of network-space Instances -> [(boxes, scores, classes int64)] on the CPU"""
    res = []
    for inst, (oh, ow) in zip(insts, out_sizes):
        ih, iw = inst.image_size
        n = len(inst.scores)
        ob, os_, oc, on = R.postprocess(inst.pred_boxes.tensor.cpu().reshape(1, n, 4), inst.scores.cpu().reshape(1, n),
                                        inst.pred_classes.cpu().to(torch.int32).reshape(1, n), [n], [R.desc((ow, oh), (ow / iw, oh / ih))])
        k = int(on[0])
        res.append((ob[0, :k], os_[0, :k], oc[0, :k].to(torch.int64)))
    return res


def _same(result, want, size):
    inst = result["instances"]
    assert tuple(inst.image_size) == tuple(size)
    assert inst.pred_boxes.tensor.is_cuda and inst.pred_classes.dtype == torch.int64
    assert torch.equal(inst.pred_boxes.tensor.cpu(), want[0]) and torch.equal(inst.scores.cpu(), want[1]) and torch.equal(inst.pred_classes.cpu(), want[2])


@pytest.mark.parametrize("kind", ["r50", "detr"])
def test_inference_with_postprocess_equals_the_restatement(kind):
    """fails before the feature with the AssertionError of `assert not do_postprocess`"""
    from aldi_amd.structures import Instances
    model = _model(kind)
    data = [{"image": im, "height": 128, "width": 200} for im in _images(2)]
    data[1].pop("height")                                                # a missing key falls back to the network-input size
    net = model.inference(data, do_postprocess=False)
    assert isinstance(net, list) and all(isinstance(o, Instances) and tuple(o.image_size) == (H, W) for o in net)     # as before: network-input space
    assert all(len(o.scores) > 0 for o in net)
    assert all(isinstance(o, Instances) for o in model(data))            # the eval-mode forward is unchanged too
    out = model.inference(data, do_postprocess=True)
    sizes = [(128, 200), (H, 200)]
    assert isinstance(out, list) and len(out) == 2 and all(set(o) == {"instances"} for o in out)
    for o, want, size in zip(out, _restated(net, sizes), sizes):
        _same(o, want, size)


def test_predictor_equals_the_manual_chain():
    from aldi_amd import aug
    from aldi_amd.predictor import Predictor
    model = _model("r50")
    pred = Predictor(_rcnn_cfg(), model=model)
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, (50, 70, 3)).astype(np.uint8)
    p = aug.WeakParams(50, 70, 64, 90, False)                            # ResizeShortestEdge(64, 96) of 50 x 70
    view = aug.weak_views([torch.from_numpy(img).to(DEV)], [p], chw_out=True, chw_in=False)[0]
    assert tuple(view.shape) == (3, 64, 90)
    want = _restated(model.inference([{"image": view}], do_postprocess=False), [(50, 70)])[0]
    _same(pred(img), want, (50, 70))
    _same(pred(torch.from_numpy(img)), want, (50, 70))                   # a host tensor
    _same(pred(torch.from_numpy(img).to(DEV)), want, (50, 70))           # a device tensor
    # INPUT.FORMAT "RGB": the channels are reversed before the resize
    rgb = Predictor(_rcnn_cfg("INPUT.FORMAT", "RGB"), model=model)
    a, b = rgb(img)["instances"], pred(np.ascontiguousarray(img[:, :, ::-1]))["instances"]
    assert torch.equal(a.pred_boxes.tensor, b.pred_boxes.tensor) and torch.equal(a.scores, b.scores) and torch.equal(a.pred_classes, b.pred_classes)
    assert not torch.equal(a.scores.cpu(), want[1])                      # (and the order matters to the model)
    # a ragged batch: one resize call, one inference call on the two-image batch
    img2 = rng.randint(0, 256, (40, 90, 3)).astype(np.uint8)
    p2 = aug.WeakParams(40, 90, *aug.ResizeShortestEdge.get_output_shape(40, 90, 64, 96), False)
    views = aug.weak_views([torch.from_numpy(img).to(DEV), torch.from_numpy(img2).to(DEV)], [p, p2], chw_out=True, chw_in=False)
    wants = _restated(model.inference([{"image": v} for v in views], do_postprocess=False), [(50, 70), (40, 90)])
    for o, w_, size in zip(pred.batch([img, img2]), wants, [(50, 70), (40, 90)]):
        _same(o, w_, size)
    # MIN_SIZE_TEST 0: no resize
    same = Predictor(_rcnn_cfg("INPUT.MIN_SIZE_TEST", 0), model=model)
    keep = _restated(model.inference([{"image": torch.from_numpy(img).to(DEV).permute(2, 0, 1).contiguous()}], do_postprocess=False), [(50, 70)])[0]
    _same(same(img), keep, (50, 70))


def test_tta_wrapper_equals_the_restated_merge():
    from aldi_amd import aug
    from aldi_amd.tta import GeneralizedRCNNWithTTA, tta_views
    cfg, model = _rcnn_cfg(), _model("r50")
    image = _images(1, [(50, 70)], seed=5)[0].to(DEV)
    inp = {"image": image, "height": 100, "width": 140, "image_id": 7}   # the input image is itself a resize of a 100 x 140 original
    shapes = [(48, 67, False), (48, 67, True), (64, 90, False), (64, 90, True)]
    views, tfms = tta_views(cfg, image, 100, 140)
    assert [tuple(v["image"].shape) for v in views] == [(3, nh, nw) for nh, nw, _ in shapes] and len(tfms) == 4
    params = [aug.WeakParams(50, 70, nh, nw, fl) for nh, nw, fl in shapes]
    mine = aug.weak_views([image] * 4, params, chw_out=True, chw_in=True)
    assert all(torch.equal(v["image"], m) for v, m in zip(views, mine))
    out = GeneralizedRCNNWithTTA(cfg, model, batch_size=3)([inp])
    assert len(out) == 1
    # the reference uses the wrapper's batching (the padded canvas depends on the batch): views 0..2 together, then view 3
    dets = model.inference([{"image": m} for m in mine[:3]], do_postprocess=False) + model.inference([{"image": mine[3]}], do_postprocess=False)
    D = max(len(d.scores) for d in dets)
    boxes, scores, classes = np.zeros((4, D, 4), F), np.zeros((4, D), F), np.full((4, D), -1, np.int32)
    for a, d in enumerate(dets):
        n = len(d.scores)
        boxes[a, :n], scores[a, :n], classes[a, :n] = d.pred_boxes.tensor.cpu().numpy(), d.scores.cpu().numpy(), d.pred_classes.cpu().numpy()
    descs = [R.view_desc(50, 70, nh, nw, fl, 100, 140) for nh, nw, fl in shapes]
    rb, rs, rc, rn = R.merge(boxes, scores, classes, [len(d.scores) for d in dets], descs, K, 1e-8, cfg.MODEL.ROI_HEADS.NMS_THRESH_TEST, 20)
    assert 0 < rn <= 20
    _same(out[0], (torch.from_numpy(rb[:rn]), torch.from_numpy(rs[:rn]), torch.from_numpy(rc[:rn]).to(torch.int64)), (100, 140))


@pytest.mark.parametrize("device_eval", [False, True])
def test_ground_truth_model_scores_100_through_test_with_tta(device_eval, tmp_path):
    """a "model" that answers every view with the ground truth transformed into that view (flipped views included): the merge
    must bring every view back onto the same boxes, so the evaluators see each annotation once, exactly"""
    from aldi_amd import aug
    from aldi_amd.structures import Boxes, Instances
    from aldi_amd.trainer import ALDITrainer
    # (suppression at 0.99: the copies of one annotation in the views overlap at IoU 1 up to rounding and collapse to one detection,
    # while two different annotations of one class are never that close)
    cfg = _rcnn_cfg("TEST.DEVICE_EVAL", device_eval, "MODEL.ROI_HEADS.NMS_THRESH_TEST", 0.99, "TEST.AUG.MIN_SIZES", (64, 120), "TEST.AUG.MAX_SIZE", 150)
    cfg.OUTPUT_DIR = str(tmp_path)
    _, records = ALDITrainer.build_test_loader(cfg, "synthetic_val")
    seen = []

    class GroundTruthModel:
        training = False

        def eval(self):
            return self

        def train(self, mode=True):
            return self

        def inference(self, views, do_postprocess=False):
            assert not do_postprocess and len(views) <= 3
            out = []
            for v in views:
                p, r = v["transforms"], records[v["image_id"]]
                seen.append((v["image_id"], p.new_h, p.new_w, p.flip))
                assert tuple(v["image"].shape) == (3, p.new_h, p.new_w) and (v["height"], v["width"]) == (96, 128)
                gt = np.array([a["bbox"] for a in r["annotations"]], dtype=np.float64).reshape(-1, 4)
                inst = Instances((p.new_h, p.new_w))
                inst.pred_boxes = Boxes(torch.from_numpy(aug.transform_boxes(gt, p)).to(torch.float32))
                inst.scores = torch.linspace(0.99, 0.5, len(gt))
                inst.pred_classes = torch.tensor([a["category_id"] for a in r["annotations"]], dtype=torch.int64)
                out.append(inst)
            return out
    res = ALDITrainer.test_with_TTA(cfg, GroundTruthModel())
    assert set(res) == {"bbox_TTA"}
    assert res["bbox_TTA"]["AP"] == pytest.approx(100.0) and res["bbox_TTA"]["AP50"] == pytest.approx(100.0), res
    assert seen[:4] == [(0, 64, 85, False), (0, 64, 85, True), (0, 113, 150, False), (0, 113, 150, True)] and len(seen) == 12
