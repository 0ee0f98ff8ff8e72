"""Host-side pieces of the device COCO evaluator (aldi_amd/evaluation.py: TEST.DEVICE_EVAL, ground-truth packing, the rank-merge
helper, the constants handed to the kernels); the kernels themselves are held against the host evaluator in test_eval_device_gpu.py."""
import numpy as np
import torch


def test_device_eval_defaults_off_and_the_adapter_is_built():
    from aldi_amd.config import add_aldi_config, get_cfg
    from aldi_amd.evaluation import Detectron2COCOEvaluatorAdapter
    from aldi_amd.trainer import ALDITrainer
    cfg = get_cfg()
    add_aldi_config(cfg)
    assert cfg.TEST.DEVICE_EVAL is False
    recs = [dict(image_id=0, height=10, width=10, annotations=[dict(bbox=[1, 1, 5, 5], bbox_mode="XYWH_ABS", category_id=0)])]
    ev = ALDITrainer.build_evaluator(cfg, "toy_val", dataset_dicts=recs)
    assert type(ev) is Detectron2COCOEvaluatorAdapter


def _records():
    return [
        dict(image_id=7, height=400, width=600, annotations=[
            dict(bbox=[40, 20, 200, 100], bbox_mode="XYWH_ABS", category_id=1),                      # no area: y * w = 4000
            dict(bbox=[10.5, 20.25, 110.75, 90.5], bbox_mode="XYXY_ABS", category_id=0, iscrowd=1),
            dict(bbox=[5, 6, 30, 40], bbox_mode="XYWH_ABS", category_id=1, area=1234.5)]),
        dict(image_id=3, height=400, width=600, annotations=[]),
        dict(image_id=9, height=200, width=300, annotations=[
            dict(bbox=[1, 2, 3, 4], bbox_mode=0, category_id=2, iscrowd=0, area=2.0),                 # BoxMode.XYXY_ABS == 0
            dict(bbox=[50, 60, 70, 80], category_id=0),
            dict(bbox=[9, 9, 9, 9], bbox_mode="XYWH_ABS", category_id=2)]),
    ]


def test_ground_truth_packing_matches_the_adapter_annotations():
    from aldi_amd.evaluation import Detectron2COCOEvaluatorAdapter, maybe_add_optional_annotations, pack_ground_truth
    K = 3
    host = Detectron2COCOEvaluatorAdapter("toy_val", _records(), K, distributed=False)
    before = [dict(a) for a in host.annotations]
    g = pack_ground_truth(host.images, host.annotations, K)
    assert host.annotations == before                                  # the adapter's list is not modified
    anns = [dict(a) for a in host.annotations]
    maybe_add_optional_annotations(anns)
    off = g["off"]
    assert off.dtype == np.int32 and off.shape == (len(host.images) * K + 1,) and off[0] == 0 and off[-1] == len(anns)
    assert g["boxes"].dtype == np.float64 and g["area"].dtype == np.float64 and g["flags"].dtype == np.uint8
    for i, im in enumerate(host.images):
        for c in range(K):
            want = [a for a in anns if a["image_id"] == im["id"] and a["category_id"] == c]       # annotation order inside a segment
            lo, hi = off[i * K + c], off[i * K + c + 1]
            assert hi - lo == len(want)
            for k, a in enumerate(want):
                assert g["boxes"][lo + k].tolist() == a["bbox"]
                assert g["area"][lo + k] == a["area"]
                assert g["flags"][lo + k] == (1 if a["iscrowd"] else 0)
    seg = lambda i, c: slice(off[i * K + c], off[i * K + c + 1])
    assert g["area"][seg(0, 1)].tolist() == [20.0 * 200.0, 1234.5]      # the reference's bbox[1] * bbox[2]
    assert g["boxes"][seg(0, 0)].tolist() == [[10.5, 20.25, 110.75 - 10.5, 90.5 - 20.25]] and g["flags"][seg(0, 0)].tolist() == [1]
    assert g["boxes"][seg(2, 2)].tolist() == [[1.0, 2.0, 2.0, 2.0], [9.0, 9.0, 9.0, 9.0]]
    assert off[1 * K:2 * K + 1].tolist() == [off[K]] * (K + 1)          # the image without annotations: empty segments


def test_packing_keeps_an_ignore_flag_and_drops_what_the_host_never_looks_up():
    from aldi_amd.evaluation import pack_ground_truth
    anns = [dict(image_id=0, category_id=0, bbox=[0.0, 0.0, 5.0, 5.0], area=25.0, ignore=1),
            dict(image_id=0, category_id=5, bbox=[0.0, 0.0, 5.0, 5.0], area=25.0),                  # category outside 0..K-1
            dict(image_id=4, category_id=0, bbox=[0.0, 0.0, 5.0, 5.0], area=25.0),                  # unknown image
            dict(image_id=0, category_id=0, bbox=[1.0, 1.0, 5.0, 5.0], area=25.0, iscrowd=1, ignore=1)]
    g = pack_ground_truth([dict(id=0)], anns, 2)
    assert g["off"].tolist() == [0, 2, 2] and g["flags"].tolist() == [2, 3]


def _shard(rng, image_ids):
    out = []
    for i in image_ids:
        n = int(rng.randint(0, 5))
        out.append((torch.from_numpy(rng.uniform(0, 100, (n, 4))), torch.from_numpy(np.round(rng.rand(n), 1)), torch.from_numpy(rng.randint(0, 3, n)),
                    torch.full((n,), i, dtype=torch.int64), torch.from_numpy(rng.rand(n) < 0.8)))
    return out


def test_rank_merge_gives_the_unsharded_arrays_in_either_gather_order():
    from aldi_amd.evaluation import merge_detection_shards
    per_image = _shard(np.random.RandomState(0), range(7))
    whole = tuple(torch.cat([p[k] for p in per_image]) for k in range(5))                            # one rank, images in order
    rank = lambda r: tuple(torch.cat([p[k] for p in per_image[r::2]]) for k in range(5))             # InferenceSampler-style shards
    for shards in ([rank(0), rank(1)], [rank(1), rank(0)]):
        merged = merge_detection_shards(shards)
        assert len(merged) == 5
        for m, w in zip(merged, whole):
            assert m.dtype == w.dtype and torch.equal(m, w)
    for m, w in zip(merge_detection_shards([whole]), whole):
        assert torch.equal(m, w)


def test_kernel_constants_are_the_host_thresholds_bytewise():
    from aldi_amd.evaluation import AREA_RNG, IOU_THRS, REC_THRS, kernel_constants
    c = kernel_constants()
    assert c["iou_thrs"].dtype == np.float64 and c["iou_thrs"].tobytes() == IOU_THRS.tobytes() and c["iou_thrs"].shape == (10,)
    assert c["rec_thrs"].dtype == np.float64 and c["rec_thrs"].tobytes() == REC_THRS.tobytes() and c["rec_thrs"].shape == (101,)
    assert c["area_rng"].dtype == np.float64 and c["area_rng"].tolist() == [list(r) for r in AREA_RNG.values()]
    assert c["area_rng"].flags["C_CONTIGUOUS"] and c["area_rng"].shape == (4, 2)


def test_summarize_bbox_is_what_coco_bbox_metrics_returns():
    from aldi_amd.evaluation import AREA_RNG, MAX_DETS, accumulate, coco_bbox_metrics, evaluate_img, summarize_bbox
    anns = [dict(image_id=0, category_id=0, bbox=[0.0, 0.0, 50.0, 50.0], area=2500.0, iscrowd=0),
            dict(image_id=0, category_id=0, bbox=[100.0, 100.0, 60.0, 60.0], area=3600.0, iscrowd=0)]
    dets = [dict(image_id=0, category_id=0, bbox=[0.0, 0.0, 50.0, 50.0], score=0.9), dict(image_id=0, category_id=0, bbox=[300.0, 300.0, 40.0, 40.0], score=0.8),
            dict(image_id=0, category_id=0, bbox=[100.0, 100.0, 60.0, 55.0], score=0.7)]
    res = coco_bbox_metrics([dict(id=0)], [dict(a) for a in anns], dets, [0, 1])
    prec = {(c, an): accumulate([evaluate_img(dets if c == 0 else [], anns if c == 0 else [], rng, MAX_DETS[-1])]) for c in (0, 1)
            for an, rng in AREA_RNG.items()}
    mine = summarize_bbox(prec, [0, 1])
    assert list(mine) == list(res) and all(mine[k] == res[k] or (mine[k] != mine[k] and res[k] != res[k]) for k in res)
