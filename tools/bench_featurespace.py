"""Measurement for the device feature-space PCA (aldi_amd/featurespace.py, csrc/featstat.hip).  Prints ONE JSON line (and writes it to
--out).  On the synthetic validation split (SYNTHETIC.VAL_IMAGES images of 800 x 1333, one per batch, bf16, ALDI-Best-Cityscapes.yaml):

* `RCNN.feature_pass` next to `RCNN.inference` on the same images (device events around every call, median per image);
* the three new kernels alone on one image's tensors (50 back-to-back launches between two events, divided; median of --repeats): pool_rows on p6, pool_rows_counted on the
  (P, 7, 7, 256) RoIAlign output, moments_accum on both levels, project2 on the proposal rows;
* pool_rows_counted's achieved bytes/s against its compulsory traffic (the valid rows of x read once, the pooled rows written once)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from aldi_amd import ops
from aldi_amd.arch import FPN_C, POOL

KB = 50     # back-to-back launches per timed interval of a single kernel


def timed(fn, repeats, warmup=3, batch=1):
    """median ms of one call; batch > 1: `batch` back-to-back calls between the two events, divided (the launches queue up behind
    each other, so the figure is the kernel's own time and not the launch latency of a microsecond-scale kernel)"""
    ts = []
    for k in range(warmup + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        if k >= warmup:
            ts.append(a.elapsed_time(b) / batch)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from aldi_amd.config import add_aldi_config, get_cfg
    from aldi_amd.trainer import ALDITrainer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(os.path.join(root, "configs", "cityscapes", "ALDI-Best-Cityscapes.yaml"))
    cfg.merge_from_list(["SEED", 1])
    model = ALDITrainer.build_model(cfg)
    m = model.engine
    batches, _ = ALDITrainer.build_test_loader(cfg, "synthetic_val")
    images = [[b["image"].cuda() for b in batch] for batch in batches]
    with torch.no_grad():
        t_inf = statistics.median(timed(lambda im=im: m.inference(im, 2.0), a.repeats) for im in images)
        t_fp = statistics.median(timed(lambda im=im: m.feature_pass(im), a.repeats) for im in images)
        # one image's tensors for the kernels alone
        im = images[0]
        st, sizes, hw = m.stage_images(im)
        c = m.trunk(st, sizes, save=False)
        m.rpn_head(c, save=False)
        _, geom, anchors = m.geometry(st.shape[2], st.shape[3])
        props, _, pcount = m.proposals(c, geom, anchors, hw, 1, training=False)
        P = props.shape[1]
        rois = torch.empty((P, 5), dtype=torch.float32, device=m.device)
        ops.rois_from_proposals(props, pcount, P, 1, rois)
        pooled = torch.empty((P, POOL, POOL, FPN_C), dtype=m.dtype, device=m.device)
        ops.roialign(m.roi_feats(c), rois, P, POOL, pooled, backward=False)
        p6 = c.P[4]
        img = torch.empty((1, FPN_C), dtype=torch.float32, device=m.device)
        prop = torch.empty((P, FPN_C), dtype=torch.float32, device=m.device)
        total = torch.zeros(1, dtype=torch.int32, device=m.device)
        x4 = pooled.view(1, P, POOL * POOL, FPN_C)
        x3 = p6.view(1, p6.shape[1] * p6.shape[2], FPN_C)
        t_pool_img = timed(lambda: ops.pool_rows(x3, img), a.repeats, batch=KB)
        t_pool_prop = timed(lambda: ops.pool_rows_counted(x4, pcount, prop, total), a.repeats, batch=KB)
        n = int(total)
        ws = ops.moments_workspace(FPN_C, m.device)
        acc = [torch.zeros(s, dtype=torch.float64, device=m.device) for s in (FPN_C, FPN_C * FPN_C, 1)]
        t_mom_prop = timed(lambda: ops.moments_accum(prop, acc[0], acc[1].view(FPN_C, FPN_C), acc[2], ws, n_dev=total), a.repeats, batch=KB)
        t_mom_img = timed(lambda: ops.moments_accum(img, acc[0], acc[1].view(FPN_C, FPN_C), acc[2], ws), a.repeats, batch=KB)
        mean = torch.zeros(FPN_C, dtype=torch.float64, device=m.device)
        comp = torch.zeros(2, FPN_C, dtype=torch.float64, device=m.device)
        y = torch.empty((n, 2), dtype=torch.float32, device=m.device)
        xs = prop[:n].contiguous()
        t_proj = timed(lambda: ops.project2(xs, mean, comp, out=y), a.repeats, batch=KB)
    nbytes = n * POOL * POOL * FPN_C * pooled.element_size() + n * FPN_C * 4
    out = {"bench": "featurespace", "gpu": torch.cuda.get_device_name(0), "dtype": str(m.dtype), "images": len(images),
           "canvas": [int(st.shape[2]), int(st.shape[3])], "proposals_per_image": n, "p6_positions": int(x3.shape[1]),
           "inference_ms_per_image": round(t_inf, 4), "feature_pass_ms_per_image": round(t_fp, 4),
           "feature_pass_over_inference": round(t_fp / t_inf, 4),
           "kernel_us": {"pool_rows_image": round(t_pool_img * 1e3, 2), "pool_rows_counted_proposals": round(t_pool_prop * 1e3, 2),
                         "moments_accum_proposals": round(t_mom_prop * 1e3, 2), "moments_accum_image": round(t_mom_img * 1e3, 2),
                         "project2_proposals": round(t_proj * 1e3, 2)},
           "pool_rows_counted_compulsory_bytes": nbytes, "pool_rows_counted_GBps": round(nbytes / (t_pool_prop * 1e-3) / 1e9, 1),
           "added_kernels_share_of_feature_pass": round((t_pool_img + t_pool_prop + t_mom_prop + t_mom_img) / t_fp, 4),
           "timing": "passes: device events around one call; kernels: events around %d back-to-back launches, divided; median of --repeats after 3 warm-up rounds" % KB}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
