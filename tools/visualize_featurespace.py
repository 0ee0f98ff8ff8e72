#!/usr/bin/env python
"""Domain-gap diagnostic: 2-component PCA of image-level (p6, pooled) and proposal-level (7x7 RoIAlign bins, pooled) features of a
source and a target test set -- what the reference's tools/visualize_featurespace.py plots -- computed on the device
(aldi_amd/featurespace.py: only a 256 x 256 moment matrix per level and the 2-D coordinates reach the host).

    python tools/visualize_featurespace.py --config-file configs/cityscapes/ALDI-Best-Cityscapes.yaml [--resume] [KEY VALUE ...]

Source and target: two DATASETS.TEST names, or one DATASETS.TRAIN plus one DATASETS.TEST name (anything else is an error).  A
config that names no data set at all runs on the synthetic loaders, which ignore the name, as `ALDITrainer.test` does.
Writes OUTPUT_DIR/featurespace.npz (per level: components, mean, explained_variance_ratio, count, coords of either data set) and, when
matplotlib is installed, OUTPUT_DIR/feature_vis_image_pca.png and feature_vis_proposal_pca.png."""
import argparse
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

SYNTHETIC_NAMES = ("synthetic_source", "synthetic_target")
logger = logging.getLogger("visualize_featurespace")


def setup(args):
    from aldi_amd.config import add_aldi_config, get_cfg
    cfg = get_cfg()
    add_aldi_config(cfg)
    cfg.merge_from_file(args.config_file)
    cfg.merge_from_list(list(args.opts))
    return cfg


def dataset_names(cfg):
    from aldi_amd.featurespace import select_datasets
    train, test = list(cfg.DATASETS.TRAIN), list(cfg.DATASETS.TEST)
    if not train and not test:
        logger.info("the config names no data sets: using the synthetic loaders as %s", SYNTHETIC_NAMES)
        return SYNTHETIC_NAMES
    return select_datasets(train, test)


def load_model(cfg, resume: bool):
    from aldi_amd.checkpoint import DetectionCheckpointerWithEMA
    from aldi_amd.ema import EMA
    from aldi_amd.trainer import ALDITrainer
    model = ALDITrainer.build_model(cfg)
    ckpt = DetectionCheckpointerWithEMA(model, save_dir=cfg.OUTPUT_DIR)
    if cfg.EMA.ENABLED and cfg.EMA.LOAD_FROM_EMA_ON_START:
        ckpt.add_checkpointable("ema", EMA(ALDITrainer.build_model(cfg), cfg.EMA.ALPHA, cfg.EMA.START_ITER))
    ckpt.resume_or_load(cfg.MODEL.WEIGHTS, resume=resume)
    return model


def plot(path, title, coords, alpha):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        logger.info("matplotlib is not installed: %s not written (the coordinates are in featurespace.npz)", os.path.basename(path))
        return False
    fig, ax = plt.subplots()
    for name, xy in coords.items():
        ax.scatter(xy[:, 0], xy[:, 1], label=name, alpha=alpha, s=1)
    leg = ax.legend(markerscale=4)
    for handle in getattr(leg, "legend_handles", getattr(leg, "legendHandles", [])):
        handle.set_alpha(1)
    ax.set_title(title)
    fig.savefig(path, bbox_inches="tight")
    plt.close(fig)
    return True


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config-file", required=True, metavar="FILE")
    ap.add_argument("--resume", action="store_true", help="load OUTPUT_DIR's last checkpoint instead of MODEL.WEIGHTS")
    ap.add_argument("--pooling", default="avg", choices=("avg", "max"))
    ap.add_argument("opts", nargs=argparse.REMAINDER, help="KEY VALUE pairs merged into the config")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    from aldi_amd.featurespace import LEVELS, FeatureSpaceCollector
    from aldi_amd.trainer import ALDITrainer
    cfg = setup(args)
    names = dataset_names(cfg)
    model = load_model(cfg, args.resume)
    model.eval()
    col = FeatureSpaceCollector(model, pooling=args.pooling, keep_features=True)
    for name in names:
        col.collect(name, ALDITrainer.build_test_loader(cfg, name))
    os.makedirs(cfg.OUTPUT_DIR, exist_ok=True)
    out = {"datasets": np.array(list(names))}
    for level, label, alpha in zip(LEVELS, ("Image", "Proposal"), (0.5, 0.1)):
        res = col.pca(level)
        for key in ("components", "mean", "explained_variance_ratio", "count"):
            out[f"{level}_{key}"] = np.asarray(res[key])
        for i, name in enumerate(names):
            out[f"{level}_coords_{i}"] = res["coords"][name]
        evr = float(np.sum(res["explained_variance_ratio"]))
        logger.info("%s level: %d rows, explained variance ratio %.4f", level, res["count"], evr)
        plot(os.path.join(cfg.OUTPUT_DIR, f"feature_vis_{level}_pca.png"), f"{label}-level PCA (exp. var. {evr:.2f})", res["coords"], alpha)
    path = os.path.join(cfg.OUTPUT_DIR, "featurespace.npz")
    np.savez(path, **out)
    logger.info("wrote %s", path)
    return path


if __name__ == "__main__":
    main()
