#!/usr/bin/env python
"""Train or evaluate from a config file: the reference's tools/train_net.py entry point (--config-file, --eval-only, --resume, trailing
KEY VALUE overrides), single process -- a data-parallel launcher is not part of this tool.

  python tools/train_net.py --config-file configs/cityscapes/ALDI-Best-Cityscapes.yaml --dataset-root datasets \\
      DATASETS.TRAIN '("cityscapes_train",)' DATASETS.UNLABELED '("cityscapes_foggy_train",)' DATASETS.TEST '("cityscapes_foggy_val",)'
  python tools/train_net.py --config-file ... --dataset-root datasets --eval-only MODEL.WEIGHTS output/model_final.pth

--dataset-root DIR registers the reference's dataset names under DIR (aldi_amd/datasets.py register_reference_datasets; nothing is read
until a dataset is used) and turns DATASETS.FILES and AUG.DEVICE_WEAK on: the loaders then read those datasets from disk.  Without it
the loaders are the synthetic ones, whatever names the config holds."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config-file", default="", metavar="FILE", help="path to the config file")
    ap.add_argument("--resume", action="store_true", help="resume from the last checkpoint in OUTPUT_DIR")
    ap.add_argument("--eval-only", action="store_true", help="evaluate MODEL.WEIGHTS (or the last checkpoint with --resume) and exit")
    ap.add_argument("--dataset-root", default=None, metavar="DIR", help="register the reference's datasets under DIR and read them (DATASETS.FILES)")
    ap.add_argument("opts", nargs=argparse.REMAINDER, default=[], help="KEY VALUE pairs that override the config")
    return ap.parse_args(argv)


def setup(args):
    from aldi_amd.config import add_aldi_config, get_cfg
    cfg = get_cfg()
    add_aldi_config(cfg)
    if args.config_file:
        cfg.merge_from_file(args.config_file)
    if args.dataset_root is not None:
        from aldi_amd.datasets import register_reference_datasets
        register_reference_datasets(args.dataset_root)
        cfg.merge_from_list(["DATASETS.FILES", True, "AUG.DEVICE_WEAK", True])
    opts = list(args.opts)
    if opts and opts[0] == "--":
        opts = opts[1:]
    cfg.merge_from_list(opts)                                          # (after the switches above: the command line has the last word)
    return cfg


def main(args):
    from aldi_amd.checkpoint import DetectionCheckpointerWithEMA
    from aldi_amd.ema import EMA
    from aldi_amd.trainer import ALDITrainer
    cfg = setup(args)
    if args.eval_only:
        model = ALDITrainer.build_model(cfg)
        ckpt = DetectionCheckpointerWithEMA(model, save_dir=cfg.OUTPUT_DIR)
        if cfg.EMA.ENABLED and cfg.EMA.LOAD_FROM_EMA_ON_START:
            ckpt.add_checkpointable("ema", EMA(ALDITrainer.build_model(cfg), cfg.EMA.ALPHA, cfg.EMA.START_ITER))
        ckpt.resume_or_load(cfg.MODEL.WEIGHTS, resume=args.resume)
        res = ALDITrainer.test(cfg, model)
        if cfg.TEST.AUG.ENABLED:
            res.update(ALDITrainer.test_with_TTA(cfg, model))
        print(res)
        return res
    trainer = ALDITrainer(cfg)
    trainer.resume_or_load(resume=args.resume)
    return trainer.train()


if __name__ == "__main__":
    a = parse_args()
    print("Command Line Args:", a)
    main(a)
