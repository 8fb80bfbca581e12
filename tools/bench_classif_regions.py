#!/usr/bin/env python3
"""Side measurement of the sub-region classifier training step (pipeline stage 2) on ONE MI355X: TuneClassifSub(ResNet-50), the reference's
hyper-parameters (train/classif_regions_p.py: batch 32, micro-batch 1, SGD momentum 0.9 wd 5e-4 -- lr see --lr, loss averaged, BatchNorm
frozen), a resident synthetic 448 x 448 set with its 224 scale.  Two configurations:

  engines    frozen prefix once per scale and mini-batch(es) on the folded HIP trunk, layer4 on isx.suffix.SuffixEngine, box pool -> classifier
             -> cross-entropy over the windows on isx.classif_head (all micro-batches of a scale in one pass)
  autograd   ISX_CLASSIF_ENGINE=0 ISX_SUFFIX_ENGINE=0: layer4, pool, classifier and loss on torch autograd (MIOpen) per micro-batch behind the
             same HIP prefix -- the generic route, the baseline

Per configuration: ms per optimizer step and images/s, the MEDIAN over the epochs after the first (warm-up), device-synchronised at every
epoch boundary; plus the box-pool backward alone at 32 x 14 x 14 x 2048 (HIP events around --pool-calls calls of ops.boxpool_s1_bwd_nhwc,
launch and output allocation included).  Prints one JSON object.
    python tools/bench_classif_regions.py [--images 128] [--labels 16] [--epochs 4] [--configs engines,autograd] [--size 448] [--scales 0,224]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instance-search_amd"))
import torch  # noqa: E402


def run_config(name, args):
    import utils.train_general as tg
    from model import siamese
    from model.custom_modules import CrossEntropyLoss
    from train import _common as TC
    from train import classif_regions as cr
    from utils.dataset import synthetic_image_set
    siamese.CLASSIF_ENGINE = siamese.SUFFIX_ENGINE = name == "engines"
    torch.manual_seed(0); random.seed(0)
    P = cr.P
    P.cuda_device, P.cnn_model, P.feature_size2d, P.bn_model, P.preload_net = 0, args.backbone, (7, 7), "", ""
    P.train_epochs, P.train_batch_size, P.train_micro_batch = args.epochs, args.batch, args.micro
    P.train_loss_int, P.train_test_int, P.train_annealing, P.train_bn = 10 ** 9, 10 ** 9, {}, False
    P.train_lr = args.lr
    TC.drop_resident()
    scales = [int(v) or None for v in args.scales.split(",")]
    plain = synthetic_image_set(args.images, args.labels, (3, args.size, args.size), seed=1)
    tr = cr.multi_scale_items(plain, scales)
    cr.labels[:] = sorted(set(l for _, l, _ in tr))
    P.num_classes = len(cr.labels)
    net = cr.get_class_net()
    opt = tg.make_sgd((p for p in net.parameters() if p.requires_grad), P.train_lr, P.train_momentum, P.train_weight_decay)
    marks = []
    real_anneal = tg.anneal

    def marking_anneal(*a, **k):                 # train_gen calls anneal() first thing in every epoch
        torch.cuda.synchronize()
        marks.append(time.perf_counter())
        return real_anneal(*a, **k)
    tg.anneal = marking_anneal
    try:
        cr.train_classif_subparts(net, tr, (plain[:8], plain[:8]), CrossEntropyLoss(P.train_loss_avg), opt)
    finally:
        tg.anneal = real_anneal
    torch.cuda.synchronize()
    marks.append(time.perf_counter())
    steps = len(tr) // P.train_batch_size
    epochs = [b - a for a, b in zip(marks, marks[1:])][1:]                     # the first epoch is the warm-up
    med = statistics.median(epochs)
    return {"config": name, "micro_batch": args.micro, "steps_per_epoch": steps, "epochs_measured": len(epochs),
            "ms_per_step": 1e3 * med / steps, "ms_per_step_min": 1e3 * min(epochs) / steps, "ms_per_step_max": 1e3 * max(epochs) / steps,
            "images_per_s": steps * P.train_batch_size / med,
            "region_classif_engine": net.classif_head_engine() is not None, "suffix_engine": net.suffix_engine() is not None}


def pool_backward(calls):
    """isx_boxpool_s1_bwd_nhwc at 32 x 14 x 14 x 2048, window 7 x 7: 6.6 MB read + 51.4 MB written per call."""
    from isx import ops
    B, C, H, W, k = 32, 2048, 14, 14, 7
    g = torch.randn(B, H - k + 1, W - k + 1, C, device="cuda").permute(0, 3, 1, 2)
    for _ in range(10):
        ops.boxpool_s1_bwd_nhwc(g, H, W, k, k)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        ops.boxpool_s1_bwd_nhwc(g, H, W, k, k)
    b.record()
    torch.cuda.synchronize()
    us = 1e3 * a.elapsed_time(b) / calls
    nbytes = 4.0 * B * C * (H * W + (H - k + 1) * (W - k + 1))
    return {"shape": [B, H, W, C], "window": [k, k], "calls": calls, "us_per_call": us, "bytes": nbytes, "gb_per_s": nbytes / us / 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--labels", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--micro", type=int, default=1)
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--scales", default="0,224")
    ap.add_argument("--backbone", default="resnet50")
    # the seeded default-init weights that stand in for ImageNet's overflow within a few steps at the reference's rate (BatchNorm frozen at
    # identity statistics); the work of a step does not depend on the rate, the default keeps the run finite
    ap.add_argument("--lr", type=float, default=1e-6)
    ap.add_argument("--configs", default="engines,autograd")
    ap.add_argument("--pool-calls", type=int, default=200)
    args = ap.parse_args()
    if args.epochs < 4:
        ap.error("--epochs >= 4: the first epoch is the warm-up, the median needs three")
    from utils.general import cap_torch_threads
    cap_torch_threads()
    rows = [run_config(c, args) for c in args.configs.split(",")]
    print(json.dumps({"bench": "classif_regions_step", "backbone": args.backbone, "images": args.images, "batch": args.batch, "size": args.size,
                      "scales": args.scales, "device": torch.cuda.get_device_name(0), "rows": rows,
                      "boxpool_s1_bwd_nhwc": pool_backward(args.pool_calls) if args.pool_calls > 0 else None}))


if __name__ == "__main__":
    main()
