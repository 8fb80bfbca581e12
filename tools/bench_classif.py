#!/usr/bin/env python3
"""Side measurement of the classification fine-tuning step (pipeline stage 1) on ONE MI355X: TuneClassif(ResNet-50), the reference's
hyper-parameters (train/classif_finetune_p.py: batch 32, SGD momentum 0.9 wd 5e-4 -- lr see --lr, loss averaged, BatchNorm frozen), a resident
synthetic 224 x 224 set, micro-batch 0 (the whole mini-batch at once, the reference's setting) and micro-batch 8.  Two configurations:

  engines    frozen prefix once per mini-batch(es) on the folded HIP trunk, layer4 on isx.suffix.SuffixEngine, pool -> classifier ->
             cross-entropy on isx.classif_head (all micro-batches in one pass)
  autograd   ISX_CLASSIF_ENGINE=0 ISX_SUFFIX_ENGINE=0: layer4, pool, classifier and loss on torch autograd (MIOpen) per micro-batch behind
             the same HIP prefix -- what the reference itself executes above the frozen layers, the baseline

Per (configuration, micro-batch): ms per optimizer step and images/s, the MEDIAN over the epochs after the first (warm-up: code objects,
workspaces, momentum buffers), device-synchronised at every epoch boundary.  Prints one JSON object.
    python tools/bench_classif.py [--images 512] [--labels 64] [--epochs 5] [--configs engines,autograd] [--micro 0,8]"""
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


def run_config(name, micro, args):
    import utils.train_general as tg
    from model import siamese
    from model.custom_modules import CrossEntropyLoss
    from train import _common as TC
    from train import classif_finetune as cf
    from utils.dataset import synthetic_image_set
    siamese.CLASSIF_ENGINE = siamese.SUFFIX_ENGINE = name == "engines"
    torch.manual_seed(0); random.seed(0)
    P = cf.P
    P.cuda_device, P.cnn_model, P.feature_size2d = 0, args.backbone, (7, 7)
    P.train_epochs, P.train_batch_size, P.train_micro_batch = args.epochs, args.batch, micro
    P.train_loss_int, P.train_test_int, P.train_annealing, P.train_bn = 10 ** 9, 10 ** 9, {}, False
    P.train_lr = args.lr
    TC.drop_resident()
    tr = synthetic_image_set(args.images, args.labels, seed=1)
    cf.labels[:] = sorted(set(l for _, l, _ in tr))
    P.num_classes = len(cf.labels)
    net = cf.get_class_net()
    opt = tg.make_sgd((p for p in net.parameters() if p.requires_grad), P.train_lr, P.train_momentum, P.train_weight_decay)
    marks = []
    real_anneal = tg.anneal

    def marking_anneal(*a, **k):                 # train_gen calls anneal() first thing in every epoch
        torch.cuda.synchronize()
        marks.append(time.perf_counter())
        return real_anneal(*a, **k)
    tg.anneal = marking_anneal
    try:
        cf.train_classif(net, tr, (tr[:8], tr), CrossEntropyLoss(P.train_loss_avg), opt)
    finally:
        tg.anneal = real_anneal
    torch.cuda.synchronize()
    marks.append(time.perf_counter())
    steps = len(tr) // P.train_batch_size
    epochs = [b - a for a, b in zip(marks, marks[1:])][1:]                     # the first epoch is the warm-up
    med = statistics.median(epochs)
    return {"config": name, "micro_batch": micro, "steps_per_epoch": steps, "epochs_measured": len(epochs),
            "ms_per_step": 1e3 * med / steps, "ms_per_step_min": 1e3 * min(epochs) / steps, "ms_per_step_max": 1e3 * max(epochs) / steps,
            "images_per_s": steps * P.train_batch_size / med,
            "classif_engine": net.classif_head_engine() is not None, "suffix_engine": net.suffix_engine() is not None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--labels", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--backbone", default="resnet50")
    # the seeded default-init weights that stand in for ImageNet's overflow within a few steps at the reference's 1e-2 (BatchNorm frozen at
    # identity statistics); the work of a step does not depend on the rate, the default keeps the run finite
    ap.add_argument("--lr", type=float, default=1e-6)
    ap.add_argument("--configs", default="engines,autograd")
    ap.add_argument("--micro", default="0,8")
    args = ap.parse_args()
    if args.epochs < 4:
        ap.error("--epochs >= 4: the first epoch is the warm-up, the median needs three")
    from utils.general import cap_torch_threads
    cap_torch_threads()
    rows = [run_config(c, int(m), args) for m in args.micro.split(",") for c in args.configs.split(",")]
    print(json.dumps({"bench": "classif_finetune_step", "backbone": args.backbone, "images": args.images, "batch": args.batch,
                      "device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
