#!/usr/bin/env python3
"""Side measurement of the region-descriptor siamese training step (pipeline stage 3) on ONE MI355X: RegionDescriptorNet(TuneClassifSub(
ResNet-50)), the reference's hyper-parameters (train/siamese_regions_p.py: k = 6 windows, feature_dim 2048, micro-batch 1, BatchNorm frozen --
lr see --lr), a resident synthetic 448 x 448 set; batch and epoch length small enough that the generic route finishes in minutes.  Two
configurations:

  engines    frozen prefix once per mini-batch(es) on the folded HIP trunk, layer4 on isx.suffix.SuffixEngine, everything behind it with both
             losses on isx.region_head.RegionHeadEngine (all triplets of the step in one pass, the 822 MB Linear on one row per image)
  generic    ISX_REGION_ENGINE=0 ISX_SUFFIX_ENGINE=0: the whole net on torch autograd (MIOpen), triplet by triplet, every window through the
             Linear on its own -- the route the stage took before, the baseline

Per configuration: ms per optimizer step and triplets/s, the MEDIAN over the epochs after the first (warm-up); an epoch is timed from the end
of its mining pass (train_gen's begin_epoch) to the start of the next epoch, device-synchronised at both ends.  Plus the two region kernels alone
at 192 x 14 x 14 x 2048, k = 6 (HIP events around --kernel-calls calls of the ops wrappers, launches and output allocation included), in us per
call and GB/s of the bytes the call has to move.  Prints one JSON object.
    python tools/bench_siamese_regions.py [--images 32] [--labels 8] [--batch 8] [--epochs 4] [--configs engines,generic] [--size 448]"""
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
    from train import _common as TC
    from train import siamese_regions as sr
    from utils.dataset import synthetic_image_set
    siamese.REGION_ENGINE = siamese.SUFFIX_ENGINE = name == "engines"
    torch.manual_seed(0); random.seed(0)
    P = sr.P
    P.cuda_device, P.cnn_model, P.feature_size2d, P.classif_model, P.preload_net = 0, args.backbone, (7, 7), "", ""
    P.feature_dim, P.regions_k = args.feature_dim, args.k
    P.train_epochs, P.train_batch_size, P.train_seed = args.epochs, args.batch, 1
    P.train_loss_int, P.train_test_int, P.train_annealing, P.train_bn, P.test_upfront = 10 ** 9, 10 ** 9, {}, False, False
    P.train_lr = args.lr
    TC.drop_resident()
    tr = synthetic_image_set(args.images, args.labels, (3, args.size, args.size), seed=1, structure=0.5)
    starts, ends, routes = [], [], []
    real_anneal, real_begin, real_route = tg.anneal, tg._Stepper.begin_epoch, tg._Stepper._route

    def marking_anneal(*a, **k):                 # train_gen calls anneal() first thing in every epoch: the end of the epoch before
        torch.cuda.synchronize()
        ends.append(time.perf_counter())
        return real_anneal(*a, **k)

    def marking_begin(self, *a, **k):            # ... and begin_epoch() once the epoch's mining pass has produced its triplets
        torch.cuda.synchronize()
        starts.append(time.perf_counter())
        return real_begin(self, *a, **k)

    def noting_route(self, *a, **k):
        r = real_route(self, *a, **k)
        routes.append(r is not None)
        return r
    tg.anneal, tg._Stepper.begin_epoch, tg._Stepper._route = marking_anneal, marking_begin, noting_route
    # evaluation between and after the epochs is not part of the step
    real_test = sr.test_print_descriptor
    sr.test_print_descriptor = lambda *a, **k: 0
    try:
        net, _ = sr.main(tr, tr, tr[:8])
    finally:
        tg.anneal, tg._Stepper.begin_epoch, tg._Stepper._route, sr.test_print_descriptor = real_anneal, real_begin, real_route, real_test
    torch.cuda.synchronize()
    ends.append(time.perf_counter())
    steps = len(routes) // args.epochs
    epochs = [e - s for s, e in zip(starts, ends[1:])][1:]                     # ends[0] precedes the first epoch; the first epoch is the warm-up
    med = statistics.median(epochs)
    return {"config": name, "steps_per_epoch": steps, "epochs_measured": len(epochs), "ms_per_step": 1e3 * med / steps,
            "ms_per_step_min": 1e3 * min(epochs) / steps, "ms_per_step_max": 1e3 * max(epochs) / steps, "triplets_per_s": steps * args.batch / med,
            "engine_route_steps": sum(routes), "steps": len(routes)}


def kernels(calls):
    """isx_region_sum_l2_nhwc / isx_region_sum_l2_bwd_nhwc at 192 x 14 x 14 x 2048, window 7 x 7, k = 6, as the region head calls them (the
    class term for every third image: the anchors).  Bytes a call has to move: forward the map read + the rows written (+ Shift); backward the
    map and g read, the class term of a third of the images read, the gradient map written."""
    from isx import ops
    B, C, H, W, kh, k = 192, 2048, 14, 14, 7, 6
    Wp = W - kh + 1
    F_ = C * kh * kh
    x = torch.relu(torch.randn(B, H, W, C, device="cuda")).permute(0, 3, 1, 2)
    idx = torch.stack([torch.randperm(Wp * Wp, device="cuda")[:k] for _ in range(B)])
    shift = torch.randn(F_, device="cuda") * 1e-3
    g = torch.randn(B, F_, device="cuda") * F_ ** -0.5
    add = torch.randn(B // 3, H, W, C, device="cuda").permute(0, 3, 1, 2) * 1e-3
    rows, n2 = ops.region_sum_l2_nhwc(x, kh, kh, idx, Wp, shift)
    out = {}
    for name, fn, nbytes in (("region_sum_l2_nhwc", lambda: ops.region_sum_l2_nhwc(x, kh, kh, idx, Wp, shift), 4.0 * (B * H * W * C + B * F_ + F_)),
                             ("region_sum_l2_bwd_nhwc", lambda: ops.region_sum_l2_bwd_nhwc(x, g, n2, kh, kh, idx, Wp, add=add, add_every=3),
                              4.0 * (2 * B * H * W * C + B // 3 * H * W * C + B * F_))):
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        us = 1e3 * a.elapsed_time(b) / calls
        out[name] = {"shape": [B, H, W, C], "window": [kh, kh], "k": k, "calls": calls, "us_per_call": us, "bytes": nbytes, "gb_per_s": nbytes / us / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--labels", type=int, default=8)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--feature-dim", type=int, default=2048)
    ap.add_argument("--backbone", default="resnet50")
    # the seeded default-init weights that stand in for ImageNet's overflow within a few steps at the reference's rate (BatchNorm frozen at
    # identity statistics); the work of a step does not depend on the rate, the default keeps the run finite
    ap.add_argument("--lr", type=float, default=1e-9)
    ap.add_argument("--configs", default="engines,generic")
    ap.add_argument("--kernel-calls", type=int, default=50)
    args = ap.parse_args()
    if args.epochs < 4:
        ap.error("--epochs >= 4: the first epoch is the warm-up, the median needs three")
    from utils.general import cap_torch_threads
    cap_torch_threads()
    rows = [run_config(c, args) for c in args.configs.split(",") if c]
    print(json.dumps({"bench": "siamese_regions_step", "backbone": args.backbone, "images": args.images, "batch": args.batch, "size": args.size,
                      "k": args.k, "feature_dim": args.feature_dim, "device": torch.cuda.get_device_name(0), "rows": rows,
                      "kernels": kernels(args.kernel_calls) if args.kernel_calls > 0 else None}))


if __name__ == "__main__":
    main()
