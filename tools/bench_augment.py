#!/usr/bin/env python3
"""Side measurement of the training-time augmentation (isx_affine_noisy_u8, csrc/augment.hip) on ONE MI355X.  Three figures, one JSON line:

  kernels    the three launches of one call alone at 192 x 224 x 224 (a 64-triplet step's images) out of a resident set through `rows`: median of
             the timed calls after warm-up (device events around each call), and the algorithmic bytes over that time against 8 TB/s of HBM
  host       the numpy route (utils.image.affine_noisy, what --device=-1 runs) on images of the same set, per image
  training   the train.siamese_descriptor step of tools/bench_train.py's reference configuration, three ways: as bench_train measures it
             (pre-processed set, frozen prefix of 8 mini-batches per launch), the same with P.train_prefix_ahead = 1 (what an augmented run can
             use: its batches cannot be built ahead of their turn), and with --augment=reference

    python tools/bench_augment.py [--batch 192] [--size 224] [--calls 30] [--epochs 5] [--skip-training]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instance-search_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_BYTES_PER_S = 8e12


def median(v):
    return sorted(v)[len(v) // 2]


def bench_kernels(args):
    from isx import ops
    from utils.image import random_affine_noisy_cv
    B, S = args.batch, args.size
    g = torch.Generator().manual_seed(0)
    resident = torch.randint(0, 256, (512, S, S, 3), generator=g, dtype=torch.uint8).cuda()
    aug = random_affine_noisy_cv(rotation=45, hs_range=.25, vs_range=.25, h_flip=True)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    times = []
    for call in range(args.warmup + args.calls):
        keys = np.stack([np.full(B, 1), np.full(B, call), np.arange(B), np.zeros(B, int)], 1)
        mats, ids = aug.plan(keys, S, S)
        rows = torch.randint(0, 512, (B,), generator=g).cuda()
        mats_d, ids_d = torch.from_numpy(mats).cuda(), torch.from_numpy(ids).cuda()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.affine_noisy(resident, rows, mats_d, 1, ids_d, mean, std, channels_last=True)
        e1.record()
        torch.cuda.synchronize()
        if call >= args.warmup:
            times.append(e0.elapsed_time(e1))
    px = B * S * S * 3
    # uint8 in; coefficients written by the column pass, read and written by the row pass, read (as 16 taps, mostly from cache) by the warp; fp32 out
    moved = px * (1 + 8 + 16 + 8 + 4)
    ms = median(times)
    return {"shape": [B, S, S], "calls": len(times), "ms_median": ms, "ms_min_max": [min(times), max(times)], "algorithmic_bytes": moved,
            "bytes_per_s": moved / (ms * 1e-3), "frac_of_hbm_8TBps": moved / (ms * 1e-3) / HBM_BYTES_PER_S,
            "includes": "workspace allocation from torch's caching allocator + three launches; parameters already on the device"}, resident


def bench_host(args, resident):
    from utils.image import affine_noisy, random_affine_noisy_cv
    aug = random_affine_noisy_cv(rotation=45, hs_range=.25, vs_range=.25, h_flip=True)
    imgs = resident[:args.host_images].cpu().numpy()
    mats, ids = aug.plan(np.stack([np.full(len(imgs), 1), np.zeros(len(imgs), int), np.arange(len(imgs)), np.zeros(len(imgs), int)], 1), args.size, args.size)
    affine_noisy(imgs[0], mats[0], 1, int(ids[0]))
    times = []
    for i in range(len(imgs)):
        t0 = time.perf_counter()
        affine_noisy(imgs[i], mats[i], 1, int(ids[i]))
        times.append(1e3 * (time.perf_counter() - t0))
    return {"ms_per_image_median": median(times), "ms_per_image_min_max": [min(times), max(times)], "images": len(times),
            "ms_per_step_of_%d_images" % args.batch: median(times) * args.batch}


def bench_training(args):
    import bench_train as BT
    import utils.dataset as D
    from train import _common as TC
    from train import siamese_descriptor as sd
    ns = BT.make_parser().parse_args(["--epochs", str(args.epochs), "--configs", "reference"])
    real = D.synthetic_image_set
    out = {}
    for name, ahead, augment in (("plain", None, False), ("plain_prefix_ahead_1", 1, False), ("augmented", None, True)):
        default_ahead = sd.P.train_prefix_ahead
        try:
            ns.prefix_ahead = ahead
            if augment:
                D.synthetic_image_set = lambda *a, **k: TC._raw_u8_set(real(*a, **k))
                sd.P.train_pre_proc, sd.P.train_trans = False, TC.parse_augment("reference")
            r = BT.run_config("reference", ns, 1, 0, 0)
        finally:
            D.synthetic_image_set = real
            sd.P.train_pre_proc, sd.P.train_trans, sd.P.train_prefix_ahead = True, None, default_ahead
            TC.drop_resident()
        steps = r["optimizer_steps_per_epoch"]
        out[name] = {"ms_per_step": r["ms_per_step"], "ms_per_step_min_max": r["ms_per_step_min_max"], "triplets_per_s": r["triplets_per_s"],
                     "epoch_seconds": r["epoch_seconds"], "optimizer_steps_per_epoch": steps, "statistic": r["statistic"]}
    p, a = out["plain"], out["augmented"]
    spread = (p["ms_per_step_min_max"][1] - p["ms_per_step_min_max"][0]) / p["ms_per_step"]
    out["augmented_over_plain"] = a["ms_per_step"] / p["ms_per_step"]
    out["augmented_over_plain_prefix_ahead_1"] = a["ms_per_step"] / out["plain_prefix_ahead_1"]["ms_per_step"]
    out["plain_epoch_to_epoch_spread"] = spread
    out["within_acceptance"] = bool(out["augmented_over_plain"] <= 1.0 + max(0.10, spread))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=192)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-images", type=int, default=6)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--skip-training", action="store_true")
    args = ap.parse_args()
    from utils.general import cap_torch_threads
    cap_torch_threads()
    torch.cuda.set_device(0)
    line = {}
    line["kernels"], resident = bench_kernels(args)
    line["host"] = bench_host(args, resident)
    del resident
    torch.cuda.empty_cache()
    if not args.skip_training:
        line["training"] = bench_training(args)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
