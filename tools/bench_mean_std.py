#!/usr/bin/env python3
"""Side measurement of the dataset statistics (isxp_channel_moments_u8, csrc/prep.hip; create_mean_std_file.py) on ONE MI355X.  One JSON line:

  kernel     isx.prep.channel_moments_u8 alone on a resident (B,224,224,3) uint8 block, B = 4096 (616 MB: past the 256 MiB Infinity Cache, an
             HBM stream) and B = 192 (a training step's images, 29 MB: cache resident after the first call): device events around `calls`
             back-to-back calls, median over `repeats` after warm-up, and the bytes READ over that time.  Baseline in the same run on the same
             block, alternating with it: isx.ops.images_u8_to_f32, which reads the same bytes and writes four per byte read.
  tool       create_mean_std_file.collect_moments on a resident synthetic set of 4096 images, --device=0 against --device=-1 (wall clock, the
             device synchronised), and the same tool on a folder of JPEGs written from that set, with the share of its time spent in decode.

    python tools/bench_mean_std.py [--sizes 4096,192] [--calls 20] [--repeats 15] [--tool-images 4096] [--folder-images 2048]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instance-search_amd"))
import torch  # noqa: E402

HBM_READ_BYTES_PER_S = 6.3e12          # what a read stream achieves on this chip (8 TB/s is the specification)


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn, calls, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return out


def bench_kernel(B, args):
    from isx import ops, prep
    g = torch.Generator().manual_seed(B)
    img = torch.randint(0, 256, (B, 224, 224, 3), generator=g, dtype=torch.uint8).cuda()
    out = torch.empty((B, 3, 2), dtype=torch.int64, device="cuda")
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    moments = lambda: prep.channel_moments_u8(img, out=out)
    baseline = lambda: ops.images_u8_to_f32(img, mean, std)
    t_m, t_b = [], []
    for _ in range(3):                                       # alternate the two, so that a drift of the box hits both
        t_m += timed(moments, args.calls, args.repeats // 3)
        t_b += timed(baseline, args.calls, args.repeats // 3)
    want = prep.channel_moments_u8_host(img[:2].cpu())
    assert torch.equal(out[:2].cpu(), want), "the timed kernel does not give the host's integers"
    nbytes = img.numel()
    ms, mb = median(t_m), median(t_b)
    return {"shape": [B, 224, 224, 3], "bytes_read": nbytes, "calls_per_sample": args.calls, "samples": len(t_m),
            "moments_ms_median": ms, "moments_ms_min_max": [min(t_m), max(t_m)], "moments_read_GBps": nbytes / (ms * 1e-3) / 1e9,
            "moments_frac_of_read_stream_6.3TBps": nbytes / (ms * 1e-3) / HBM_READ_BYTES_PER_S,
            "images_u8_to_f32_ms_median": mb, "images_u8_to_f32_ms_min_max": [min(t_b), max(t_b)],
            "images_u8_to_f32_read_GBps": nbytes / (mb * 1e-3) / 1e9, "images_u8_to_f32_bytes_written": 4 * nbytes,
            "moments_over_baseline": ms / mb,
            "includes": "the memset of the 48 B per image and one launch (moments); the allocation of the fp32 output from torch's caching "
                        "allocator and one launch (baseline)"}


def bench_tool(args):
    import create_mean_std_file as T
    from isx import prep
    g = torch.Generator().manual_seed(7)
    n, batch = args.tool_images, 256
    images = list(torch.randint(0, 256, (n, 224, 224, 3), generator=g, dtype=torch.uint8))
    parts = [images[a:a + batch] for a in range(0, n, batch)]
    res = {"images": n, "batch": batch}
    got = {}
    for name, device in (("device_0", 0), ("device_-1", -1)):
        if device >= 0:
            T.collect_moments(parts[:1], batch, device)        # pinned block, code object
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got[name] = T.collect_moments(parts, batch, device)
        torch.cuda.synchronize()
        res[name + "_seconds"] = time.perf_counter() - t0
    assert torch.equal(got["device_0"][0], got["device_-1"][0]), "device and host integers differ"
    res["mean_std"] = prep.mean_std(got["device_0"][0], got["device_0"][1])
    res["host_over_device"] = res["device_-1_seconds"] / res["device_0_seconds"]
    if args.folder_images > 0:
        from PIL import Image
        with tempfile.TemporaryDirectory() as d:
            for i, im in enumerate(images[:args.folder_images]):
                Image.fromarray(im.numpy()).save(os.path.join(d, "c%03d-%05d.jpg" % (i % 8, i)), quality=90)
            timer = {"decode": 0.0, "moments": 0.0}
            t0 = time.perf_counter()
            T.collect_moments(T._folder_images(d, batch, timer), batch, 0, timer)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        res["folder"] = {"jpeg_files": args.folder_images, "seconds": wall, "decode_seconds": timer["decode"], "moments_seconds": timer["moments"],
                         "decode_share": timer["decode"] / wall}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,192")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--tool-images", type=int, default=4096)
    ap.add_argument("--folder-images", type=int, default=2048)
    args = ap.parse_args()
    from utils.general import cap_torch_threads
    cap_torch_threads()
    torch.cuda.set_device(0)
    line = {"kernel": [bench_kernel(int(b), args) for b in args.sizes.split(",")]}
    torch.cuda.empty_cache()
    if args.tool_images > 0:
        line["tool"] = bench_tool(args)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
