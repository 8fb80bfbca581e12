#!/usr/bin/env python3
"""Side measurement of the cubic resize of 8-bit images (isxs_resize_cubic_u8, csrc/scale.hip; pre_process_dataset.py) on ONE MI355X.  One
JSON line:

  kernel     isx.scale.resize_cubic_u8 alone on a resident uint8 block, three shapes: (a) 192 x 448 x 448 -> 224 x 224, the second scale of
             train.classif_regions; (b) 64 x 1080 x 1920 -> 448 x 796; (c) 64 x 300 x 1000 padded to 500 x 1000 (max_ar = 2) -> 448 x 896.
             Device events around `calls` back-to-back calls, median and range over `repeats` after warm-up, and the bytes read (the source,
             once) plus written over that time, against the 6.3 TB/s read stream of this chip.  Baseline in the same run on the same block,
             alternating with it: what the second scale was before -- isx.ops.images_u8_to_f32, then torch's bicubic interpolate of the fp32
             tensor (for (c) on the unpadded block to the same output size: the same traffic, not the same operation).
  pil        PIL's Image.resize(BICUBIC) per image on the host, the stand-in for the reference's per-image cv2.resize loop: NOT the same
             pixels (PIL widens its kernel when it reduces), `pil_images` images per shape, scaled to the block.
  tool       pre_process_dataset end to end on a folder of JPEGs, --device=0, with the decode, resize and encode shares of its wall clock.

    python tools/bench_resize.py [--calls 10] [--repeats 15] [--pil-images 8] [--folder-images 256]"""
import argparse
import contextlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instance-search_amd"))
import torch  # noqa: E402

HBM_READ_BYTES_PER_S = 6.3e12          # what a read stream achieves on this chip (8 TB/s is the specification)
SHAPES = [("a_stage2_second_scale", 192, 448, 448, None, 224), ("b_full_hd", 64, 1080, 1920, None, 448), ("c_padded", 64, 300, 1000, 2.0, 448)]


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


def bench_kernel(name, B, Hs, Ws, max_ar, short, args):
    from PIL import Image
    from isx import ops, scale
    g = torch.Generator().manual_seed(B + Hs)
    img = torch.randint(0, 256, (B, Hs, Ws, 3), generator=g, dtype=torch.uint8).cuda()
    pad = scale.aspect_pad(Hs, Ws, max_ar) if max_ar else (0, 0, Hs, Ws)
    Hd, Wd = scale.short_side_size(pad[2], pad[3], short)
    ids = torch.arange(B, dtype=torch.int64, device="cuda")
    out = torch.empty((B, Hd, Wd, 3), dtype=torch.uint8, device="cuda")
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    resize = lambda: scale.resize_cubic_u8(img, (Hd, Wd), pad=pad, seed=1, noise_ids=ids, out=out)
    baseline = lambda: torch.nn.functional.interpolate(ops.images_u8_to_f32(img, mean, std), size=(Hd, Wd), mode="bicubic", align_corners=False)
    t_r, t_b = [], []
    for _ in range(3):                                       # alternate the two, so that a drift of the box hits both
        t_r += timed(resize, args.calls, args.repeats // 3)
        t_b += timed(baseline, args.calls, args.repeats // 3)
    want = scale.resize_cubic_u8_host(img[:1].cpu(), (Hd, Wd), pad=pad, seed=1, noise_ids=[0])
    assert torch.equal(out[:1].cpu(), want), "the timed kernel does not give the host's bytes"
    moved = img.numel() + out.numel()
    ms, mb = median(t_r), median(t_b)
    res = {"case": name, "src": [B, Hs, Ws, 3], "pad": list(pad), "dst": [B, Hd, Wd, 3], "bytes_read_plus_written": moved,
           "calls_per_sample": args.calls, "samples": len(t_r),
           "resize_ms_median": ms, "resize_ms_min_max": [min(t_r), max(t_r)], "resize_GBps": moved / (ms * 1e-3) / 1e9,
           "resize_frac_of_read_stream_6.3TBps": moved / (ms * 1e-3) / HBM_READ_BYTES_PER_S,
           "fp32_route_ms_median": mb, "fp32_route_ms_min_max": [min(t_b), max(t_b)], "resize_over_fp32_route": ms / mb,
           "fp32_route": "ops.images_u8_to_f32 + interpolate(bicubic) on the %s block; its fp32 tensors come from torch's caching allocator"
                         % ("unpadded" if max_ar else "same")}
    if args.pil_images > 0:
        host = img[:args.pil_images].cpu().numpy()
        t0 = time.perf_counter()
        for a in host:
            Image.fromarray(a).resize((Wd, Hd), Image.BICUBIC)
        per = (time.perf_counter() - t0) / len(host)
        res.update({"pil_bicubic_ms_per_image": per * 1e3, "pil_bicubic_ms_for_the_block": per * 1e3 * B,
                    "pil_note": "not the same pixels: no padding, and PIL widens the kernel when it reduces"})
    return res


def bench_tool(args):
    from PIL import Image
    import pre_process_dataset as T
    from train import _decode_farm
    g = torch.Generator().manual_seed(11)
    n = args.folder_images
    with tempfile.TemporaryDirectory() as d:
        src, out = os.path.join(d, "set"), os.path.join(d, "out")
        os.makedirs(src)
        for i in range(n):
            small = torch.rand((1, 3, 30, 40), generator=g)
            H, W = (600, 800) if i % 16 else (300, 1000)         # one in sixteen is beyond the ratio
            big = torch.nn.functional.interpolate(small, size=(H, W), mode="bilinear", align_corners=False)[0]
            Image.fromarray((big * 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()).save(os.path.join(src, "c%03d-%05d.jpg" % (i % 8, i)), quality=90)
        try:
            with contextlib.redirect_stdout(sys.stderr):     # code object, decoder processes; the tool's own report is not part of the JSON line
                T.main(["--dataset=" + src, "--out=" + os.path.join(d, "warm"), "--device=0", "--batch=64"])
            timer = {"decode": 0.0, "resize": 0.0, "encode": 0.0}
            a = argparse.Namespace(batch=64, max_ar=2.0, short_side=448, size=None, device=0, seed=0)
            t0 = time.perf_counter()
            written = T.process_folder(src, out, a, timer)
            torch.cuda.synchronize()
            wall = time.perf_counter() - t0
        finally:
            _decode_farm.shutdown()
    return {"jpeg_files": n, "written": len(written), "seconds": wall, "decode_seconds": timer["decode"], "resize_seconds": timer["resize"],
            "encode_seconds": timer["encode"], "decode_share": timer["decode"] / wall, "resize_share": timer["resize"] / wall,
            "encode_share": timer["encode"] / wall, "resize_includes": "stacking the run, the copies to and from the device, the launch"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--pil-images", type=int, default=8)
    ap.add_argument("--folder-images", type=int, default=256)
    args = ap.parse_args()
    from utils.general import cap_torch_threads
    cap_torch_threads()
    torch.cuda.set_device(0)
    line = {"kernel": []}
    for shape in SHAPES:
        line["kernel"].append(bench_kernel(*shape, args))
        torch.cuda.empty_cache()
    if args.folder_images > 0:
        line["tool"] = bench_tool(args)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
