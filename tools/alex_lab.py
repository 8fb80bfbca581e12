#!/usr/bin/env python3
"""Times every layer of AlexNet's `features` at B = 256, 224 x 224 (the batch tools/bench_paths.py extracts with) on the HIP route (ISX_ALEX = 1:
libisxalex / libisx, epilogue fused) and on the parent's route (ISX_ALEX = 0: MIOpen + torch ReLU / torch max-pool), and the whole extraction
`extract_global_alexnet_224` of tools/bench_paths.py under ISX_ALEX = 0, 1 and auto.  What model/nn_utils._ALEX_AUTO_KINDS is decided from.

    python tools/alex_lab.py [--calls N] [--no-e2e]        one JSON object on the last line

Per layer both routes run in ONE process on the same input, alternating call by call after a warm-up of both (MIOpen picks its algorithm on the
first call of a shape): device events around each call, median / min / max of >= 30 calls per route.  A convolution is timed WITH the ReLU behind it
(the HIP route fuses it; the parent's route runs torch's in-place ReLU as a second pass) and, as `+pool`, with the pool behind that.  The rule for
`auto`: a layer kind goes native only if its median is no slower than the parent route's median by more than the parent route's own min-max spread.
End to end every mode runs in a process of its own (the mode is read when model.nn_utils is imported)."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instance-search_amd"))

B = int(os.environ.get("LAB_B", "256"))
# (name, kind, Cin, H of the input map, and for a convolution Cout, K, stride, pad)
LAYERS = [("conv1 11x11/4 3->64 @224", "conv11", 3, 224, 64, 11, 4, 2), ("pool1 64 @55", "pool", 64, 55),
          ("conv2 5x5 64->192 @27", "conv5", 64, 27, 192, 5, 1, 2), ("pool2 192 @27", "pool", 192, 27),
          ("conv3 3x3 192->384 @13", "conv3", 192, 13, 384, 3, 1, 1), ("conv4 3x3 384->256 @13", "conv3", 384, 13, 256, 3, 1, 1),
          ("conv5 3x3 256->256 @13", "conv3", 256, 13, 256, 3, 1, 1), ("pool3 256 @13", "pool", 256, 13)]


def _stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": len(ms)}


def time_pair(torch, f_new, f_old, calls):
    """Both routes alternating; returns (stats of the new route, stats of the parent's)."""
    for _ in range(5):
        f_new(); f_old()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(calls):
        for which, f in enumerate((f_new, f_old)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[which].append(a.elapsed_time(b))
    return _stats(ms[0]), _stats(ms[1])


def layers(calls):
    import torch
    import torch.nn as nn
    from model import nn_utils
    out = {}
    torch.manual_seed(0)

    def routes(mods):
        """The same modules folded under ISX_ALEX = 1 and = 0 (the mode is read at fold time and at every forward: set around both)."""
        built = {}
        for mode in ("1", "0"):
            nn_utils._ALEX_MODE = mode
            built[mode] = nn_utils.fold_batch_norm(nn.Sequential(*mods)).cuda().to(memory_format=torch.channels_last)

        def run(mode, x):
            nn_utils._ALEX_MODE = mode
            return built[mode](x)
        return run

    with torch.no_grad():
        for spec in LAYERS:
            name, kind, Cin, H = spec[:4]
            x = torch.relu(torch.randn(B, Cin, H, H, device="cuda")).contiguous(memory_format=torch.channels_last)
            if kind == "pool":
                run = routes([nn.MaxPool2d(3, 2)])
                new, old = time_pair(torch, lambda: run("1", x), lambda: run("0", x), calls)
                same = torch.equal(run("1", x), run("0", x))
                nbytes = 4.0 * B * Cin * (H * H + ((H - 3) // 2 + 1) ** 2)
                out[name] = {"kind": kind, "hip": new, "parent": old, "same_bits": same, "hip_GBps": nbytes / new["median_ms"] / 1e6}
            else:
                Cout, K, s, p = spec[4:]
                conv = nn.Conv2d(Cin, Cout, K, s, p)
                Ho = (H + 2 * p - K) // s + 1
                run = routes([conv, nn.ReLU(inplace=True)])
                new, old = time_pair(torch, lambda: run("1", x), lambda: run("0", x), calls)
                a, b = run("1", x).double(), run("0", x).double()
                flop = 2.0 * B * Ho * Ho * K * K * Cin * Cout
                out[name] = {"kind": kind, "hip": new, "parent": old, "max_abs_diff_over_max": float((a - b).abs().max() / b.abs().max()),
                             "hip_TFLOPs": flop / new["median_ms"] / 1e9, "parent_TFLOPs": flop / old["median_ms"] / 1e9}
                if Ho >= 3 and name[:5] in ("conv1", "conv2", "conv5"):
                    # the un-fused round trip: convolution (+ ReLU) and the pool behind it as two calls against MIOpen + ReLU + torch's pool
                    runp = routes([conv, nn.ReLU(inplace=True), nn.MaxPool2d(3, 2)])
                    newp, oldp = time_pair(torch, lambda: runp("1", x), lambda: runp("0", x), calls)
                    out[name + " +pool"] = {"kind": kind + "+pool", "hip": newp, "parent": oldp}
            r = out[name]
            print("%-28s hip %8.3f ms [%7.3f .. %7.3f]   parent %8.3f ms [%7.3f .. %7.3f]" % (name, r["hip"]["median_ms"], r["hip"]["min_ms"], r["hip"]["max_ms"],
                  r["parent"]["median_ms"], r["parent"]["min_ms"], r["parent"]["max_ms"]), flush=True)
            del x
    # the rule for `auto`, per kind over the layers of that kind (the medians and the parent's spreads added up)
    verdict = {}
    for kind in ("conv11", "conv5", "conv3", "pool"):
        rows = [r for r in out.values() if r["kind"] == kind]
        hip, par = sum(r["hip"]["median_ms"] for r in rows), sum(r["parent"]["median_ms"] for r in rows)
        spread = sum(r["parent"]["max_ms"] - r["parent"]["min_ms"] for r in rows)
        verdict[kind] = {"hip_ms": hip, "parent_ms": par, "parent_spread_ms": spread, "native_by_rule": hip <= par + spread}
    return {"layers": out, "auto_rule": verdict}


def e2e_child():
    """extract_global_alexnet_224 of tools/bench_paths.py under this process's ISX_ALEX; one JSON line."""
    import time
    import torch
    from isx import backbones, ops
    from model.nn_utils import alex_route_active, fold_batch_norm
    from model.siamese import TuneClassif
    with torch.no_grad():
        x = torch.randn(B, 3, 224, 224, device="cuda").to(memory_format=torch.channels_last)
        a = TuneClassif(backbones.alexnet(pretrained=True), 464).eval()
        folded = alex_route_active(a.features)
        if folded:
            a.features = fold_batch_norm(a.features)
        a = a.cuda().to(memory_format=torch.channels_last)
        a.classifier = torch.nn.Sequential()
        f = lambda: ops.l2norm_rows(a(x))
        for _ in range(5):
            f()
        torch.cuda.synchronize()
        rates = []
        for _ in range(7):                                   # seven windows of ~0.3 s or more
            n, t = 0, time.perf_counter()
            while n < 10 or time.perf_counter() - t < 0.3:
                f()
                n += 1
                if n % 10 == 0:
                    torch.cuda.synchronize()
            torch.cuda.synchronize()
            rates.append(B * n / (time.perf_counter() - t))
    print(json.dumps({"mode": os.environ.get("ISX_ALEX", "auto"), "folded": folded, "images_per_s_median": statistics.median(rates),
                      "images_per_s_min": min(rates), "images_per_s_max": max(rates)}))


def main():
    if "--e2e-child" in sys.argv:
        return e2e_child()
    calls = int(sys.argv[sys.argv.index("--calls") + 1]) if "--calls" in sys.argv else 40
    result = {}
    if "--no-e2e" not in sys.argv:                            # first: this process has not touched the GPU yet, one process holds it at a time
        result["extract_global_alexnet_224"] = {}
        for mode in ("0", "1", "auto", "0", "1"):             # the two fixed routes twice: the second pass shows the spread between processes
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--e2e-child"], env=dict(os.environ, ISX_ALEX=mode), capture_output=True, text=True,
                                 timeout=300)
            if run.returncode != 0:
                print(run.stdout + run.stderr, flush=True)
                raise SystemExit("the ISX_ALEX=%s child ended with status %d: nothing more is started" % (mode, run.returncode))
            line = json.loads(run.stdout.strip().splitlines()[-1])
            result["extract_global_alexnet_224"].setdefault(mode, []).append(line)
            print("extract_global_alexnet_224 ISX_ALEX=%-4s folded=%-5s %9.1f images/s [%9.1f .. %9.1f]" % (mode, line["folded"], line["images_per_s_median"],
                  line["images_per_s_min"], line["images_per_s_max"]), flush=True)
    result.update(layers(max(calls, 30)))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
