"""Pipeline stage 0: write the mean/std file of a dataset's TRAINING images -- the file every entry point reads through
train.global_p.mean_std_files[dataset id] before it decodes its first image (reference create_mean_std_file.py).

    python -m create_mean_std_file --dataset=<folder | synthetic:...> [--out=FILE] [--device=0] [--batch=256] [--per-image]

The images of <folder> itself (not its `test` sub-folder) stream through the decoder processes of train/_decode_farm.py, at most --batch decoded
at a time; consecutive images of one shape go to the device as one pinned block and through one isx.prep.channel_moments_u8 launch.  What is
kept per image is six integers and a pixel count, so nothing grows with the dataset but that table (the reference holds every image in fp32),
and the integers make the result independent of --batch and of --device: --device=-1 adds the same integers on the host and writes the same
bytes.  Convention (isx.prep.mean_std): pooled when every image has one shape, per image otherwise or with --per-image."""
from __future__ import print_function

import argparse
import os
import sys
import time

import torch

from isx import prep


def _synthetic_images(spec, batch):
    from test._common import load_sets
    from train._common import _raw_u8_set
    _, ref = load_sets(spec, [])
    images = [im for im, _, _ in _raw_u8_set(ref)]
    return [images[a:a + batch] for a in range(0, len(images), batch)]


def _folder_images(folder, batch, timer):
    """The decoded (H,W,3) uint8 images of `folder` in lists of at most `batch`: one list is alive at a time."""
    from test._common import imread_rgb, to_raw_tensor
    from train import _decode_farm as DF
    from utils import get_images_labels
    files = [f for f, _ in get_images_labels(folder)]
    if not files:
        return
    t0 = time.perf_counter()
    first = to_raw_tensor(imread_rgb(files[0]))
    slot = max(1 << 20, 2 * first.numel())                  # a ragged folder: a file larger than the slot is decoded in this process
    farm = DF.decode_farm()
    timer["decode"] += time.perf_counter() - t0
    for a in range(0, len(files), batch):
        t0 = time.perf_counter()
        part = files[a:a + batch]
        images = DF.decode_files(part, slot) if farm is not None else [to_raw_tensor(imread_rgb(f)) for f in part]
        timer["decode"] += time.perf_counter() - t0
        yield images
        del images


def _runs(images):
    """Runs of consecutive images of one shape."""
    run = []
    for im in images:
        if run and im.shape != run[0].shape:
            yield run
            run = []
        run.append(im)
    if run:
        yield run


def collect_moments(parts, batch, device, timer=None):
    """((N,3,2) int64 moments, (N,) pixel counts, set of image shapes) of (H,W,3) uint8 CPU tensors that arrive in lists of at most `batch`."""
    timer = timer if timer is not None else {"decode": 0.0, "moments": 0.0}
    moments, pixels, shapes = [], [], set()
    pinned = None
    for run in (r for part in parts for r in _runs(part)):
        t0 = time.perf_counter()
        shape = tuple(run[0].shape)
        if len(shape) != 3 or shape[2] != 3 or run[0].dtype != torch.uint8:
            raise ValueError("expected (H,W,3) uint8 images, got %s %s" % (shape, run[0].dtype))
        shapes.add(shape)
        if device >= 0:
            if pinned is None or tuple(pinned.shape[1:]) != shape:
                pinned = torch.empty((batch,) + shape, dtype=torch.uint8).pin_memory()
            block = torch.stack(run, out=pinned[:len(run)])
            m = prep.channel_moments_u8(block.cuda(non_blocking=True)).cpu()       # the copy back waits for the launch: the block is free again
        else:
            m = prep.channel_moments_u8_host(torch.stack(run))
        moments.append(m)
        pixels.extend([shape[0] * shape[1]] * len(run))
        timer["moments"] += time.perf_counter() - t0
    if not moments:
        raise ValueError("the dataset has no images")
    return torch.cat(moments), pixels, shapes


def main(argv=None):
    from test._common import dataset_id_of, is_synthetic
    from train.global_p import mean_std_files
    from utils.general import cap_torch_threads
    ap = argparse.ArgumentParser(prog="python -m create_mean_std_file", description="Write the mean/std file of a dataset's training images.")
    ap.add_argument("--dataset", required=True, help="folder of the training images, or synthetic:<id>[:n=..][:labels=..][:size=..]")
    ap.add_argument("--out", help="file to write (default: train.global_p.mean_std_files[dataset id])")
    ap.add_argument("--device", type=int, default=0, help="GPU to use; negative: the same integers on the CPU")
    ap.add_argument("--batch", type=int, default=256, help="most images decoded and sent to the device at a time")
    ap.add_argument("--per-image", action="store_true", help="the per-image convention also when every image has one shape")
    args = ap.parse_args(argv)
    if args.batch < 1:
        ap.error("--batch must be positive")
    out = args.out or mean_std_files.get(dataset_id_of(args.dataset))
    if out is None:
        ap.error("--out is required: %r is not a dataset id of train.global_p.mean_std_files" % dataset_id_of(args.dataset))
    if not is_synthetic(args.dataset) and not os.path.isdir(args.dataset):
        ap.error("--dataset: %r is not a folder" % args.dataset)
    cap_torch_threads()
    timer = {"decode": 0.0, "moments": 0.0}
    t0 = time.perf_counter()
    images = _synthetic_images(args.dataset, args.batch) if is_synthetic(args.dataset) else _folder_images(args.dataset, args.batch, timer)
    if args.device >= 0:
        with torch.cuda.device(args.device):
            moments, pixels, shapes = collect_moments(images, args.batch, args.device, timer)
    else:
        moments, pixels, shapes = collect_moments(images, args.batch, args.device, timer)
    per_image = args.per_image or len(shapes) > 1
    mean, std = prep.mean_std(moments, pixels, per_image)
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    prep.write_mean_std(out, mean, std)
    print("Mean/std (%s) of %d images: mean %s std %s" % ("per image" if per_image else "pooled", len(pixels),
                                                          " ".join(map(repr, mean)), " ".join(map(repr, std))))
    print("Written to %s (%.2f s: decode %.2f s, moments on %s %.2f s)" % (out, time.perf_counter() - t0, timer["decode"],
                                                                          "cuda:%d" % args.device if args.device >= 0 else "the CPU", timer["moments"]))
    return mean, std


if __name__ == "__main__":
    main(sys.argv[1:])
