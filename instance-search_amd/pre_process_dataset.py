"""Dataset preparation: resize every image of a dataset into a new folder -- the script that makes the data/pre_proc/<id>_448 folders the
train/*_p.py files point at (reference pre_process_dataset.py).

    python -m pre_process_dataset --dataset=<folder> --out=<folder> [--short-side=448 | --size=WxH] [--max-ar=2.0] [--device=0] [--batch=64] [--seed=0]

The images of <folder> itself go to --out and those of its `test` sub-folder to <out>/test (the two calls at the bottom of the reference
script); file names are kept and the file type follows the extension (JPEG at quality 95, cv2.imwrite's default, PNG as is).  An image whose
aspect ratio exceeds --max-ar is first padded with random bytes to that ratio (isx.scale.aspect_pad), then its shorter side is brought to
--short-side (isx.scale.short_side_size), or the image to --size; an image that needs neither is written from its decoded pixels unchanged.

The images stream through the decoder processes of train/_decode_farm.py, at most --batch decoded at a time; consecutive images of one shape
go through one isx.scale.resize_cubic_u8 launch (a ragged folder: one launch per run of equal shapes).  The padding bytes are the counter-based
generator of utils.image.noise_bytes with the image's position in the folder's sorted file list as its noise id -- not the reference's
np.random stream -- and the resize is the integer operation of include/isx_scale.h (OpenCV's INTER_CUBIC conventions; the pixels are defined
here and were never compared with an OpenCV binary): the result depends neither on --batch nor on --device, --device=-1 computes the same
pixels on the host and writes the same files."""
from __future__ import print_function

import argparse
import os
import sys
import time

import numpy as np
import torch

from isx import scale


def sorted_files(folder):
    from utils import get_images_labels
    return sorted(f for f, _ in get_images_labels(folder))


def plan(H, W, max_ar, short_side=None, size=None):
    """((top, left, Hp, Wp), (Hd, Wd)) of an (H, W) image: the pad to --max-ar, then --size = (Hd, Wd) or the shorter side to --short-side."""
    pad = scale.aspect_pad(H, W, max_ar)
    return pad, (tuple(size) if size is not None else scale.short_side_size(pad[2], pad[3], short_side))


def _decoded(files, batch, timer):
    """The decoded (H,W,3) uint8 images of `files` in lists of at most `batch`: one list is alive at a time."""
    from test._common import imread_rgb, to_raw_tensor
    from train import _decode_farm as DF
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
        yield a, images
        del images


def _runs(images):
    """(offset, run) of the runs of consecutive images of one shape."""
    start = 0
    for i in range(1, len(images) + 1):
        if i == len(images) or images[i].shape != images[start].shape:
            yield start, images[start:i]
            start = i


def resize_run(run, ids, max_ar, short_side, size, device, seed):
    """A list of (H,W,3) uint8 CPU tensors of ONE shape -> their outputs, (n,Hd,Wd,3) uint8 on the CPU; `ids`: their noise ids."""
    shape = tuple(run[0].shape)
    if len(shape) != 3 or shape[2] != 3 or run[0].dtype != torch.uint8:
        raise ValueError("expected (H,W,3) uint8 images, got %s %s" % (shape, run[0].dtype))
    pad, hw = plan(shape[0], shape[1], max_ar, short_side, size)
    block = torch.stack(run)
    if pad == (0, 0, shape[0], shape[1]) and hw == shape[:2]:
        return block                                          # neither pad nor resize: the decoded pixels
    if device >= 0:
        noise = torch.tensor(ids, dtype=torch.int64).cuda()
        return scale.resize_cubic_u8(block.pin_memory().cuda(non_blocking=True), hw, pad=pad, seed=seed, noise_ids=noise).cpu()
    return scale.resize_cubic_u8_host(block, hw, pad=pad, seed=seed, noise_ids=ids)


def write_image(path, pixels):
    """(H,W,3) uint8 -> the file; the type follows the extension."""
    from PIL import Image
    im = Image.fromarray(np.ascontiguousarray(pixels))
    if path.lower().endswith(".png"):
        im.save(path, format="PNG")
    else:
        im.save(path, format="JPEG", quality=95)


def process_folder(folder, out_dir, args, timer):
    """Every image of `folder` (not of its sub-folders) resized into `out_dir`.  Returns [(output file, (Hd, Wd))] in sorted-file order."""
    files = sorted_files(folder)
    written = []
    if files:
        os.makedirs(out_dir, exist_ok=True)
    for a, images in _decoded(files, args.batch, timer):
        for off, run in _runs(images):
            t0 = time.perf_counter()
            ids = list(range(a + off, a + off + len(run)))     # the position in the sorted file list: independent of --batch
            out = resize_run(run, ids, args.max_ar, args.short_side, args.size, args.device, args.seed).numpy()
            timer["resize"] += time.perf_counter() - t0
            t0 = time.perf_counter()
            for k in range(len(run)):
                path = os.path.join(out_dir, os.path.basename(files[a + off + k]))
                write_image(path, out[k])
                written.append((path, tuple(out[k].shape[:2])))
            timer["encode"] += time.perf_counter() - t0
    return written


def _parse_size(arg):
    try:
        w, h = (int(v) for v in arg.lower().split("x"))
    except ValueError:
        raise argparse.ArgumentTypeError("--size takes WxH, got %r" % (arg,))
    if w < 1 or h < 1:
        raise argparse.ArgumentTypeError("--size takes positive sides, got %r" % (arg,))
    return h, w


def main(argv=None):
    from utils.general import cap_torch_threads
    ap = argparse.ArgumentParser(prog="python -m pre_process_dataset", description="Resize all images of a dataset into a new folder.")
    ap.add_argument("--dataset", required=True, help="folder of the training images; its `test` sub-folder holds the test images")
    ap.add_argument("--out", required=True, help="folder to write to (the test images go to its `test` sub-folder)")
    ap.add_argument("--short-side", type=int, default=None, help="shorter side of every output (default 448)")
    ap.add_argument("--size", type=_parse_size, default=None, help="WxH: every output has this size")
    ap.add_argument("--max-ar", type=float, default=2.0, help="largest aspect ratio; images beyond it are padded with random bytes (< 1: never)")
    ap.add_argument("--device", type=int, default=0, help="GPU to use; negative: the same pixels on the CPU")
    ap.add_argument("--batch", type=int, default=64, help="most images decoded and sent to the device at a time")
    ap.add_argument("--seed", type=int, default=0, help="seed of the padding bytes")
    args = ap.parse_args(argv)
    if args.batch < 1:
        ap.error("--batch must be positive")
    if args.short_side is not None and args.size is not None:
        ap.error("--short-side and --size exclude each other")
    if args.short_side is None and args.size is None:
        args.short_side = 448
    if args.short_side is not None and args.short_side < 1:
        ap.error("--short-side must be positive")
    if not os.path.isdir(args.dataset):
        ap.error("--dataset: %r is not a folder" % args.dataset)
    cap_torch_threads()
    timer = {"decode": 0.0, "resize": 0.0, "encode": 0.0}
    t0 = time.perf_counter()

    def both():
        out = process_folder(args.dataset, args.out, args, timer)
        test = os.path.join(args.dataset, "test")
        return out, (process_folder(test, os.path.join(args.out, "test"), args, timer) if os.path.isdir(test) else [])
    if args.device >= 0:
        with torch.cuda.device(args.device):
            train, test = both()
    else:
        train, test = both()
    print("%d + %d images written to %s (%.2f s: decode %.2f s, resize on %s %.2f s, encode %.2f s)"
          % (len(train), len(test), args.out, time.perf_counter() - t0, timer["decode"], "cuda:%d" % args.device if args.device >= 0 else "the CPU",
             timer["resize"], timer["encode"]))
    return train, test


if __name__ == "__main__":
    main(sys.argv[1:])
