"""Dataset statistics (pipeline stage 0): ctypes loader of libisxprep.so (the C ABI of include/isx_prep.h), its torch wrapper, the same
integers on the host, and the exact mean/std arithmetic behind create_mean_std_file.py.

libisxprep.so is a library of its own (csrc/prep.hip, built by the same Makefile): dataset preparation is an offline tool, not part of the
drop-in boundary of libisx.so / include/isx.h / isx/ops.py.  The loader follows isx/_lib.py (a missing library is an error, never a fall-back)
and the wrapper the argument contract of isx/ops.py (tensor metadata first, device residency last, then the launch on torch's current stream).

The moments are integers -- sum and sum of squares of the uint8 values of every channel of every image -- so they have no summation order:
the device and the host give the same bits for any batch size, and mean_std() turns them into the two floats per channel in exact rational
arithmetic with ONE rounding (two for std: the variance, then its square root)."""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import torch

from ._lib import IsxError
from .ops import _on_current_device, _out

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
LIB_PATH = os.path.join(_CSRC, "libisxprep.so")

_lib = None

_SIGNATURES = {
    "isxp_version": (C.c_int, []),
    "isxp_last_error": (C.c_char_p, []),
    "isxp_channel_moments_u8": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
}
EXPORTS = tuple(sorted(_SIGNATURES))


def lib():
    """The loaded library; raises (never falls back) when libisxprep.so is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IsxError("libisxprep.so not found at %s -- run `make -C %s` (or __graft_entry__.build()); "
                           "channel_moments_u8_host is the CPU path and is never chosen silently" % (LIB_PATH, _CSRC))
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            f = getattr(h, name)
            f.restype, f.argtypes = res, args
        _lib = h
    return _lib


def _image_batch(img_u8):
    return _out(img_u8, (None, None, None, 3), torch.uint8, "img_u8").shape


def channel_moments_u8(img_u8, out=None):
    """(B,H,W,3) uint8 RGB on the GPU -> (B,3,2) int64: [b][c][0] the sum of channel c of image b, [b][c][1] its sum of squares
    (isxp_channel_moments_u8).  `out`: the caller's (B,3,2) int64 buffer, overwritten in place."""
    B, H, W, _ = _image_batch(img_u8)
    m = out if out is None else _out(out, (B, 3, 2), torch.int64, "out")
    for name, t in (("img_u8", img_u8), ("out", m)):
        if t is not None:
            if not t.is_cuda:
                raise IsxError("%s must be a CUDA tensor (channel_moments_u8_host takes CPU tensors)" % name)
            _on_current_device(t, name)
    if m is None:
        m = torch.empty((B, 3, 2), device=img_u8.device, dtype=torch.int64)
    rc = lib().isxp_channel_moments_u8(img_u8.data_ptr(), B, H, W, m.data_ptr(), torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise IsxError("isxp_channel_moments_u8 failed (%d): %s" % (rc, lib().isxp_last_error().decode()))
    return m


def channel_moments_u8_host(img_u8):
    """The integers of channel_moments_u8 from a CPU tensor (what --device=-1 runs): int64 sums in numpy, one image at a time."""
    B, H, W, _ = _image_batch(img_u8)
    if img_u8.is_cuda:
        raise IsxError("img_u8 must be a CPU tensor (channel_moments_u8 takes CUDA tensors)")
    a = img_u8.numpy().reshape(B, H * W, 3)
    m = np.empty((B, 3, 2), np.int64)
    for b in range(B):
        m[b, :, 0] = a[b].sum(axis=0, dtype=np.int64)
        m[b, :, 1] = np.square(a[b], dtype=np.uint16).sum(axis=0, dtype=np.int64)          # 255^2 = 65025 fits 16 bits
    return torch.from_numpy(m)


def _ints(v):
    return v.tolist() if hasattr(v, "tolist") else list(v)


def mean_std(moments, pixels, per_image=False):
    """(mean, std): two lists of three floats for ToTensor + Normalize, from the (N,3,2) integer moments of N images and their (N,) pixel
    counts H W.  The two conventions are the two branches of the reference's create_mean_std_file.py:25-46 on v / 255:

    pooled (image_size given)        over all values of a channel: the mean and the UNBIASED standard deviation (divisor n - 1: Tensor.std())
    per image (image_size = None)    mean = the average over images of each image's mean; std^2 = the average over images of each image's mean
                                     squared deviation from THAT mean, (S2/255^2 - 2 mean S1/255 + n mean^2) / n: images weigh alike

    Every value is a fractions.Fraction of the integers, rounded once to float64; std = math.sqrt(float(variance))."""
    m, n = _ints(moments), [int(p) for p in _ints(pixels)]
    N = len(n)
    if N < 1 or len(m) != N or any(len(im) != 3 or any(len(ch) != 2 for ch in im) for im in m):
        raise IsxError("moments has %d images, needs (N,3,2) with N = len(pixels) = %d >= 1" % (len(m), N))
    if min(n) < 1:
        raise IsxError("pixels must be positive, got %d" % min(n))
    mean, std = [], []
    for c in range(3):
        if per_image:
            by_n = {}                                     # images of one pixel count share a denominator: the Fractions stay small
            for i in range(N):
                t = by_n.setdefault(n[i], [0, 0])
                t[0] += int(m[i][c][0])
                t[1] += int(m[i][c][1])
            mu = sum(Fraction(s1, 255 * k) for k, (s1, _) in by_n.items()) / N
            var = sum((Fraction(s2, 65025) - 2 * mu * Fraction(s1, 255)) / k for k, (s1, s2) in by_n.items()) / N + mu * mu
        else:
            T, S1, S2 = sum(n), sum(int(im[c][0]) for im in m), sum(int(im[c][1]) for im in m)
            mu = Fraction(S1, 255 * T)
            var = Fraction(S2 * T - S1 * S1, 65025 * T * (T - 1)) if T > 1 else None
        mean.append(float(mu))
        std.append(float("nan") if var is None else math.sqrt(float(var)))      # one value has no unbiased deviation: nan, as Tensor.std()
    return mean, std


def write_mean_std(path, mean, std):
    """The file utils.general.read_mean_std reads (reference create_mean_std_file.py:48-52): the reprs of the means on one line, of the stds
    on the next."""
    with open(path, "w") as f:
        f.write(" ".join(map(repr, mean)))
        f.write("\n")
        f.write(" ".join(map(repr, std)))
        f.write("\n")
