"""Cubic resize of 8-bit images (dataset preparation, and the second scale of train.classif_regions): ctypes loader of libisxscale.so (the C ABI
of include/isx_scale.h), its torch wrapper, the same bytes on the host, and the two size rules of the reference's pre_process_dataset.py.

libisxscale.so is a library of its own (csrc/scale.hip, built by the same Makefile), like libisxprep.so.  The loader follows isx/_lib.py (a
missing library is an error, never a fall-back) and the wrapper the argument contract of isx/ops.py (tensor metadata first, device residency
last, then the launch on torch's current stream).

The operation is defined in integers (include/isx_scale.h): half-pixel centres, the cubic with a = -3/4 in 11-bit coefficients, a 22-bit
rounding shift, replicated borders, no antialiasing -- OpenCV's INTER_CUBIC conventions for 8-bit images, but the pixels are defined here and
were never compared with an OpenCV binary.  Integer sums have no order, so the device and the host give the same bytes."""
import ctypes as C
import math
import os

import numpy as np
import torch

from ._lib import IsxError
from .ops import _on_current_device, _out

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
LIB_PATH = os.path.join(_CSRC, "libisxscale.so")

_lib = None

_SIGNATURES = {
    "isxs_version": (C.c_int, []),
    "isxs_last_error": (C.c_char_p, []),
    "isxs_resize_cubic_u8": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_void_p,
                                       C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
}
EXPORTS = tuple(sorted(_SIGNATURES))

MAX_OUT, MAX_IN = 16384, 32768                    # the limits of isxs_resize_cubic_u8, held on the host route too


def lib():
    """The loaded library; raises (never falls back) when libisxscale.so is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IsxError("libisxscale.so not found at %s -- run `make -C %s` (or __graft_entry__.build()); "
                           "resize_cubic_u8_host is the CPU path and is never chosen silently" % (LIB_PATH, _CSRC))
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            f = getattr(h, name)
            f.restype, f.argtypes = res, args
        _lib = h
    return _lib


# ---- the reference's size rules --------------------------------------------------------------------------------------------------------------------
def short_side_size(H, W, new):
    """(Hd, Wd) of an (H, W) image whose shorter side goes to `new` (reference utils/image.py scale_cv, pre_process_dataset.py:48-54): the
    longer side is Python's round() of new * long / short; unchanged when the shorter side already equals `new`."""
    H, W, new = int(H), int(W), int(new)
    if H < 1 or W < 1 or new < 1:
        raise IsxError("short_side_size: H, W and the new size must be positive, got %d x %d -> %d" % (H, W, new))
    if (W <= H and W == new) or (H <= W and H == new):
        return H, W
    if W < H:
        return int(round(float(new * H) / W)), new
    return new, int(round(float(new * W) / H))


def aspect_pad(H, W, max_ar):
    """(top, left, Hp, Wp): the padded canvas that brings an (H, W) image to an aspect ratio of at most `max_ar` (reference
    pre_process_dataset.py:29-46): the short side becomes ceil(long / max_ar), the odd pixel goes to the top / left; (0, 0, H, W) when the image
    is within the ratio or max_ar < 1."""
    H, W, max_ar = int(H), int(W), float(max_ar)
    if H < 1 or W < 1:
        raise IsxError("aspect_pad: H and W must be positive, got %d x %d" % (H, W))
    if max_ar >= 1.0 and H > W and float(H) / W > max_ar:
        Wp = int(math.ceil(float(H) / max_ar))
        return 0, (Wp - W) // 2 + (Wp - W) % 2, H, Wp
    if max_ar >= 1.0 and H < W and float(W) / H > max_ar:
        Hp = int(math.ceil(float(W) / max_ar))
        return (Hp - H) // 2 + (Hp - H) % 2, 0, Hp, W
    return 0, 0, H, W


# ---- arguments -------------------------------------------------------------------------------------------------------------------------------------
def _geometry(img_u8, size, pad):
    B, Hs, Ws, _ = _out(img_u8, (None, None, None, 3), torch.uint8, "img_u8").shape
    try:
        Hd, Wd = (int(v) for v in size)
        top, left, Hp, Wp = (0, 0, Hs, Ws) if pad is None else (int(v) for v in pad)
    except (TypeError, ValueError):
        raise IsxError("size must be (Hd, Wd) and pad (top, left, Hp, Wp), got size=%r pad=%r" % (size, pad))
    if min(Hs, Ws, Hd, Wd, Hp, Wp) < 1 or B > 65535 or top < 0 or left < 0 or top + Hs > Hp or left + Ws > Wp:
        raise IsxError("bad shape: img_u8 %s at (%d,%d) of %dx%d -> %dx%d (sides >= 1, B <= 65535, top + Hs <= Hp, left + Ws <= Wp)"
                       % (tuple(img_u8.shape), top, left, Hp, Wp, Hd, Wd))
    if max(Hd, Wd) > MAX_OUT or max(Hp, Wp) > MAX_IN or 3 * Hp * Wp >= 1 << 31 or 3 * Hd * Wd >= 1 << 31:
        raise IsxError("image too large: %dx%d -> %dx%d, needs Hd, Wd <= %d, Hp, Wp <= %d, 3 Hp Wp < 2^31 and 3 Hd Wd < 2^31"
                       % (Hp, Wp, Hd, Wd, MAX_OUT, MAX_IN))
    return B, Hs, Ws, top, left, Hp, Wp, Hd, Wd, (top, left, Hp, Wp) != (0, 0, Hs, Ws)


def resize_cubic_u8(img_u8, size, pad=None, seed=0, noise_ids=None, out=None):
    """(B,Hs,Ws,3) uint8 RGB on the GPU -> (B,Hd,Wd,3) uint8, size = (Hd, Wd) (isxs_resize_cubic_u8).  pad = (top, left, Hp, Wp): the image
    sits at (top, left) of an (Hp, Wp) canvas of noise bytes noise_bytes(seed, noise_ids[b], Hp, Wp) and the canvas is what is resized;
    noise_ids: (B,) int64 on the GPU, required when the pad adds anything.  `out`: the caller's (B,Hd,Wd,3) uint8 buffer, overwritten in place."""
    B, Hs, Ws, top, left, Hp, Wp, Hd, Wd, padded = _geometry(img_u8, size, pad)
    y = out if out is None else _out(out, (B, Hd, Wd, 3), torch.uint8, "out")
    if noise_ids is not None:
        _out(noise_ids, (B,), torch.int64, "noise_ids")
    elif padded:
        raise IsxError("noise_ids must be given, (B,) int64, when pad adds pixels")
    for name, t in (("img_u8", img_u8), ("noise_ids", noise_ids), ("out", y)):
        if t is not None:
            if not t.is_cuda:
                raise IsxError("%s must be a CUDA tensor (resize_cubic_u8_host takes CPU tensors)" % name)
            _on_current_device(t, name)
    if y is None:
        y = torch.empty((B, Hd, Wd, 3), device=img_u8.device, dtype=torch.uint8)
    rc = lib().isxs_resize_cubic_u8(img_u8.data_ptr(), B, Hs, Ws, top, left, Hp, Wp, int(seed) & (2 ** 64 - 1),
                                    None if noise_ids is None else noise_ids.data_ptr(), y.data_ptr(), Hd, Wd, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise IsxError("isxs_resize_cubic_u8 failed (%d): %s" % (rc, lib().isxs_last_error().decode()))
    return y


# ---- the same bytes on the host --------------------------------------------------------------------------------------------------------------------
def axis_table(S, T):
    """(taps (T,4) int64, coefficients (T,4) int64) of an axis of source length S and output length T (include/isx_scale.h), in int64 numpy:
    // on integers is floor division."""
    j = np.arange(T, dtype=np.int64)
    D = np.int64(2 * T)
    num = (2 * j + 1) * np.int64(S) - np.int64(T)
    s = num // D
    r = num - s * D
    q = D - r
    D3 = D * D * D

    def nearest(n):
        return (2 * n + D3) // (2 * D3)
    c0 = nearest(-1536 * r * q * q)
    c1 = nearest(2560 * r * r * r - 4608 * r * r * D + 2048 * D3)
    c2 = nearest(2560 * q * q * q - 4608 * q * q * D + 2048 * D3)
    coef = np.stack([c0, c1, c2, 2048 - c0 - c1 - c2], 1)
    taps = np.clip(s[:, None] - 1 + np.arange(4, dtype=np.int64)[None, :], 0, S - 1)
    return taps, coef


def padded_image(img, top, left, Hp, Wp, seed, noise_id):
    """The (Hp,Wp,3) canvas the resize reads: `img` (Hs,Ws,3) at (top, left), utils.image.noise_bytes(seed, noise_id, Hp, Wp) around it."""
    if (top, left, Hp, Wp) == (0, 0, img.shape[0], img.shape[1]):
        return img
    from utils.image import noise_bytes
    canvas = noise_bytes(seed, noise_id, Hp, Wp)
    canvas[top:top + img.shape[0], left:left + img.shape[1]] = img
    return canvas


def resize_cubic_u8_host(img_u8, size, pad=None, seed=0, noise_ids=None):
    """The bytes of resize_cubic_u8 from CPU tensors (what --device=-1 runs): int64 numpy, one image at a time, columns then rows."""
    B, Hs, Ws, top, left, Hp, Wp, Hd, Wd, padded = _geometry(img_u8, size, pad)
    if img_u8.is_cuda or (isinstance(noise_ids, torch.Tensor) and noise_ids.is_cuda):
        raise IsxError("img_u8 and noise_ids must be CPU tensors (resize_cubic_u8 takes CUDA tensors)")
    ids = [0] * B if noise_ids is None else [int(v) for v in (noise_ids.tolist() if hasattr(noise_ids, "tolist") else noise_ids)]
    if padded and (noise_ids is None or len(ids) != B):
        raise IsxError("noise_ids must be given, (B,) int64, when pad adds pixels")
    tx, cx = axis_table(Wp, Wd)
    ty, cy = axis_table(Hp, Hd)
    rows = np.unique(ty)                                       # the source rows any output row reads
    at = np.searchsorted(rows, ty)
    src = img_u8.numpy()
    dst = np.empty((B, Hd, Wd, 3), np.uint8)
    for b in range(B):
        P = padded_image(src[b], top, left, Hp, Wp, seed, ids[b])[rows].astype(np.int64)
        h = sum(cx[None, :, k, None] * P[:, tx[:, k]] for k in range(4))                    # (rows, Wd, 3)
        v = sum(cy[:, i, None, None] * h[at[:, i]] for i in range(4))                       # (Hd, Wd, 3)
        dst[b] = np.clip((v + (1 << 21)) >> 22, 0, 255)
    return torch.from_numpy(dst)
