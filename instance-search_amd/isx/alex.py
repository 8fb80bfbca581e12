"""The convolutions and pools of an AlexNet-style `features` trunk: ctypes loader of libisxalex.so (the C ABI of include/isx_alex.h) and its two
torch wrappers.

libisxalex.so is a library of its own (csrc/alex.hip, built by the same Makefile), like libisxprep.so and libisxscale.so.  The loader follows
isx/_lib.py (a missing library is an error, never a fall-back) and the wrappers the argument contract of isx/ops.py: tensor metadata first (rank,
dtype, shapes, memory layout -- testable without a GPU), device residency last, then the output is allocated and the call enqueued on torch's
current stream.  There is no torch route behind them."""
import ctypes as C
import os

import torch

from ._lib import IsxError
from .ops import _cuda, _f32, _new_nhwc, _nhwc

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
LIB_PATH = os.path.join(_CSRC, "libisxalex.so")

_lib = None

_SIGNATURES = {
    "isxa_version": (C.c_int, []),
    "isxa_last_error": (C.c_char_p, []),
    "isxa_conv2d_nhwc": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                   C.c_void_p, C.c_void_p]),
    "isxa_maxpool3s2_nhwc": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
}
EXPORTS = tuple(sorted(_SIGNATURES))

MAX_K, MAX_STRIDE = 16, 4                       # ISXA_MAX_K and the stride limit of isxa_conv2d_nhwc


def lib():
    """The loaded library; raises (never falls back) when libisxalex.so is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IsxError("libisxalex.so not found at %s -- run `make -C %s` (or __graft_entry__.build()); there is no torch route behind isx.alex"
                           % (LIB_PATH, _CSRC))
        h = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            f = getattr(h, name)
            f.restype, f.argtypes = res, args
        _lib = h
    return _lib


def _launch(name, *args):
    rc = getattr(lib(), name)(*args, torch.cuda.current_stream().cuda_stream)
    if rc != 0:
        raise IsxError("%s failed (%d): %s" % (name, rc, lib().isxa_last_error().decode()))


def conv_out_size(size, K, stride, pad):
    """Output length of an axis of `size` inputs: floor((size + 2 pad - K) / stride) + 1; below 1 where the kernel does not fit."""
    return (size + 2 * pad - K) // stride + 1 if size + 2 * pad >= K else 0


def conv2d_applicable(conv):
    """Can `conv2d_nhwc` run this nn.Conv2d?  Square kernel up to MAX_K, equal strides up to MAX_STRIDE, equal padding below the kernel size and
    zeros, groups 1, dilation 1, Cout % 32 == 0."""
    k, s, p = tuple(conv.kernel_size), tuple(conv.stride), conv.padding
    return (isinstance(p, tuple) and k[0] == k[1] and 1 <= k[0] <= MAX_K and s[0] == s[1] and 1 <= s[0] <= MAX_STRIDE and p[0] == p[1]
            and 0 <= p[0] < k[0] and conv.padding_mode == "zeros" and conv.groups == 1 and tuple(conv.dilation) == (1, 1) and conv.out_channels % 32 == 0)


def conv2d_nhwc(x, w_ohwi, bias, stride=1, pad=0, relu=True):
    """Square K x K convolution (groups 1, dilation 1) of a channels-last (B,Cin,H,W) fp32 tensor with the epilogue fused: act(conv(x) + bias), the
    canonical two-level sum of the trunk kernels (isxa_conv2d_nhwc).  w_ohwi: (Cout,K,K,Cin) contiguous (= conv.weight.permute(0,2,3,1)),
    Cout % 32 == 0; 1 <= K <= 16, 1 <= stride <= 4, 0 <= pad < K.  Returns channels-last (B,Cout,Ho,Wo), Ho = (H + 2 pad - K) // stride + 1."""
    B, Cin, H, W = _nhwc(x, "x")
    w = _f32(w_ohwi, "w_ohwi", (None, None, None, Cin), "(Cout, K, K, Cin)")
    Cout, K = w.shape[0], w.shape[1]
    stride, pad = int(stride), int(pad)
    if w.shape[2] != K or not 1 <= K <= MAX_K or Cout % 32 != 0 or Cout < 32:
        raise IsxError("w_ohwi has shape %s, needs (Cout, K, K, Cin) with Cout %% 32 == 0 and 1 <= K <= %d" % (tuple(w.shape), MAX_K))
    if not 1 <= stride <= MAX_STRIDE or not 0 <= pad < K:
        raise IsxError("stride=%d pad=%d: needs 1 <= stride <= %d and 0 <= pad < K = %d" % (stride, pad, MAX_STRIDE, K))
    Ho, Wo = conv_out_size(H, K, stride, pad), conv_out_size(W, K, stride, pad)
    if Cin < 1 or Ho < 1 or Wo < 1:
        raise IsxError("x has shape %s: a %dx%d kernel with pad %d has no output on it" % (tuple(x.shape), K, K, pad))
    bias = _f32(bias, "bias", Cout)
    y = _new_nhwc((B, Cout, Ho, Wo), _cuda(x=x, w_ohwi=w, bias=bias))
    _launch("isxa_conv2d_nhwc", x.data_ptr(), B, H, W, Cin, w.data_ptr(), Cout, K, stride, pad, bias.data_ptr(), 1 if relu else 0, y.data_ptr())
    return y


def maxpool3s2(x):
    """MaxPool2d(3, stride 2) -- no padding, floor -- of a channels-last (B,C,H,W) fp32 tensor, C % 4 == 0, H, W >= 3 (isxa_maxpool3s2_nhwc): the bits
    of torch.nn.functional.max_pool2d, NaN, infinities and the sign of zero included.  Returns channels-last (B,C,(H-3)//2+1,(W-3)//2+1)."""
    B, Cc, H, W = _nhwc(x, "x")
    if Cc % 4 != 0 or Cc < 4 or H < 3 or W < 3:
        raise IsxError("x has shape %s, needs (B,C,H,W) with C %% 4 == 0 and H, W >= 3" % (tuple(x.shape),))
    y = _new_nhwc((B, Cc, (H - 3) // 2 + 1, (W - 3) // 2 + 1), _cuda(x=x))
    _launch("isxa_maxpool3s2_nhwc", x.data_ptr(), B, H, W, Cc, y.data_ptr())
    return y
