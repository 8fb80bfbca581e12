"""CPU model of libisxalex (include/isx_alex.h): the general K x K convolution with the trunk's canonical two-level sum and the un-padded 3 / 2
max-pool, shared by tests/test_alex_model.py (the model against oracle.conv3x3_nhwc, float64, torch's CPU pool, and the wrong orders it has to
tell apart) and tests/test_gpu_alex.py (the kernels against the model, bit for bit).  It imports nothing from the libraries.

The convolution is a zero-padded im2col in (kh, kw, ci) order; every chunk of 64 terms is one oracle.cosine_sim call -- a k-ordered fp32 fmaf chain
from +0, the chain the fp32 MFMA computes -- as tests/_head_model.chains does it; the chunk sums are added in order in numpy float32 (one rounding
each, never fused), then the epilogue.  A padding tap is a term like any other: fma(0, w, acc)."""
import functools

import numpy as np

from _head_model import chains, inputs

F = np.float32
CHUNK = 64                                        # ISXA_CONV_CHUNK = ISX_CONV_CHUNK


def out_size(size, K, stride, pad):
    return (size + 2 * pad - K) // stride + 1


def im2col(x, K, stride, pad):
    """(B,H,W,Cin) -> (B Ho Wo, K K Cin): row m = the window of output pixel m flattened in (kh, kw, ci) order, zeros where it hangs over the edge."""
    x = np.asarray(x, F)
    B, H, W, Cin = x.shape
    Ho, Wo = out_size(H, K, stride, pad), out_size(W, K, stride, pad)
    assert Ho >= 1 and Wo >= 1
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    taps = [xp[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride, :] for kh in range(K) for kw in range(K)]
    return np.ascontiguousarray(np.stack(taps, 3).reshape(B * Ho * Wo, K * K * Cin)), (B, Ho, Wo)


def tap_inside(H, W, K, stride, pad):
    """(Ho Wo, K K) bool: tap (kh, kw) of output pixel (ho, wo) lies inside the image."""
    Ho, Wo = out_size(H, K, stride, pad), out_size(W, K, stride, pad)
    hi = (np.arange(Ho) * stride - pad)[:, None] + np.arange(K)[None, :]
    wi = (np.arange(Wo) * stride - pad)[:, None] + np.arange(K)[None, :]
    okh, okw = (hi >= 0) & (hi < H), (wi >= 0) & (wi < W)
    return (okh[:, None, :, None] & okw[None, :, None, :]).reshape(Ho * Wo, K * K)


def two_level(A, Wm, chunk=CHUNK):
    """tot = 0; for every chunk of `chunk` columns in order: tot = tot + chain(chunk)."""
    tot = np.zeros((A.shape[0], Wm.shape[0]), F)
    for lo in range(0, A.shape[1], chunk):
        tot = tot + chains(A[:, lo:lo + chunk], Wm[:, lo:lo + chunk])
    return tot


def epilogue(tot, bias, relu):
    """y = tot + bias (one rounded add); relu: max(y, 0) with a NaN going to 0, as fmaxf(y, 0) does."""
    y = tot + np.asarray(bias, F)[None, :]
    return np.where(y > 0, y, F(0)) if relu else y


def conv2d(x, w_ohwi, bias, stride, pad, relu, chunk=CHUNK):
    """isxa_conv2d_nhwc: (B,H,W,Cin), (Cout,K,K,Cin), (Cout) -> (B,Ho,Wo,Cout)."""
    w = np.asarray(w_ohwi, F)
    Cout, K = w.shape[0], w.shape[1]
    A, (B, Ho, Wo) = im2col(x, K, stride, pad)
    return epilogue(two_level(A, w.reshape(Cout, -1), chunk), bias, relu).reshape(B, Ho, Wo, Cout)


def conv2d_one_chain(x, w_ohwi, bias, stride, pad, relu):
    """A WRONG order the model is told apart from: one chain over the whole reduction."""
    return conv2d(x, w_ohwi, bias, stride, pad, relu, chunk=1 << 30)


def conv2d_chunks_skip_padding(x, w_ohwi, bias, stride, pad, relu):
    """A WRONG order the model is told apart from: the padding taps are left out BEFORE the reduction is cut into chunks, so that behind a padding
    tap every chunk boundary sits Cin terms further on in the window."""
    w = np.asarray(w_ohwi, F)
    Cout, K, Cin = w.shape[0], w.shape[1], w.shape[3]
    A, (B, Ho, Wo) = im2col(x, K, stride, pad)
    Wm = w.reshape(Cout, -1)
    inside = tap_inside(x.shape[1], x.shape[2], K, stride, pad)
    tot = np.zeros((B, Ho * Wo, Cout), F)
    A = A.reshape(B, Ho * Wo, -1)
    for pattern in np.unique(inside, axis=0):
        pix = np.flatnonzero((inside == pattern[None, :]).all(1))
        cols = np.flatnonzero(np.repeat(pattern, Cin))
        rows = np.ascontiguousarray(A[:, pix][:, :, cols].reshape(B * len(pix), len(cols)))
        tot[:, pix] = two_level(rows, np.ascontiguousarray(Wm[:, cols])).reshape(B, len(pix), Cout)
    return epilogue(tot.reshape(B * Ho * Wo, Cout), bias, relu).reshape(B, Ho, Wo, Cout)


def conv2d_f64(x, w_ohwi, bias, stride, pad, relu):
    """The same convolution in float64: what the fp32 bounds are measured against.  Also returns sum |x w| + |bias| per output."""
    w = np.asarray(w_ohwi, np.float64)
    Cout, K = w.shape[0], w.shape[1]
    A, (B, Ho, Wo) = im2col(x, K, stride, pad)
    A = A.astype(np.float64)
    Wm = w.reshape(Cout, -1)
    y = A @ Wm.T + np.asarray(bias, np.float64)[None, :]
    mag = np.abs(A) @ np.abs(Wm).T + np.abs(np.asarray(bias, np.float64))[None, :]
    if relu:
        y = np.maximum(y, 0)
    return y.reshape(B, Ho, Wo, Cout), mag.reshape(B, Ho, Wo, Cout)


def maxpool3s2(x):
    """isxa_maxpool3s2_nhwc: (B,H,W,C) -> (B,(H-3)//2+1,(W-3)//2+1,C); the window in (kh, kw) order from its first element,
    `if (v > m || v != v) m = v`."""
    x = np.asarray(x, F)
    B, H, W, C = x.shape
    Ho, Wo = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    m = None
    with np.errstate(invalid="ignore"):
        for kh in range(3):
            for kw in range(3):
                v = x[:, kh:kh + 2 * (Ho - 1) + 1:2, kw:kw + 2 * (Wo - 1) + 1:2, :]
                m = v.copy() if m is None else np.where((v > m) | (v != v), v, m)
    return np.ascontiguousarray(m)


def trunk(layers, x):
    """A `features` trunk layer by layer on a channels-last (B,H,W,3) batch.  layers: ("conv", w_ohwi, bias, stride, pad, relu) | ("pool",)."""
    for layer in layers:
        x = conv2d(x, *layer[1:]) if layer[0] == "conv" else maxpool3s2(x)
    return x


# ---- shared, read-only cases ----------------------------------------------------------------------------------------------------------------
# name -> (B, H, W, Cin, Cout, K, stride, pad): the table of the issue, and the two shapes at which the launch takes its larger tiles
CONV_CASES = {
    "11x11s4_3to64": (2, 35, 47, 3, 64, 11, 4, 2),            # K K Cin = 363: odd, last chunk 43 terms; M = 176 pixels, no tile multiple
    "5x5_64to192": (3, 7, 9, 64, 192, 5, 1, 2),               # K K Cin = 1600: exactly 25 chunks
    "3x3s1_32to64": (2, 5, 6, 32, 64, 3, 1, 1),
    "3x3s2_32to64": (2, 5, 6, 32, 64, 3, 2, 1),
    "3x3s1_192to384": (1, 13, 13, 192, 384, 3, 1, 1),
    "3x3s2_192to384": (1, 13, 13, 192, 384, 3, 2, 1),
    "6x6_32to32": (1, 7, 8, 32, 32, 6, 1, 0),                 # even kernel, one 32-column half of a tile
    "1x1_4to64": (2, 5, 7, 4, 64, 1, 1, 0),                   # smallest reduction: one k-tile, four live terms
    "3x3s3_5to32": (1, 9, 10, 5, 32, 3, 3, 2),                # Cin % 4 != 0 with Cin > 4, stride 3, padding 2
    "tile128x64": (1, 362, 362, 4, 64, 1, 1, 0),              # 1024 tiles of 128 x 64 (M = 131044: the last one partial)
    "tile128x128": (1, 256, 257, 4, 128, 1, 1, 0),            # 514 tiles of 128 x 128
}
POOL_CASES = ((2, 7, 9, 64), (1, 55, 55, 64), (3, 13, 13, 256))


# ---- the refusals of include/isx_alex.h, one table for the CPU test (pointers that are never dereferenced) and the GPU test (live buffers) ----
# A valid call; the pointers are byte addresses on a 16-byte boundary.  An override names arguments; "x+" / "w+" / "y+": that pointer moved by bytes.
CONV_GOOD = dict(x=1 << 20, B=1, H=5, W=6, Cin=4, w=2 << 20, Cout=32, K=3, stride=1, pad=1, bias=3 << 20, relu=1, y=4 << 20)
CONV_REFUSALS = [
    ("bad shape", dict(B=-1)), ("bad shape", dict(H=0)), ("bad shape", dict(W=0)), ("bad shape", dict(Cin=0)), ("bad shape", dict(Cout=0)),
    ("bad shape", dict(Cout=48)), ("bad shape", dict(Cout=16)), ("bad shape", dict(K=0)), ("bad shape", dict(K=17, pad=0, H=40, W=40)),
    ("bad shape", dict(stride=0)), ("bad shape", dict(stride=5)), ("bad shape", dict(pad=-1)), ("bad shape", dict(pad=3)),
    ("bad shape", dict(H=(1 << 20) + 1)), ("bad shape", dict(W=(1 << 20) + 1)), ("bad shape", dict(Cin=(1 << 20) + 4)), ("bad shape", dict(Cout=(1 << 20) + 32)),
    ("bad shape", dict(K=5, pad=0, H=4)), ("bad shape", dict(K=5, pad=0, W=4)),                   # Ho or Wo < 1
    ("bad shape", dict(K=11, pad=0, H=11, W=11, Cin=1 << 16)),                                     # K K Cin above 2^22
    ("bad shape", dict(K=16, pad=0, H=16, W=1 << 20, Cin=1 << 8)),                                 # K (W + 1) Cin not below 2^31
    ("bad shape", dict(K=1, pad=0, B=1 << 21, H=1 << 10, W=1 << 10)),                              # B Ho Wo above 2^40
    ("bad shape", dict(K=1, pad=0, B=1 << 12, H=1 << 10, W=1 << 10)),                              # 2^26 rows of tiles
    ("null pointer", dict(x=None)), ("null pointer", dict(w=None)), ("null pointer", dict(bias=None)), ("null pointer", dict(y=None)),
    ("alias", dict(alias=True)),
    ("16-B aligned", {"x+": 4}), ("16-B aligned", {"w+": 8}), ("16-B aligned", {"y+": 4}),
]
POOL_GOOD = dict(x=1 << 20, B=1, H=5, W=6, C=8, y=4 << 20)
POOL_REFUSALS = [
    ("bad shape", dict(B=-1)), ("bad shape", dict(H=2)), ("bad shape", dict(W=2)), ("bad shape", dict(C=0)), ("bad shape", dict(C=6)),
    ("bad shape", dict(B=1 << 40, H=1 << 12, W=1 << 12)),
    ("null pointer", dict(x=None)), ("null pointer", dict(y=None)), ("alias", dict(alias=True)),
    ("16-B aligned", {"x+": 4}), ("16-B aligned", {"y+": 8}),
]


def call_abi(L, entry, a, stream):
    """One call of `entry` of the loaded library L from an argument table like CONV_GOOD / POOL_GOOD (with the overrides of a refusal applied)."""
    a = dict(a)
    for k in ("x", "w", "y"):
        if k + "+" in a:
            a[k] += a.pop(k + "+")
    if a.pop("alias", False):
        a["y"] = a["x"]
    if entry == "isxa_conv2d_nhwc":
        return L.isxa_conv2d_nhwc(a["x"], a["B"], a["H"], a["W"], a["Cin"], a["w"], a["Cout"], a["K"], a["stride"], a["pad"], a["bias"], a["relu"], a["y"], stream)
    return L.isxa_maxpool3s2_nhwc(a["x"], a["B"], a["H"], a["W"], a["C"], a["y"], stream)


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def conv_inputs(name):
    """(x, w_ohwi, bias): the reduction's columns scaled over 1e-2 .. 1e2 (tests/_head_model.inputs), so that partial sums of different lengths
    round differently; ReLU-like x (half the entries 0) for the layers behind one."""
    B, H, W, Cin, Cout, K, stride, pad = CONV_CASES[name]
    seed = sum(map(ord, name))
    x = inputs(B * H * W, Cin, seed, special_rows=False).reshape(B, H, W, Cin)
    w = (inputs(Cout, K * K * Cin, seed + 1, special_rows=False) * F((K * K * Cin) ** -0.5)).reshape(Cout, K, K, Cin)
    bias = np.random.default_rng(seed + 2).standard_normal(Cout).astype(F)
    return _frozen(np.ascontiguousarray(x), np.ascontiguousarray(w), bias)


@functools.lru_cache(maxsize=None)
def conv_case(name, relu=True):
    """(x, w_ohwi, bias, y) of CONV_CASES[name], computed once."""
    x, w, bias = conv_inputs(name)
    stride, pad = CONV_CASES[name][6:]
    return _frozen(x, w, bias, conv2d(x, w, bias, stride, pad, relu))


@functools.lru_cache(maxsize=None)
def pool_case(shape):
    """(x, y): standard normals with NaN (two payloads and signs), +-inf and +-0 planted -- alone in a window, together, first and last."""
    B, H, W, C = shape
    rng = np.random.default_rng(B * 1000 + H)
    x = rng.standard_normal(shape).astype(F)
    flat = x.reshape(-1)
    at = rng.choice(flat.size, size=min(flat.size // 6, 6000), replace=False)
    special = np.array([0x7FC00000, 0xFFC00001, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000], np.uint32).view(F)
    flat[at] = special[np.arange(at.size) % 6]
    x[0, :3, :3, 0] = F(-0.0); x[0, 1, 1, 0] = F(0.0)                      # +0 behind -0: the first stays
    x[0, :3, :3, 1] = F(0.0); x[0, 2, 2, 1] = F(-0.0)
    x[0, :3, :3, 2] = special[0]; x[0, 2, 2, 2] = special[1]               # the last NaN met is the result
    x[0, :3, :3, 3] = F(-np.inf)
    return _frozen(x, maxpool3s2(x))
