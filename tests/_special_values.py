"""Operand plans with non-finite, subnormal and overflowing values for the trunk kernels, and the references they are compared with.  numpy and
the CPU oracle only (no torch, no GPU): tests/test_special_values_model.py asserts on the references alone that every case is non-vacuous,
tests/test_gpu_special_values.py runs the kernels on the same operands.

The base data of a case is what the case builders of tests/test_gpu_trunk_guards.py produce (same formulas and seeds).  A plan changes it:

  planted             NaNs (both signs, two payloads; neither is a poison or guard pattern of tests/_guards.py) and +-inf at sites that meet a
                      shortcut of the kernels: first / last element of a row, the last row, rows on both sides of a 64- and a 128-row tile border,
                      the first element of the row behind a finite row (what a one-sided k-tail fill would multiply by 0), corner / edge /
                      interior pixels of a map; the last k of one output channel and the centre tap of a 3x3 weight; one +inf bias; one -inf
                      residual under that bias and one NaN residual.
  subnormal_inputs    x 2^-130 (every input subnormal), weights as they are, bias and residual 2^-130.
  subnormal_products  x 2^-70, w 2^-66 (every PRODUCT subnormal, the operands normal), bias alternately 0 and subnormal, residual 2^-136.
  overflowing         x and w scaled to a product of 2^128 times the base data's: chains, chunk sums and the epilogue overflow.  A chain of finite
                      terms never gives NaN (a sum that reached +inf stays there: the exact product is finite); NaN needs two chunk sums of
                      opposite sign, i.e. a reduction longer than one chunk of 64.

Comparison rule (compare): the NaN positions are the same set, every other element equal bit for bit; NaN sign and payload are free; -0 folds onto
+0 only where the caller says so (max(-0, +0) of the bias / pool kernels under ReLU)."""
import functools

import numpy as np

import oracle as O

F = np.float32
PLANS = ("planted", "subnormal_inputs", "subnormal_products", "overflowing")
NAN_A = np.array([0x7FC12345], np.uint32).view(F)[0]          # +NaN; tests/_guards.py: poison 0x7FC0DEAD, operand guard 0x7FC0BEEF
NAN_B = np.array([0xFFD54321], np.uint32).view(F)[0]          # -NaN, another payload
PINF, NINF = F(np.inf), F(-np.inf)
TINY = F(2.0 ** -126)


def scale(a, e):
    """a * 2^e in fp32, one rounding (exact unless the result is subnormal or overflows)."""
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(np.asarray(a, F), e).astype(F)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def keeps_subnormals():
    return bool(F(1e-40) * F(0.5) != 0) and bool(np.ldexp(F(1), -140).astype(F) != 0)


# ---- comparison -------------------------------------------------------------------------------------------------------------------------------
def compare(got, want, what="", fold_zero_sign=False):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F, (what, got.shape, want.shape, got.dtype, want.dtype)
    gn, wn = np.isnan(got), np.isnan(want)
    bad = gn != wn
    assert not bad.any(), ("NaN positions differ", what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())
    gb, wb = bits(got), bits(want)
    if fold_zero_sign:
        gb, wb = np.where(gb == 0x80000000, 0, gb), np.where(wb == 0x80000000, 0, wb)
    bad = (gb != wb) & ~wn
    assert not bad.any(), ("bits differ", what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


# ---- non-vacuity conditions ---------------------------------------------------------------------------------------------------------------------
def stats(y):
    y = np.asarray(y, F).reshape(-1)
    a = np.abs(y)
    return dict(n=y.size, nan=int(np.isnan(y).sum()), pinf=int((y == PINF).sum()), ninf=int((y == NINF).sum()), zero=int((y == 0).sum()),
                sub=int(((a > 0) & (a < TINY)).sum()), finite=int(np.isfinite(y).sum()), nonzero=int((np.nan_to_num(a, nan=1.0) > 0).sum()))


def check_plan(plan, y, what="", can_nan=True, signed=True, ignore=None):
    """The conditions that keep a GPU comparison from passing emptily, on the reference output `y` (planted: the run WITHOUT ReLU).
    signed = False: outputs behind a ReLU (no -inf to ask for).  can_nan = False: an overflowing reduction that cannot give NaN (one chunk of
    finite terms) and must not; None: a case of one pixel, where it is a matter of luck.  ignore: mask of outputs left out (behind a ReLU: where the
    unscaled base data gives 0 as well -- a zero of the ReLU, not of a flush)."""
    y = np.asarray(y, F)
    s = stats(y if ignore is None else y[~ignore])
    if plan == "planted":
        assert s["nan"] >= 1 and s["pinf"] >= 1 and (s["ninf"] >= 1 or not signed), (what, s)
        assert 4 * s["nan"] <= s["n"], (what, s)
    elif plan.startswith("subnormal"):
        assert 10 * s["sub"] >= 9 * s["nonzero"] and 10 * s["zero"] < s["n"] and s["nan"] == 0, (what, s)
    else:
        assert s["pinf"] >= 1 and (s["ninf"] >= 1 or not signed) and 4 * (s["finite"] - s["zero"] * (not signed)) >= s["n"], (what, s)
        assert can_nan is None or (s["nan"] >= 1) == can_nan, (what, s)
    return s


# ---- planting -----------------------------------------------------------------------------------------------------------------------------------
def row_sites(M, Cin, map_shape=None, level=2, nan_in_x=True):
    """[(row, channel, value)] for activations seen as (M, Cin) rows.  level 2: every site; 1: corner, interior, last row; 0: none.
    NaNs sit in rows 0 and 128 only, so that most planted rows give infinities."""
    if level == 0:
        return []
    s = {}
    def put(r, c, v):
        if 0 <= r < M:
            s.setdefault((r, c), v)
    put(0, 0, PINF); put(0, Cin - 1, NAN_A if nan_in_x else NINF)           # first and last element of a row
    put(M - 1, 0, NINF)                                                   # last row; row M - 2 stays finite
    if map_shape is not None:
        B, H, W = map_shape
        if H >= 3 and W >= 3:
            put(((B - 1) * H + H // 2) * W + W // 2, Cin // 2, PINF)      # interior pixel of the last image
    if level >= 2:
        if M > 3:
            put(2, 0, PINF)                                               # row 1 is finite: its k tail must not reach this value
        if M > 64:
            put(63, Cin - 1, PINF); put(64, 0, NINF)
        if M > 128:
            put(127, Cin - 1, NINF); put(128, 0, NAN_B)
        if map_shape is not None and map_shape[2] >= 3:
            put(map_shape[2] // 2, 1, NINF)                               # edge pixel (row 0 of image 0)
    return [(r, c, v) for (r, c), v in s.items()]


def plant_rows(x, level=2, sites=None, nan_in_x=True):
    x = np.array(x, F)
    flat = x.reshape(-1, x.shape[-1])
    ms = x.shape[:3] if x.ndim == 4 else None
    for r, c, v in (row_sites(flat.shape[0], flat.shape[1], ms, level, nan_in_x) if sites is None else sites):
        flat[r, c] = v
    return x


def plant_weight(w, centre_only=False):
    """-NaN on the last k of the last output channel (3x3: the last k of the CENTRE tap when centre_only, where every row order agrees),
    +inf on the centre tap (1x1: the first k) of output channel 1."""
    w = np.array(w, F)
    Cout = w.shape[0]
    if w.ndim == 4:
        kh = w.shape[1] // 2
        w[1, kh, kh, 0] = PINF
        if centre_only:
            w[Cout - 1, kh, kh, -1] = NAN_B
        else:
            w[Cout - 1, -1, -1, -1] = NAN_B
    else:
        w[1, 0] = PINF
        w[Cout - 1, -1] = NAN_B
    return w


def plant_epilogue(b, r):
    """+inf bias on channel 2; residual: -inf under that bias in row 1 (inf - inf), -inf in channel 3 of row 0, NaN in row 1 channel 0."""
    b = np.array(b, F)
    b[2] = PINF
    if r is not None:
        r = np.array(r, F)
        rf = r.reshape(-1, r.shape[-1])
        if rf.shape[0] > 1:
            rf[1, 2] = NINF
        rf[0, 3] = NINF
        rf[min(1, rf.shape[0] - 1), 0] = NAN_A
    return b, r


def conv_plan(plan, x, w, b, r, level=2, centre_only=False, nan_in_x=True):
    """(x, w, b, r) of a convolution-like entry under `plan` (r may be None)."""
    if plan == "planted":
        b2, r2 = plant_epilogue(b, r)
        return plant_rows(x, level, nan_in_x=nan_in_x), plant_weight(w, centre_only), b2, r2
    if plan == "subnormal_inputs":
        return scale(x, -130), np.array(w, F), scale(b, -130), None if r is None else scale(r, -130)
    if plan == "subnormal_products":
        b2 = scale(b, -136)
        b2[::2] = 0
        return scale(x, -70), scale(w, -66), b2, None if r is None else scale(r, -136)
    assert plan == "overflowing"
    # a chunk of 64 terms of a reduction of K has a sum of about 2^128 sqrt(32 / K) with these scales (ReLU'd normals times normals / sqrt(K)):
    # past K = 128 one more power of two keeps single chunks overflowing (the source of inf - inf)
    K = int(np.prod(np.shape(w)[1:]))
    return scale(x, 62 + (K > 128)), scale(w, 66), scale(b, 125), None if r is None else scale(r, 125)


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False
    return arrays


def flags(plan):
    """The second axis of every case: planted runs with and without ReLU (always with the residual the entry takes); the other plans run
    without ReLU, with and without the residual.  -> [(residual, relu)]"""
    return [(True, True), (True, False)] if plan == "planted" else [(True, False), (False, False)]


# ---- isx_conv1x1_nhwc ---------------------------------------------------------------------------------------------------------------------------
C1_TILED = [(65, 32, 36), (129, 100, 130), (130, 64, 256)]
C1_TAIL = (133956, 64, 200)                       # tests/test_gpu_trunk_guards.py::test_conv1x1_tail_grid
C1_STREAM = [(16384 + 77, 64, 64), (16384 + 77, 64, 256)]


def c1_base(M, Cin, Cout):
    rng = np.random.default_rng(M * 7 + Cin * 3 + Cout)
    x = np.maximum(rng.standard_normal((M, Cin), dtype=F), 0)
    w = rng.standard_normal((Cout, Cin), dtype=F) * F(Cin ** -0.5)
    return x, w, rng.standard_normal(Cout, dtype=F), rng.standard_normal((M, Cout), dtype=F)


def c1_windows(M, split=None):
    """Rows the oracle evaluates of a large 1x1 case."""
    if split is None:
        return np.r_[0:200, M // 2:M // 2 + 200, M - 200:M]
    return np.r_[0:100, split - 100:split + 100, M - 100:M]


@functools.lru_cache(maxsize=4)
def c1_operands(M, Cin, Cout, plan, res, split=None):
    x, w, b, r = c1_base(M, Cin, Cout)
    if plan == "planted" and M > 1000:
        # large shapes: the sites of a small one at the start, around the tile border the case is about, and in the ragged last tile
        edge = split if split is not None else M // 2 + 64
        sites = row_sites(130, Cin) + [(edge - 1, Cin - 1, PINF), (edge, 0, NINF), (edge + 1, Cin // 2, NAN_B), (M - 70, 0, PINF), (M - 1, Cin - 1, NINF)]
        b2, r2 = plant_epilogue(b, r)
        ops = plant_rows(x, sites=sites), plant_weight(w), b2, r2
    else:
        ops = conv_plan(plan, x, w, b, r)
    return _frozen(ops[0], ops[1], ops[2], ops[3] if res else None)


@functools.lru_cache(maxsize=None)
def c1_reference(M, Cin, Cout, plan, res, relu, split=None):
    x, w, b, r = c1_operands(M, Cin, Cout, plan, res, split)
    rows = np.arange(M) if M < 1000 else c1_windows(M, split)
    return O.conv1x1_nhwc(x[rows], w, b, None if r is None else r[rows], relu)


# ---- isx_conv1x1_dual_nhwc ------------------------------------------------------------------------------------------------------------------------
DUAL = [(2, 9, 7, 32, 64, 130, 2), (2, 8, 6, 64, 64, 256, 1)]


def dual_base(B, H, W, K1, K2, Cout, stride):
    rng = np.random.default_rng(B + H * 10 + W + K1 + K2 + Cout + stride)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    t = np.maximum(rng.standard_normal((B, Ho, Wo, K1), dtype=F), 0)
    x = np.maximum(rng.standard_normal((B, H, W, K2), dtype=F), 0)
    w = rng.standard_normal((Cout, K1 + K2), dtype=F) * F((K1 + K2) ** -0.5)
    return t, x, w, rng.standard_normal(Cout, dtype=F)


@functools.lru_cache(maxsize=4)
def dual_operands(case, plan):
    """No residual in this entry: the second axis of a non-planted plan is only its ReLU.  x is planted at pixels the stride reads (and at
    one it skips: the output must not see it)."""
    B, H, W, K1, K2, Cout, stride = case
    t, x, w, b = dual_base(*case)
    if plan == "planted":
        t2, w2, b2, _ = conv_plan(plan, t, w, b, None, level=1)
        x2 = np.array(x, F)
        x2[0, 0, stride, K2 - 1] = NINF                       # stride 2: column 2 is read
        if stride == 2:
            x2[0, 1, 1, 0] = NAN_B                            # never read
            x2[B - 1, 2, 2, 0] = NAN_B
        else:
            x2[B - 1, 1, 1, 0] = NAN_B
        w2[3, K1] = NINF                                      # the first k of the second operand
        return _frozen(t2, x2, w2, b2)
    t2, w2, b2, _ = conv_plan(plan, t, w, b, None)
    x2 = conv_plan(plan, x, w, b, None)[0]
    return _frozen(t2, x2, w2, b2)


@functools.lru_cache(maxsize=None)
def dual_reference(case, plan, relu):
    t, x, w, b = dual_operands(case, plan)
    return O.conv1x1_dual_nhwc(t, x, w, b, case[6], relu)


# ---- isx_conv3x3_nhwc -----------------------------------------------------------------------------------------------------------------------------
C3_PIXEL = [(2, 3, 2, 32, 96, 2), (1, 9, 11, 64, 130, 2), (3, 5, 5, 64, 64, 1)]
C3_POSMAJ = [(129, 3, 5, 64, 128, 1), (129, 6, 5, 64, 128, 2)]


def c3_base(B, H, W, Cin, Cout, stride):
    rng = np.random.default_rng(B * 1000 + H * 100 + W * 10 + Cin + Cout + stride)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = np.maximum(rng.standard_normal((B, H, W, Cin), dtype=F), 0)
    w = rng.standard_normal((Cout, 3, 3, Cin), dtype=F) * F((9 * Cin) ** -0.5)
    return x, w, rng.standard_normal(Cout, dtype=F), rng.standard_normal((B, Ho, Wo, Cout), dtype=F)


def _c3_level(case):
    B, H, W, Cin, Cout, stride = case
    pixels = B * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
    return 2 if pixels >= 64 else 1


@functools.lru_cache(maxsize=4)
def c3_operands(case, plan, res):
    x, w, b, r = c3_base(*case)
    B, H, W, Cin, Cout, stride = case
    pixels = B * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
    ops = conv_plan(plan, x, w, b, r, level=_c3_level(case), centre_only=B >= 128, nan_in_x=pixels >= 16)
    return _frozen(ops[0], ops[1], ops[2], ops[3] if res else None)


@functools.lru_cache(maxsize=None)
def c3_reference(case, plan, res, relu):
    x, w, b, r = c3_operands(case, plan, res)
    return O.conv3x3_nhwc(x, w, b, case[5], r, relu)


def c3_padding_taps(H, W, stride):
    """(Ho, Wo, 3, 3) bool: tap (kh, kw) of output position (ho, wo) is padding."""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    hi = (np.arange(Ho) * stride - 1)[:, None] + np.arange(3)[None, :]
    wi = (np.arange(Wo) * stride - 1)[:, None] + np.arange(3)[None, :]
    outh, outw = (hi < 0) | (hi >= H), (wi < 0) | (wi >= W)
    return outh[:, None, :, None] | outw[None, :, None, :]


@functools.lru_cache(maxsize=None)
def c3_divergence(case, relu):
    """The documented divergence of the two row orders (csrc/conv3x3_tile.hpp): +inf on tap (0, 0) of output channel 5.
    -> (operands, pixel-major reference = the oracle, position-major reference = the oracle with that tap's weights 0 where the tap is padding)."""
    B, H, W, Cin, Cout, stride = case
    x, w, b, r = c3_base(*case)
    w = np.array(w, F)
    w[5, 0, 0, Cin // 2] = PINF
    plain = O.conv3x3_nhwc(x, w, b, stride, r, relu)
    w0 = np.array(w, F)
    w0[5, 0, 0, :] = 0
    zeroed = O.conv3x3_nhwc(x, w0[5:6], b[5:6], stride, np.ascontiguousarray(r[..., 5:6]), relu)
    pad00 = c3_padding_taps(H, W, stride)[:, :, 0, 0]
    skipped = np.array(plain, F)
    skipped[:, pad00, 5] = zeroed[:, pad00, 0]
    return _frozen(x, w, b, r), plain, skipped


# ---- fused expand kernels ---------------------------------------------------------------------------------------------------------------------------
EXPAND = [(1, 1, 1, 32, 1), (1, 9, 11, 32, 2), (2, 7, 7, 64, 1)]                   # B, H, W, Cin, stride  (64 mid channels -> 256)
EXPAND_DUAL = [(1, 1, 1, 32), (1, 9, 11, 32), (2, 7, 7, 64)]
EXPAND128 = [(1, 1, 1, 64, 128), (3, 7, 7, 64, 256), (129, 3, 5, 64, 128)]        # B, H, W, Cin, Cout; the last one runs position-major


def _mid_sites(x, stride):
    """x sites for a fused pair: a NaN of conv2 must meet the inner ReLU (mid = 0 there, the output finite), so x gets ONE NaN -- at the last
    pixel -- and one +inf at pixel 0 (mid = +inf or NaN -> 0 around it; the expansion then gives +-inf and NaN)."""
    B, H, W, Cin = x.shape
    M = B * H * W
    if M == 1:
        return []
    return [(M - 1, Cin - 1, NAN_A)] + ([(0, 0, PINF)] if M >= 49 else [])


def _expand_plan(plan, x, w2, b2, w3, b3, r, centre_only=False, stride=1):
    """Operands of conv3x3 (+ bias + ReLU) -> conv1x1 (+ bias (+ residual)) under `plan`.  The scaled plans act on the FIRST convolution
    for the inputs and on the second for the outputs: mid stays subnormal (or finite and huge), the expansion makes the outputs."""
    if plan == "planted":
        x2 = plant_rows(x, sites=_mid_sites(x, 1))
        w2p = plant_weight(w2, centre_only)
        b3p, rp = plant_epilogue(b3, r)
        w3p = np.array(w3, F)
        w3p[1, 0] = PINF
        w3p[-1, -1] = NAN_B
        return x2, w2p, np.array(b2, F), w3p, b3p, rp
    if plan == "subnormal_inputs":
        return scale(x, -130), np.array(w2, F), scale(b2, -130), np.array(w3, F), scale(b3, -130), None if r is None else scale(r, -130)
    if plan == "subnormal_products":
        b3s = scale(b3, -136)
        b3s[::2] = 0
        return scale(x, -35), scale(w2, -35), scale(b2, -70), scale(w3, -66), b3s, None if r is None else scale(r, -136)
    # the mid activation is the base data's times c 2^e, chosen from the oracle's base mid so that 2^128 falls just below the SECOND largest
    # value of the pixel where that value is largest: that pixel holds two +inf, which meet as inf - inf in the expansion, and few other pixels
    # hold any.  A case of one pixel keeps its mid finite (one +inf there makes every output non-finite).
    mid = O.conv3x3_nhwc(x, w2, b2, stride, None, True).reshape(-1, w2.shape[0])
    one = mid.shape[0] == 1
    t = 4 * float(mid.max()) if one else 0.999 * float(np.sort(mid, axis=1)[:, -2].max())
    e = int(np.ceil(128 - np.log2(t)))
    c = F(2.0 ** (128 - e) / t)
    ex, e2, e3 = e // 2, e - e // 2, 127 - e + (3 if w3.shape[1] <= 64 else 2) * one
    w2, b2 = w2 * c, b2 * c
    return scale(x, ex), scale(w2, e2), scale(b2, ex + e2), scale(w3, e3), scale(b3, 125), None if r is None else scale(r, 125)


def expand_base(B, H, W, Cin, stride):
    rng = np.random.default_rng(B * 100 + H + Cin)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = np.maximum(rng.standard_normal((B, H, W, Cin), dtype=F), 0)
    w2 = rng.standard_normal((64, 3, 3, Cin), dtype=F) * F((9 * Cin) ** -0.5)
    b2 = rng.standard_normal(64, dtype=F)
    w3 = rng.standard_normal((256, 64), dtype=F) * F(0.125)
    b3 = rng.standard_normal(256, dtype=F)
    r = rng.standard_normal((B, Ho, Wo, 256), dtype=F)
    return x, w2, b2, w3, b3, r


@functools.lru_cache(maxsize=4)
def expand_operands(case, plan, res):
    ops = _expand_plan(plan, *expand_base(*case), stride=case[4])
    return _frozen(*ops[:5], ops[5] if res else None)


@functools.lru_cache(maxsize=None)
def expand_reference(case, plan, res, relu):
    """-> (mid, y): the oracle's composition."""
    x, w2, b2, w3, b3, r = expand_operands(case, plan, res)
    mid = O.conv3x3_nhwc(x, w2, b2, case[4], None, True)
    y = O.conv1x1_nhwc(mid.reshape(-1, 64), w3, b3, None if r is None else r.reshape(-1, 256), relu)
    return mid, y.reshape(mid.shape[:3] + (256,))


def expand_dual_base(B, H, W, Cin):
    rng = np.random.default_rng(B * 10 + H + Cin)
    t = np.maximum(rng.standard_normal((B, H, W, Cin), dtype=F), 0)
    x2 = np.maximum(rng.standard_normal((B, H, W, 64), dtype=F), 0)
    w2 = rng.standard_normal((64, 3, 3, Cin), dtype=F) * F((9 * Cin) ** -0.5)
    b2 = rng.standard_normal(64, dtype=F)
    wc = rng.standard_normal((256, 128), dtype=F) * F(128 ** -0.5)
    b = rng.standard_normal(256, dtype=F)
    return t, x2, w2, b2, wc, b


@functools.lru_cache(maxsize=4)
def expand_dual_operands(case, plan):
    """(t, w2, b2, x2, wc, b): the shortcut operand x2 gets the scale of mid (it shares mid's reduction)."""
    t, x2, w2, b2, wc, b = expand_dual_base(*case)
    tp, w2p, b2p, wcp, bp, _ = _expand_plan(plan, t, w2, b2, wc, b, None)
    if plan == "planted":
        x2p = np.array(x2, F)
        if x2p.shape[0] * x2p.shape[1] * x2p.shape[2] > 4:
            x2p.reshape(-1, 64)[3, 63] = NINF
        wcp[3, 64] = NINF
    else:
        x2p = scale(x2, {"subnormal_inputs": -130, "subnormal_products": -70, "overflowing": 124}[plan])
    return _frozen(tp, w2p, b2p, x2p, wcp, bp)


@functools.lru_cache(maxsize=None)
def expand_dual_reference(case, plan, relu):
    t, w2, b2, x2, wc, b = expand_dual_operands(case, plan)
    mid = O.conv3x3_nhwc(t, w2, b2, 1, None, True)
    return mid, O.conv1x1_dual_nhwc(mid, x2, wc, b, 1, relu)


def e128_base(B, H, W, Cin, Cout):
    rng = np.random.default_rng(B * 100 + H * 10 + W + Cin + Cout)
    x = np.maximum(rng.standard_normal((B, H, W, Cin), dtype=F), 0)
    w2 = rng.standard_normal((128, 3, 3, Cin), dtype=F) * F((9 * Cin) ** -0.5)
    b2 = rng.standard_normal(128, dtype=F)
    w3 = rng.standard_normal((Cout, 128), dtype=F) * F(128 ** -0.5)
    return x, w2, b2, w3, rng.standard_normal(Cout, dtype=F), rng.standard_normal((B, H, W, Cout), dtype=F)


@functools.lru_cache(maxsize=4)
def e128_operands(case, plan, res):
    ops = _expand_plan(plan, *e128_base(*case), centre_only=case[0] >= 128)
    return _frozen(*ops[:5], ops[5] if res else None)


@functools.lru_cache(maxsize=None)
def e128_reference(case, plan, res, relu):
    x, w2, b2, w3, b3, r = e128_operands(case, plan, res)
    Cout = w3.shape[0]
    mid = O.conv3x3_nhwc(x, w2, b2, 1, None, True)
    y = O.conv1x1_nhwc(mid.reshape(-1, 128), w3, b3, None if r is None else r.reshape(-1, Cout), relu)
    return mid, y.reshape(mid.shape[:3] + (Cout,))


# ---- isx_stem7x7_pool_nhwc --------------------------------------------------------------------------------------------------------------------------
STEM = [(1, 17, 12), (2, 50, 36), (1, 9, 228)]
STEM_VALUES = {"pinf": PINF, "ninf": NINF, "nan": NAN_A}


def stem_base(B, H, W):
    rng = np.random.default_rng(H * 1000 + W + B)
    x = rng.standard_normal((B, H, W, 3), dtype=F)
    w = rng.standard_normal((64, 7, 7, 3), dtype=F) * F(147 ** -0.5)
    return x, w, rng.standard_normal(64, dtype=F)


def stem_sites(B, H, W):
    """(image, row, column) of the planted pixels: an even and an odd interior column, columns 0, 4 and W - 1, the first and the last row, and
    on an image of two column bands the columns on both sides of the band border at 224."""
    b, hm = B - 1, H // 2
    s = [(b, hm, 6), (b, hm, 7), (0, hm, 0), (0, hm, 4), (b, hm, W - 1), (0, 0, 8), (b, H - 1, 5)]
    if W > 224:
        s += [(0, hm, 223), (0, hm, 224)]
    return s


def stem_planted(case, value, channel, site=None):
    """x with STEM_VALUES[value] in `channel` of one site (index into stem_sites) or of all of them."""
    x, w, b = stem_base(*case)
    x = np.array(x, F)
    sites = stem_sites(*case)
    for i, r, c in (sites if site is None else [sites[site]]):
        x[i, r, c, channel] = STEM_VALUES[value]
    return x, w, b


def stem_model(x, w, b, slot=True):
    """isx_stem7x7_pool_nhwc as include/isx.h states it for a non-finite input: the oracle's sums (_alex_model.conv2d in chunks of three filter
    rows, then the oracle's pool), and at the end of each filter row the kernel's zero-weight k slot fma(x[hi][2 wo + 4][0], 0, acc) -- NaN for
    a non-finite x, so that the convolution outputs (ho, wo, every channel) whose rows hold that input row become max(NaN, 0) = 0.  Outside the
    image the slot reads the staged zero border.  slot = False: the oracle's composition alone (the CPU test holds it against the oracle)."""
    import _alex_model as A
    x = np.asarray(x, F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        y = np.array(A.conv2d(x, w, b, 2, 3, True, chunk=63), F)
    B, H, W, _ = x.shape
    Hc, Wc = y.shape[1:3]
    bad = ~np.isfinite(x[..., 0])
    if slot and bad.any():
        for ho in range(Hc):
            rows = [hi for hi in range(2 * ho - 3, 2 * ho + 4) if 0 <= hi < H]
            for wo in range(Wc):
                if 2 * wo + 4 < W:
                    y[bad[:, rows, 2 * wo + 4].any(1), ho, wo, :] = 0
    return O.bias_relu_maxpool_nhwc(y, np.zeros(64, F))


@functools.lru_cache(maxsize=None)
def stem_reference(case, value, channel, site=None, slot=True):
    return stem_model(*stem_planted(case, value, channel, site), slot=slot)


def stem_scaled(case, plan):
    x, w, b = stem_base(*case)
    if plan == "subnormal_inputs":
        return scale(x, -130), w, scale(b, -130)
    if plan == "subnormal_products":
        b2 = scale(b, -136)
        b2[::2] = 0
        return scale(x, -70), scale(w, -66), b2
    return scale(x, 61), scale(w, 66), scale(b, 125)


@functools.lru_cache(maxsize=None)
def stem_scaled_reference(case, plan):
    return O.stem7x7_pool_nhwc(*stem_scaled(case, plan))


# ---- isx_bias_relu_maxpool_nhwc / isx_bias_act_inplace -------------------------------------------------------------------------------------------
POOL = [(1, 1, 1, 4), (2, 7, 9, 8), (2, 12, 13, 36)]
BIAS_ACT = [(35, 5, 1), (60, 5, 6), (64, 8, 1), (64, 2, 8)]                         # n, C, inner


def pool_operands(case, plan):
    B, H, W, C = case
    rng = np.random.default_rng(H + C)
    y = rng.standard_normal((B, H, W, C), dtype=F)
    b = rng.standard_normal(C, dtype=F)
    if plan == "planted":
        y = np.array(y, F)
        if H >= 7:
            y[0, 1:4, 1:4, 0] = F(-3)                        # a NaN alone among values the ReLU zeroes: the window gives 0
            y[0, 2, 2, 0] = NAN_A
            y[0, 4, 4, 1] = NAN_B                            # next to larger values
            y[0, 4, 5, 1] = F(5)
            y[B - 1, H - 1, W - 1, 2] = NAN_A                # the last element of the map
            y[B - 1, 0, 0, 3] = PINF
            y[0, 3, 6, 3] = NINF
            y[0, 6, 0, 1] = PINF; y[0, 6, 1, 1] = NAN_A      # NaN next to +inf
            b = np.array(b, F)
            b[C - 1] = PINF
            y[0, 2, 2, C - 1] = NINF                         # -inf + inf = NaN -> 0 alone... next to +inf
        else:
            y[0, 0, 0, 0] = NAN_A                            # the only element of its window
            y[0, 0, 0, 1] = PINF
            y[0, 0, 0, 2] = NINF
        return y, b
    if plan == "subnormal_inputs":
        return scale(y, -130), scale(b, -130)
    if plan == "subnormal_products":
        b2 = scale(b, -136)
        b2[::2] = 0
        return scale(y, -136), b2
    return scale(y, 127), scale(b, 127)


@functools.lru_cache(maxsize=None)
def pool_base_reference(case):
    B, H, W, C = case
    rng = np.random.default_rng(H + C)
    return O.bias_relu_maxpool_nhwc(rng.standard_normal((B, H, W, C), dtype=F), rng.standard_normal(C, dtype=F))


@functools.lru_cache(maxsize=None)
def pool_reference(case, plan):
    return O.bias_relu_maxpool_nhwc(*pool_operands(case, plan))


def bias_act_operands(case, plan, res):
    n, C, inner = case
    rng = np.random.default_rng(n + C)
    y0, b = rng.standard_normal(n, dtype=F), rng.standard_normal(C, dtype=F)
    r = rng.standard_normal(n, dtype=F)
    if plan == "planted":
        y0, b, r = np.array(y0), np.array(b), np.array(r)
        y0[0] = NAN_A; y0[n - 1] = NAN_B; y0[3] = PINF; y0[6] = NINF; y0[n // 2] = PINF
        r[n // 2] = NINF                                      # inf - inf
        r[7] = NAN_B
        b[C - 1] = PINF
        y0[5], r[5] = F(-0.0), F(-0.0)                        # with b[ch] possibly non-zero: ordinary; the zero-sign case proper is below
    elif plan == "subnormal_inputs":
        y0, b, r = scale(y0, -130), scale(b, -130), scale(r, -130)
    elif plan == "subnormal_products":
        y0, b, r = scale(y0, -136), scale(b, -136), scale(r, -136)
        b[::2] = 0
    else:
        y0, b, r = scale(y0, 127), scale(b, 127), scale(r, 127)
    return y0, b, (r if res else None)


def bias_act_reference(case, plan, res, relu):
    """Unfused fp32 adds in the kernels' order; ReLU as fmaxf(v, 0): a NaN gives 0."""
    n, C, inner = case
    y0, b, r = bias_act_operands(case, plan, res)
    with np.errstate(invalid="ignore", over="ignore"):
        v = y0 + b[(np.arange(n) // inner) % C]
        v = v + r if res else v
        return (np.where(v > 0, v, F(0)) if relu else v).astype(F)


# ---- isxa_conv2d_nhwc (tests/_alex_model.py) --------------------------------------------------------------------------------------------------------
ALEX = ["11x11s4_3to64", "5x5_64to192"]


@functools.lru_cache(maxsize=None)
def alex_operands(name):
    """The planted plan on a case of _alex_model.CONV_CASES: x sites as for a map, the weight's centre tap and last k, one +inf bias."""
    import _alex_model as A
    x, w, bias = A.conv_inputs(name)
    bias = np.array(bias, F)
    bias[2] = PINF
    return _frozen(plant_rows(x, level=1 if w.shape[1] * w.shape[1] * 4 > x.shape[1] * x.shape[2] else 2), plant_weight(w), bias)


@functools.lru_cache(maxsize=None)
def alex_reference(name, relu):
    import _alex_model as A
    x, w, bias = alex_operands(name)
    with np.errstate(invalid="ignore", over="ignore"):
        return A.conv2d(x, w, bias, A.CONV_CASES[name][6], A.CONV_CASES[name][7], relu)


# ---- the suffix backward kernels (tests/_suffix_model.py) ------------------------------------------------------------------------------------------
# The base data here is plain standard normals, not _suffix_model's inputs(): its columns span four decades each way, more than the 23 binades of
# the subnormal range, so no single scale would put a whole output there.  The chains are the model's; only the data differs.
WGRAD = {"1x1_short_and_empty_split": 10, "3x3_three_leaves": 2}         # name -> splits (isx_conv_wgrad_splits; the GPU test asserts them)
DGRAD1 = [(65, 100, 80), (129, 100, 80)]                                 # M, Cin, Cout
DGRAD3 = ["2x2", "W1"]
COL2IM = [(3, 2, 2, 4), (2, 7, 9, 8)]
RELU_N = [8, 1028]
FOLD = [(1, 64, 1, 3), (9, 64, 1, 3)]                                    # taps, Cin, leaves, S: the direct and the LDS path


def _normal(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(F)


def pair_plan(plan, a, b, K):
    """Two operands of a chain of K products of unit normals (its sum is about sqrt(K)) under one of the scaled plans."""
    lg = int(np.ceil(np.log2(K) / 2))
    if plan == "subnormal_inputs":
        return scale(a, -130 - lg), np.array(b, F)
    if plan == "subnormal_products":
        return scale(a, -70), scale(b, -66 - lg)
    assert plan == "overflowing"
    return scale(a, 62), scale(b, 66 - lg)


def out_exponent(plan, K=1):
    """The exponent that puts a unit normal at the size of pair_plan's outputs (operands added behind the chain)."""
    return {"subnormal_inputs": -130, "subnormal_products": -136, "overflowing": 125}[plan]


def quiet(f):
    @functools.wraps(f)
    def g(*a, **k):
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            return f(*a, **k)
    return g


@functools.lru_cache(maxsize=None)
def wgrad_operands(name, plan):
    """(dz (B Ho Wo, Cout), x (B H W, Cin)).  planted: a non-finite dz at pixel 0 of a 3x3 case meets padding taps -- the model's gather_rows puts
    a +0 row there, fma(inf, 0, acc) = NaN, and the kernel must give NaN too."""
    import _suffix_model as M
    g, Cin, Cout, leaves, _ = M.WGRAD_CASES[name]
    Ho, Wo = M.out_hw(g)
    K = M.wgrad_K(name)
    n = sorted(M.WGRAD_CASES).index(name)
    dz, x = _normal((g.B * Ho * Wo, Cout), 900 + n), _normal((g.B * g.H * g.W, Cin), 950 + n)
    if plan == "planted":
        per = M.split_ranges(K, WGRAD[name])[1][0][1]                    # pixels of split 0
        dz[0, 0] = PINF; dz[per - 1, 1] = NAN_A; dz[per, 2] = NINF; dz[K // 2, 3] = NAN_B; dz[-1, Cout - 1] = NINF
        x[0, 1] = NINF; x[-1, Cin - 1] = PINF; x[g.W + 1, 2] = NAN_B
        return _frozen(dz, x)
    return _frozen(*pair_plan(plan, dz, x, 160))


def zero_fill_term(v):
    """fma(+0, +0, acc) = acc + (+0): the term a gradient kernel adds for every slot that pads its reduction to a whole k-tile (both operands
    are zero-filled), and what the input-gradient epilogue adds for its absent bias.  It leaves every acc as it is but -0, which becomes +0
    (special values).  The forward kernels add the same terms; their second-level sum tot = +0 + chain hides it."""
    return v + F(0)


@functools.lru_cache(maxsize=None)
@quiet
def wgrad_reference(name, plan):
    """_suffix_model.wgrad_partials, and for every split whose pixel count is no multiple of the k-tile (32 pixels) the zero-filled slots of its
    last k-tile."""
    import _suffix_model as M
    g, Cin, Cout, leaves, which = M.WGRAD_CASES[name]
    dz, x = wgrad_operands(name, plan)
    dw, db = M.wgrad_partials(dz, x, g, leaves, WGRAD[name], which)
    for s_, (lo, hi) in enumerate(M.split_ranges(M.wgrad_K(name), WGRAD[name])[1]):
        if (hi - lo) % M.BK:
            dw[:, s_] = zero_fill_term(dw[:, s_])
    return dw, db


@functools.lru_cache(maxsize=None)
def dgrad1_operands(M_, Cin, Cout, plan):
    """(dz (M, Cout), wt (Cin, Cout), add (M, Cin), mask (M, Cin)).  The reduction runs over Cout = 80: the last k-tile of 32 is zero-filled."""
    import _suffix_model as M
    dz, wt, add = _normal((M_, Cout), 7 * M_ + Cout), _normal((Cin, Cout), 7 * M_ + Cout + 1), _normal((M_, Cin), 7 * M_ + Cout + 2)
    mask = np.array(M.mask_data((M_, Cin), 7 * M_ + Cout + 3), F)
    if plan == "planted":
        dz = plant_rows(dz)
        wt[1, 0] = PINF; wt[Cin - 1, Cout - 1] = NAN_B
        add[1, 2] = NINF; add[1, 0] = NAN_A; add[4, 3] = PINF
        mask[0, 5] = NAN_A; mask[0, 6] = NAN_B                           # a NaN in the mask selects 0 (row 0 of the sum is NaN)
        mask[M_ - 1, 0] = PINF; mask[M_ - 1, 1] = NINF
        return _frozen(dz, wt, add, mask)
    dz, wt = pair_plan(plan, dz, wt, Cout)
    return _frozen(dz, wt, scale(add, out_exponent(plan) - 2), mask)


@functools.lru_cache(maxsize=None)
@quiet
def dgrad1_reference(M_, Cin, Cout, plan, with_add, with_mask, raw=False):
    """_suffix_model.dgrad1x1 with one more term behind the chain: the epilogue it shares with the inference kernels adds its absent bias as +0
    (csrc/gemm_tile.hpp conv_epilogue_buffers), as the zero-filled slots of the last k-tile do under every tile shape but the 128x128 one.
    raw: without that term (what the CPU test looks at to see that the data holds chains ending on -0)."""
    import _suffix_model as M
    dz, wt, add, mask = dgrad1_operands(M_, Cin, Cout, plan)
    v = M.chains(dz, wt)
    if not raw:
        v = zero_fill_term(v)
    if with_add:
        v = v + add
    return M.masked(v, mask if with_mask else None)


@functools.lru_cache(maxsize=None)
def dgrad3_operands(name, plan):
    """(dz (B, H, W, Cout), wt (Cin, 3, 3, Cout), mask (B, H, W, Cin))."""
    import _suffix_model as M
    B, H, W, Cout, Cin, _ = M.DGRAD3_CASES[name]
    n = sorted(M.DGRAD3_CASES).index(name)
    dz, wt = _normal((B, H, W, Cout), 800 + n), _normal((Cin, 3, 3, Cout), 850 + n)
    mask = np.array(M.mask_data((B, H, W, Cin), 870 + n), F)
    if plan == "planted":
        # a pixel of dz reaches every pixel of a 2x2 map and three of five of a 5x1 one: dz gets infinities only, in two images; the NaNs
        # come from the weight (one input channel) and the mask
        dz[0, 0, 0, 0] = PINF
        dz[B - 1, H - 1, W - 1, Cout - 1] = NINF
        wt = plant_weight(wt)
        mask[0, 0, 0, 0] = NAN_B; mask[0, 0, 0, 2] = NINF
        return _frozen(dz, wt, mask)
    return _frozen(*pair_plan(plan, dz, wt, 9 * Cout), mask)


@functools.lru_cache(maxsize=None)
@quiet
def dgrad3_reference(name, plan, with_mask):
    import _suffix_model as M
    dz, wt, mask = dgrad3_operands(name, plan)
    return M.masked(zero_fill_term(M.dgrad3x3(dz, wt, None)), mask if with_mask else None)        # the absent bias of the shared epilogue: + (+0)


@functools.lru_cache(maxsize=None)
def col2im_operands(case, plan):
    """(dcol (B Ho Wo, 9, Cin), mask).  planted: +inf and -inf that meet in input pixel (1, 1) where the map has one, alone elsewhere."""
    import _suffix_model as M
    B, H, W, Cin = case
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dcol = _normal((B * Ho * Wo, 9, Cin), 1000 * H + 10 * W + B)
    mask = np.array(M.mask_data((B, H, W, Cin), 1000 * H + 10 * W + B + 1), F)
    if plan == "planted":
        dcol[0, 4, 0] = PINF; dcol[0, 0, 1] = NAN_A; dcol[-1, 4, Cin - 1] = NINF; dcol[-1, 4, 1] = NAN_B
        dcol[0, 8, 3] = PINF; dcol[1, 6 if Wo > 1 else 8, 3] = NINF
        mask[0, 0, 0, 0] = NAN_A
        return _frozen(dcol, mask)
    return _frozen(scale(dcol, out_exponent(plan) + (plan == "overflowing")), mask)


@functools.lru_cache(maxsize=None)
@quiet
def col2im_reference(case, plan, with_mask):
    import _suffix_model as M
    dcol, mask = col2im_operands(case, plan)
    return M.col2im_s2(dcol, *case, mask if with_mask else None)


@functools.lru_cache(maxsize=None)
def relu_operands(n, plan):
    """(dy, y).  The kernel only selects: a subnormal y > 0 lets dy through (a flushed one would not), a NaN y selects 0."""
    import _suffix_model as M
    dy, y = _normal(n, n), np.array(M.mask_data((n,), n + 1), F)
    if plan == "planted":
        dy[0], y[0] = NAN_A, F(1)
        dy[1], y[1] = NAN_B, F(-1)
        dy[2], y[2] = PINF, NAN_A
        dy[3], y[3] = NINF, PINF
        dy[4], y[4] = PINF, F(2)
        dy[6], y[6] = F(1), NINF
        dy[n - 1], y[n - 1] = NINF, TINY
        return _frozen(dy, y)
    e = out_exponent(plan)
    return _frozen(scale(dy, e), scale(y, min(e, -130)))


@functools.lru_cache(maxsize=None)
@quiet
def relu_reference(n, plan):
    import _suffix_model as M
    return M.relu_grad(*relu_operands(n, plan))


@functools.lru_cache(maxsize=None)
def fold_operands(case, plan):
    """(dwp (leaves, S, Cout, taps, Cin), db (leaves, S, Cout), w (Cout, Cin, taps), scale, mean, istd).  planted: +inf and -inf in two partials
    of one element (their sum is NaN), NaN and -inf alone, +inf and NaN in db."""
    import _suffix_model as M
    taps, Cin, leaves, S = case
    Cout = M.FOLD_COUT
    dwp, db = _normal((leaves, S, Cout, taps, Cin), 31 * Cin + taps), _normal((leaves, S, Cout), 31 * Cin + taps + 1)
    w, sc, mean, istd = (np.array(a, F) for a in M.fold_params(taps, Cin))
    w = _normal(w.shape, 31 * Cin + taps + 2)
    if plan == "planted":
        dwp[0, 0, 0, 0, 0] = PINF; dwp[0, 1, 0, 0, 0] = NINF
        dwp[0, 0, 1, 0, 1] = NAN_A
        dwp[0, S - 1, 2, taps - 1, Cin - 1] = NINF
        dwp[0, 0, 5, 0, 2] = PINF
        db[0, 0, 3] = PINF; db[0, 1, 4] = NAN_B
        return _frozen(dwp, db, w, sc, mean, istd)
    dwp, w = pair_plan(plan, dwp, w, taps * Cin)
    return _frozen(dwp, scale(db, out_exponent(plan) - 2), w, sc, mean, istd)


@functools.lru_cache(maxsize=None)
@quiet
def fold_reference(case, plan):
    import _suffix_model as M
    dwp, db, w, sc, mean, istd = fold_operands(case, plan)
    return M.fold_backward(dwp, db, w, sc, mean, istd, case[0])
