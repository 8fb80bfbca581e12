"""CPU model of the sums of the descriptor kernels (csrc/pool.hip: L2 row normalisation with and without Shift, its backward, global average
pool + L2 in both layouts; csrc/region.hip: best-location descriptor and window gather + L2 in both layouts), shared by
tests/test_desc_model.py (the model against float64 and the oracle, and against the wrong variants it has to tell apart) and
tests/test_gpu_desc_chains.py (the kernels against the model, bit for bit).  It imports nothing from the library.

Every add, multiply, divide and square root is a numpy float32 operation: one rounding each, never fused -- libisx is built with
-ffp-contract=off, and hipcc rounds fp32 division and sqrtf correctly by default (the GPU test sweeps both first).

The pieces.
  strided partials   thread t of NT adds its terms j = t, t + NT, ... in ascending order into an accumulator that starts at +0
  wave butterfly     64 lanes meet in the xor butterfly 32, 16, 8, 4, 2, 1 (v = v[:o] + v[o:2o]: an add commutes, every lane ends on the same value)
  block_sum<NT>      the butterfly in each of the NT / 64 waves, then the wave sums added in wave order from +0
  float4 term        x*x + y*y + z*z + w*w left to right, ONE term of its thread (the vector row kernels, gap_l2 NHWC); the NHWC gather adds the
                     four squares to its accumulator one by one instead

Which kernel runs is a function of the shape and of the pointers' alignment, never of the batch: l2norm_kernel(D, aligned), gap_plan(B, C, HW)
(B chooses the channels per pass, which only changes how the map is staged), gap_nhwc_plan(C, aligned).  The non-temporal variant of the NHWC
kernel (maps above 192 MB) has the same arithmetic and is left to the bench, whose 1024 x 2048 x 7 x 7 step runs it.

Signed zeros.  The scalar row kernel and both gather kernels add `shift ? shift[j] : 0.0f`: without a Shift a quotient of -0 comes out as +0.
The wave and vector row kernels add nothing without a Shift and keep -0.  The case data holds a -0 to pin that.

Forward bounds against float64 (u = 2^-24), used by test_desc_model.py, derived, not measured.
  Sum of squares.  Every term is >= 0, so each rounding on the way multiplies what it holds by (1 + e), |e| <= u, and the relative error of ss
  is at most k u to first order, k = the roundings on the longest path from an input to ss: 1 (the square) + 3 (inside a float4 term, vector
  kernels; the one-by-one adds of the NHWC gather are counted in the next item) + the adds of the thread's accumulator (ceil(terms / NT), the
  exact first add to +0 counted: it covers the second-order terms) + 6 (butterfly) + NT / 64 (wave sums; none in the wave kernel).  ss_depth().
  Row.  ss + eps is one more rounding on positive numbers (k + 1), the square root halves the relative error and adds one, the division adds
  one:  |y - y64| <= ((k + 1) / 2 + 2 + 1) u |y64|  (the last + 1 for second order), plus u |y64 + shift| for the Shift's add.  row_bound().
  Pooling.  A pooled mean is HW - 1 adds and a division of values of either sign: |p - p64| <= HW u sum_i |v_i| / HW (in order), resp.
  (ceil(HW / 64) + 6 + 1) u sum_i |v_i| / HW (lane-strided + butterfly).  The L2 stage is then compared from the model's OWN fp32 pooled values,
  with the row bound above: two stages, each against float64 of the same stage.
  Backward.  dx = (n2 dy - x c) inv, n2 = ss + eps (k2 = ss_depth + 1 roundings, relative), c = sum x dy (kc = 1 + ceil(D / 1024) + 6 + 16
  roundings, absolute error kc u sum |x dy|), inv = 1 / (n2 sqrt(n2)): relative error 1.5 k2 + 3 (n2^1.5, sqrt, product, reciprocal).  With the two
  products, the difference and the last product:
    |dx - dx64| <= u inv64 [ (k2 + 1.5 k2 + 3 + 3 + 1) (n2 |dy| + |x| |c64|) + |x| kc sum |x dy| ].  bwd_bound()."""
import functools

import numpy as np

F = np.float32
U = 2.0 ** -24
LANES = 64
EPS = 1e-10


# ---- the pieces ---------------------------------------------------------------------------------------------------------------------------------
def strided_partials(t, nt):
    """(B, n) terms -> (B, nt): thread k's sequential sum over j = k, k + nt, ... from +0; a thread past n keeps its +0."""
    B, n = t.shape
    v = np.zeros((B, nt), F)
    for j0 in range(0, n, nt):
        w = min(nt, n - j0)
        v[:, :w] = v[:, :w] + t[:, j0:j0 + w]
    return v


def wave_butterfly(v):
    """(..., 64) -> (...): xor 32, 16, ..., 1."""
    o = LANES // 2
    while o:
        v = v[..., :o] + v[..., o:2 * o]
        o //= 2
    return v[..., 0]


def block_sum(v):
    """(B, NT) per-thread values -> (B,): block_sum<NT> of isx_common.hpp."""
    B, nt = v.shape
    w = wave_butterfly(v.reshape(B, nt // LANES, LANES))
    t = np.zeros(B, F)
    for i in range(nt // LANES):
        t = t + w[:, i]
    return t


def float4_terms(x):
    """(B, 4 n) -> (B, n): x*x + y*y + z*z + w*w, left to right."""
    q = np.asarray(x, F).reshape(x.shape[0], -1, 4)
    s = q * q
    return ((s[:, :, 0] + s[:, :, 1]) + s[:, :, 2]) + s[:, :, 3]


def _sqrt(v):
    with np.errstate(all="ignore"):
        return np.sqrt(v)


def _div(a, b):
    with np.errstate(all="ignore"):
        return a / b


# ---- isx_l2norm_rows / isx_l2norm_shift_rows (launch_l2norm) --------------------------------------------------------------------------------------
def l2norm_kernel(D, aligned):
    """The dispatch of launch_l2norm.  aligned: x, y and shift (when given) are all 16-byte aligned."""
    if aligned and D % 4 == 0:
        if D <= 256:
            return "wave1"
        if D <= 512:
            return "wave2"
        if D <= 1024:
            return "wave4"
        if D <= 2048:
            return "wave8"
        return "block_vec"
    return "block_scalar"


def l2norm_ss(x, kernel):
    x = np.asarray(x, F)
    if kernel.startswith("wave"):
        return wave_butterfly(strided_partials(float4_terms(x), LANES))
    if kernel == "block_vec":
        return block_sum(strided_partials(float4_terms(x), 1024))
    assert kernel == "block_scalar"
    return block_sum(strided_partials(x * x, 1024))


def finish_rows(x, ss, eps, shift, adds_zero):
    """n = sqrt(ss + eps), y = x / n (+ shift); adds_zero: the kernel adds +0 where there is no Shift."""
    n = _sqrt(ss + F(eps))
    y = _div(np.asarray(x, F), n[:, None])
    if shift is not None:
        y = y + np.asarray(shift, F)
    elif adds_zero:
        y = y + F(0)
    return y


def l2norm_rows(x, eps=EPS, shift=None, aligned=True):
    k = l2norm_kernel(x.shape[1], aligned)
    return finish_rows(x, l2norm_ss(x, k), eps, shift, k == "block_scalar")


def ss_depth(kernel, n):
    """Roundings on the longest path from an input to ss (module docstring); n = elements of the row."""
    nt, quad, waves = {"wave": (64, 3, 0), "block_vec": (1024, 3, 16), "block_scalar": (1024, 0, 16), "block256": (256, 0, 4),
                       "nhwc512": (512, 3, 8), "gather_nhwc": (1024, 3, 16)}["wave" if kernel.startswith("wave") else kernel]
    terms = (n + 3) // 4 if quad else n
    adds = (terms + nt - 1) // nt
    if kernel == "gather_nhwc":                   # the four squares of a float4 go into the accumulator one by one
        quad, adds = 0, 4 * adds
    return 1 + quad + adds + 6 + waves


def row_bound(y64, depth, shifted64=None):
    b = ((depth + 1) / 2.0 + 3) * U * np.abs(y64)
    return b if shifted64 is None else b + U * np.abs(shifted64)


def l2norm_rows64(x, eps=EPS, shift=None):
    x = np.asarray(x, np.float64)
    y = x / np.sqrt((x * x).sum(1) + float(F(eps)))[:, None]
    return y if shift is None else y + np.asarray(shift, np.float64)


# ---- isx_l2norm_rows_bwd ------------------------------------------------------------------------------------------------------------------------------
def l2norm_rows_bwd(x, dy, eps=EPS):
    x, dy = np.asarray(x, F), np.asarray(dy, F)
    n2 = block_sum(strided_partials(x * x, 1024)) + F(eps)
    c = block_sum(strided_partials(x * dy, 1024))
    inv = _div(F(1), n2 * _sqrt(n2))
    return (n2[:, None] * dy - x * c[:, None]) * inv[:, None]


def l2norm_rows_bwd64(x, dy, eps=EPS):
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    n2 = (x * x).sum(1) + float(F(eps))
    c = (x * dy).sum(1)
    return (n2[:, None] * dy - x * c[:, None]) / (n2 * np.sqrt(n2))[:, None]


def bwd_bound(x, dy, eps=EPS):
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    D = x.shape[1]
    k2 = ss_depth("block_scalar", D) + 1
    kc = 1 + (D + 1023) // 1024 + 6 + 16
    n2 = (x * x).sum(1) + float(F(eps))
    c = (x * dy).sum(1)
    inv = 1.0 / (n2 * np.sqrt(n2))
    size = n2[:, None] * np.abs(dy) + np.abs(x) * np.abs(c)[:, None]
    return U * inv[:, None] * ((2.5 * k2 + 7) * size + np.abs(x) * (kc * np.abs(x * dy).sum(1))[:, None])


# ---- isx_gap_l2 (NCHW) --------------------------------------------------------------------------------------------------------------------------------
GAP_THREADS = 256
GAP_MAX_PASSES = 16
GAP_BUDGET = 52 * 1024
GAP_BUDGET_MANY = 26 * 1024                       # launches of GAP_MANY images or more, where it also fits
GAP_MANY = 512


def _gap_cp(stride, budget):
    cp = GAP_THREADS
    while cp > 32 and cp * stride * 4 > budget:
        cp >>= 1
    return cp


def _gap_fits(cp, stride, C, budget):
    return cp * stride * 4 <= budget and (C + cp - 1) // cp <= GAP_MAX_PASSES


def gap_plan(B, C, HW, aligned=True):
    """The launcher's rules: ("fused", CP, vec) or ("fallback", None, None).  The PATH is a function of (C, HW); B only picks CP, the channels
    staged per pass, which no result bit depends on; vec (16-byte loads into the staging) likewise."""
    stride = HW | 1
    cp = _gap_cp(stride, GAP_BUDGET)
    if not _gap_fits(cp, stride, C, GAP_BUDGET):
        return ("fallback", None, None)
    if B >= GAP_MANY:
        cp_many = _gap_cp(stride, GAP_BUDGET_MANY)
        if _gap_fits(cp_many, stride, C, GAP_BUDGET_MANY):
            cp = cp_many
    return ("fused", cp, bool(aligned and (C * HW) % 4 == 0 and (cp * HW) % 4 == 0))


def pool_in_order(f):
    """(B, C, HW) -> (B, C): ((0 + v_0) + v_1) + ..., then / (float)HW."""
    f = np.asarray(f, F)
    s = np.zeros(f.shape[:2], F)
    for i in range(f.shape[2]):
        s = s + f[:, :, i]
    return s / F(f.shape[2])


def pool_lanes(f):
    """(B, C, HW) -> (B, C): gap_only_kernel -- lane l sums i = l, l + 64, ..., the butterfly, one division."""
    f = np.asarray(f, F)
    B, C, HW = f.shape
    return (wave_butterfly(strided_partials(f.reshape(B * C, HW), LANES)) / F(HW)).reshape(B, C)


def gap_ss(pooled):
    """Thread t of 256 squares channels t, t + 256, ... whatever CP was; block_sum<256>."""
    return block_sum(strided_partials(pooled * pooled, GAP_THREADS))


def gap_l2(f, eps=EPS, B_launch=None, y_aligned=True):
    """f: (B, C, H, W).  B_launch: the size of the launch these images are part of (default: their own number)."""
    f = np.asarray(f, F)
    B, C = f.shape[:2]
    f = f.reshape(B, C, -1)
    path = gap_plan(B if B_launch is None else B_launch, C, f.shape[2])[0]
    if path == "fused":
        p = pool_in_order(f)
        return finish_rows(p, gap_ss(p), eps, None, False)
    return l2norm_rows(pool_lanes(f), eps, None, y_aligned)                     # the row kernel in place on the pooled values


def pool64(f):
    f = np.asarray(f, np.float64)
    return f.reshape(f.shape[0], f.shape[1], -1).mean(2)


def pool_bound(f, in_order):
    f = np.asarray(f, np.float64)
    f = f.reshape(f.shape[0], f.shape[1], -1)
    HW = f.shape[2]
    k = HW if in_order else (HW + LANES - 1) // LANES + 6 + 1
    return k * U * np.abs(f).sum(2) / HW


# ---- isx_gap_l2_nhwc --------------------------------------------------------------------------------------------------------------------------------------
NHWC_THREADS = 512


def gap_nhwc_plan(C, aligned=True):
    """"qpt1" / "qpt2" / "qpt4" (float4 groups per thread) or "generic" (gap_only_nhwc_kernel, then the row kernel in place)."""
    if not (aligned and C % 4 == 0 and C // 4 <= 4 * NHWC_THREADS):
        return "generic"
    nq = C // 4
    return "qpt1" if nq <= NHWC_THREADS else "qpt2" if nq <= 2 * NHWC_THREADS else "qpt4"


def gap_nhwc_ss(pooled):
    """Thread t of 512 owns the float4 groups t, t + 512, ...: one float4 term each; block_sum<512>."""
    return block_sum(strided_partials(float4_terms(pooled), NHWC_THREADS))


def gap_l2_nhwc(f, eps=EPS, map_aligned=True, y_aligned=True):
    """f: (B, HW, C), the map as it lies in memory.  Both paths walk the positions in order.  The float4 kernel needs the map AND y on 16-byte
    boundaries; on the generic path the row kernel runs in place on y, so its choice follows y alone."""
    f = np.asarray(f, F)
    p = pool_in_order(np.transpose(f, (0, 2, 1)))
    if gap_nhwc_plan(f.shape[2], map_aligned and y_aligned) == "generic":
        return l2norm_rows(p, eps, None, y_aligned)
    return finish_rows(p, gap_nhwc_ss(p), eps, None, False)


# ---- isx_best_location_desc, both layouts -----------------------------------------------------------------------------------------------------------------
def best_location(cls):
    """cls (B, K, Hp, Wp) -> (B, 2) int64 (row, col): the largest class-max (-0 folded onto +0), ties to the smallest column, then the
    smallest row."""
    cls = np.asarray(cls, F)
    B, K, Hp, Wp = cls.shape
    m = cls.max(1)
    m = np.where(m == 0, F(0), m)
    loc = np.empty((B, 2), np.int64)
    for b in range(B):
        rows, cols = np.nonzero(m[b] == m[b].max())
        i = np.argmin(cols * Hp + rows)
        loc[b] = rows[i], cols[i]
    return loc


def best_location_desc(cls, eps=EPS):
    """(desc (B, K), loc (B, 2)); the same for both layouts: ss over k = t, t + 256, ..., block_sum<256>."""
    cls = np.asarray(cls, F)
    loc = best_location(cls)
    v = np.stack([cls[b, :, r, c] for b, (r, c) in enumerate(loc)])
    return finish_rows(v, block_sum(strided_partials(v * v, 256)), eps, None, False), loc


# ---- isx_region_gather_l2, both layouts -------------------------------------------------------------------------------------------------------------------
def gather_windows(fmap, kh, kw, flat_idx, Wp, order):
    """fmap (B, C, Hf, Wf), flat_idx (B, k) -> (rows (B * k, F) in "chw" or "hwc" order, valid (B * k,)).  Invalid: a negative index, or a
    window that leaves the map; its row is all +0."""
    fmap = np.asarray(fmap, F)
    B, C, Hf, Wf = fmap.shape
    k = flat_idx.shape[1]
    rows = np.zeros((B * k, C * kh * kw), F)
    valid = np.zeros(B * k, bool)
    for b in range(B):
        for i, fi in enumerate(np.asarray(flat_idx[b]).tolist()):
            r, c = (fi // Wp, fi % Wp) if fi >= 0 else (0, 0)
            if fi < 0 or r + kh > Hf or c + kw > Wf:
                continue
            w = fmap[b, :, r:r + kh, c:c + kw]
            rows[b * k + i] = (w if order == "chw" else np.transpose(w, (1, 2, 0))).reshape(-1)
            valid[b * k + i] = True
    return rows, valid


def one_by_one_partials(x, nt):
    """(B, 4 n) -> (B, nt): thread t owns the float4s j = t, t + nt, ... and adds their four squares to its accumulator one by one."""
    s = (x * x).reshape(x.shape[0], -1, 4)
    v = np.zeros((x.shape[0], nt), F)
    for j0 in range(0, s.shape[1], nt):
        w = min(nt, s.shape[1] - j0)
        for e in range(4):
            v[:, :w] = v[:, :w] + s[:, j0:j0 + w, e]
    return v


def gather_nhwc_ss(g):
    return block_sum(one_by_one_partials(g, 1024))


def region_gather_l2(fmap, kh, kw, flat_idx, Wp, shift=None, eps=EPS, order="chw"):
    """(B, k, F).  "chw": isx_region_gather_l2 (thread t takes j = t, t + 1024, ... of the (c, a, b) row); "hwc": isx_region_gather_l2_nhwc on the
    (a, b, c) row, `shift` in that order too.  Both add +0 where there is no Shift."""
    g, valid = gather_windows(fmap, kh, kw, flat_idx, Wp, order)
    ss = block_sum(strided_partials(g * g, 1024)) if order == "chw" else gather_nhwc_ss(g)
    out = finish_rows(g, ss, eps, shift, True)
    out[~valid] = 0
    return out.reshape(flat_idx.shape[0], flat_idx.shape[1], -1)


# ---- the shapes and the data both test files walk ------------------------------------------------------------------------------------------------------
L2_D_ALIGNED = (4, 252, 256, 260, 512, 516, 1024, 1028, 2044, 2048, 2052, 4100, 8196)      # 8196: every thread of the vector block kernel holds two float4s
L2_D_SCALAR = (1, 37, 1023, 1025, 2049)
L2_D_OFFSET = (256, 2048)                         # at a base offset of one float: the scalar kernel, other bits than the aligned call
L2_B = (1, 5, 9)                                  # 5, 9: a ragged last group of four rows in the wave kernel
GAP_NCHW = ((3, 24, 7, 7), (2, 300, 7, 7), (3, 30, 5, 3), (2, 2048, 8, 8), (2, 2048, 14, 14), (1, 8, 40, 40))
GAP_BATCH = ((512, 7, 7), (2048, 8, 8))           # (C, H, W): 3 images alone and as the first 3 of a launch of GAP_MANY
GAP_NHWC_C = (4, 2048, 2052, 4096, 4100, 8192, 8196, 30)
GAP_NHWC_HW = (1, 49, 50)
BEST_K = (1, 17, 256, 257, 464, 1000)
GATHER = ((4, 3, 3), (20, 3, 17), (64, 4, 4), (1028, 1, 1), (2048, 7, 7))       # (C, kh, kw): F = 36, 1020, 1024, 1028, 100352
BWD_D = (1, 17, 1024, 1025, 2048, 5000, 100352)
BWD_B = (1, 3)
ROW_KINDS = ("normal", "relu", "zero", "eps", "spike")


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays[0] if len(arrays) == 1 else arrays


def make_rows(B, D, rng):
    """Row i is of kind ROW_KINDS[i % 5]: N(0, 1); post-ReLU with a -0 planted in front; all zero; a sum of squares of about eps (1e-10); one
    element 1e4 times the rest."""
    x = rng.standard_normal((B, D)).astype(F)
    for i in range(B):
        kind = ROW_KINDS[i % 5]
        if kind == "relu":
            x[i] = np.maximum(x[i], 0)
            x[i, 0] = -0.0
        elif kind == "zero":
            x[i] = 0
        elif kind == "eps":
            x[i] *= F(1e-5 / np.sqrt(D))
        elif kind == "spike":
            x[i, D // 2] = F(1e4) * (1 + abs(x[i, D // 2]))
    return x


@functools.lru_cache(maxsize=None)
def row_case(B, D):
    """(x (B, D), shift (D,))"""
    rng = np.random.default_rng(100000 * B + D)
    return _frozen(make_rows(B, D, rng), (F(0.1) * rng.standard_normal(D)).astype(F))


@functools.lru_cache(maxsize=None)
def bwd_case(B, D):
    """(x, dy): the rows of row_case's kinds that a training step can meet (no all-zero row at eps = 1e-10: its gradient is dy / 1e-5, fine, and
    kept), dy of N(0, 1) / sqrt(D)."""
    rng = np.random.default_rng(200000 * B + D)
    return _frozen(make_rows(B, D, rng), (rng.standard_normal((B, D)) / np.sqrt(D)).astype(F))


@functools.lru_cache(maxsize=None)
def map_case(B, C, H, W):
    """(B, C, H, W): image 0 N(0, 1), the others post-ReLU; the last image's channel 0 is all zero; when B >= 3 image 2 is scaled so that its
    sum of squared means is about eps."""
    rng = np.random.default_rng(1000 * C + 10 * H + W + B)
    f = rng.standard_normal((B, C, H, W)).astype(F)
    f[1:] = np.maximum(f[1:], 0)
    f[-1, 0] = 0
    if B >= 3:
        f[2] *= F(1e-5 / np.sqrt(C) * 2.5)
    return _frozen(f)


@functools.lru_cache(maxsize=None)
def best_case(K, Hp, Wp):
    """(3, K, Hp, Wp) scores.  Image 1: the top class-max planted at (row 2, col 0) and (row 0, col 1) -- the tie goes to the smaller column,
    where a row-major index would take (0, 1).  Image 2: all scores <= 0, the top ones -0 at (0, 1) and +0 at (1, 1): row 0 wins, the zeros are one score (an
    order that put +0 above -0 would take (1, 1))."""
    assert Hp >= 3 and Wp >= 2
    rng = np.random.default_rng(31 * K + Hp)
    cls = rng.standard_normal((3, K, Hp, Wp)).astype(F)
    cls[1, 0, 2, 0] = cls[1, 0, 0, 1] = 10.0
    cls[2] = -np.abs(cls[2]) - F(0.5)
    cls[2, K - 1, 0, 1] = -0.0
    cls[2, 0, 1, 1] = 0.0
    return _frozen(cls)


@functools.lru_cache(maxsize=None)
def gather_case(C, kh, kw):
    """(fmap (2, C, kh + 1, kw + 2), flat_idx (2, 6), Wp = 3, shift (F,) in (c, a, b) order): Hp = 2, six locations; image 0 walks 0, the last,
    -1, the first index past the map, and two more; image 1 another order.  Image 1 is post-ReLU."""
    rng = np.random.default_rng(7 * C + kh)
    fmap = rng.standard_normal((2, C, kh + 1, kw + 2)).astype(F)
    fmap[1] = np.maximum(fmap[1], 0)
    idx = np.array([[0, 5, -1, 6, 2, 3], [4, -1, 1, 5, 60, 0]], np.int64)
    shift = (F(0.1) * rng.standard_normal(C * kh * kw)).astype(F)
    return _frozen(fmap, idx) + (3,) + (_frozen(shift),)


def shift_hwc(shift, C, kh, kw):
    return np.ascontiguousarray(np.asarray(shift).reshape(C, kh, kw).transpose(1, 2, 0)).reshape(-1)


def sqrt_sweep():
    """(x (65790,), float32): both signs x every exponent 0 .. 254 (denormals included, no infinity or NaN) x 129 mantissas (0, all ones, 127
    random ones)."""
    rng = np.random.default_rng(9)
    man = np.concatenate([[0, (1 << 23) - 1], rng.integers(1, (1 << 23) - 1, 127)]).astype(np.uint32)
    exp = np.arange(255, dtype=np.uint32)
    bits = (exp[:, None] << 23) | man[None, :]
    bits = np.concatenate([bits.reshape(-1), bits.reshape(-1) | np.uint32(1 << 31)])
    return bits.astype(np.uint32).view(F)
