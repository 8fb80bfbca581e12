"""CPU model of the softmax cross-entropy kernels of the classifier tail (csrc/classif.hip: isx_softmax_xent_fwd, isx_softmax_xent_bwd,
isx_softmax_xent_leaves), shared by tests/test_xent_model.py (the model against float64 F.cross_entropy, and against the wrong readings it has
to tell apart) and tests/test_gpu_xent_chains.py (the kernels against the model, bit for bit).

Every subtraction, add, division and multiply is a numpy float32 operation: one rounding each, never fused -- libisx is built with
-ffp-contract=off.  `exp` and `log` are ARGUMENTS, float32 array -> float32 array: the device's expf and logf are not correctly rounded, so the
GPU test hands in lookups into isx_debug_expf_logf (the kernels' own functions); on the CPU they are exp_ref / log_ref, float64 rounded once.
The lane sums and the butterfly are those of _triplet_model.py.

One wave per row z[0 .. C), label y:
  m    = fmaxf over the row: lane i folds its columns i, i + 64, ... into an accumulator that starts at -inf (so a lane without a column holds
         -inf), the 64 accumulators meet in a butterfly of fmaxf.  fmaxf ignores a NaN.  A maximum is the same whatever the order; which of
         -0 and +0 wins a tie is immaterial: m enters as z_j - m (exp(+-0) = 1) and as log s + m with log s >= +0 (a sum of +0 and -0 is +0).
  d_j  = fl(z_j - m);  e_j = exp(d_j)
  s    = lane i adds e_j for j = i, i + 64, ... in ascending order from +0; the 64 lane sums meet in the butterfly xor 32, 16, 8, 4, 2, 1
  loss = fl(fl(log s + m) - z_y); NaN for y outside [0, C)
  dz_j = fl(fl(fl(e_j / s) - [j == y]) * scale), scale ONE float32: fl(scale * scale_dev[0]) resp. fl(scale_a * scale_b)
  leaf = ((+0 + loss_0) + loss_1) + ... over the leaf's rows in row order

Non-finite logits.  A -inf column (a masked class) next to a finite one: d = -inf, e = +0 exactly, dz = fl(+0 * scale), a zero with the sign
of scale; its loss, when it carries the label, is +inf.  A +inf logit (d = inf - inf), a NaN logit (fmaxf skips it, its own d is NaN) or a row
of -inf only (m = -inf, d = -inf + inf) put a NaN into s: the loss and every dz of the row are NaN.  That is what F.cross_entropy gives in
float64.  A NaN is compared as a NaN, whatever its sign and payload.

Bound against float64 (u = 2^-24), used by test_xent_model.py, derived, not measured; exp and log taken as half an ulp.  e_j carries the
rounding of d_j -- an absolute error u |d_j| of the argument is a relative error u |d_j| of the exponential -- and of exp: u (|d_j| + 1)
relative.  On its way into s it passes ceil(C/64) - 1 roundings of its lane (the first add, to +0, is exact) and 6 of the butterfly.  To first
order, with T = ceil(C/64) + 6 (the exact first add counted as a rounding covers the second-order terms left out):
  ds   = |fl(s) - s| / s <= u * sum_j e_j (|d_j| + T) / s
  loss : ds (log'(s) = 1 / s) + u (|log s| + |log s + m| + |loss|): log, the two adds
  dz_j : |scale| * (p_j (u (|d_j| + 2) + ds) + 2 u |p_j - [j == y]|): e_j, the division, s; the subtraction and the multiply; `scale` is
         the float32 the kernel multiplies by, its own rounding is not part of the comparison
plus, below the normal range, half a unit 2^-150 per rounding that lands there: C 2^-150 in s (s >= 1: nothing relative to it),
2^-149 (1 + |scale|) in dz."""
import functools

import numpy as np

from _head_model import F
from _triplet_model import LANES, U, butterfly, lane_sums, sum_in_row_order

TINY = 2.0 ** -150


# ---- exp and log on the CPU ---------------------------------------------------------------------------------------------------------------------
def exp_ref(d):
    with np.errstate(all="ignore"):
        return np.exp(np.asarray(d, F).astype(np.float64)).astype(F)


def log_ref(s):
    with np.errstate(all="ignore"):
        return np.log(np.asarray(s, F).astype(np.float64)).astype(F)


def through_unique_bits(fn):
    """fn on the distinct bit patterns of its argument only, spread back: what the GPU test sends through the hook."""
    def lookup(x):
        x = np.ascontiguousarray(x, F)
        bits, inverse = np.unique(x.view(np.uint32).reshape(-1), return_inverse=True)
        return np.asarray(fn(bits.view(F)), F)[inverse.reshape(-1)].reshape(x.shape)
    return lookup


# ---- the row --------------------------------------------------------------------------------------------------------------------------------------
def row_max(z):
    """(B, C) -> (B,): fmaxf from -inf, NaN ignored."""
    z = np.asarray(z, F)
    v = np.full((z.shape[0], LANES), -np.inf, F)
    for j0 in range(0, z.shape[1], LANES):
        w = min(LANES, z.shape[1] - j0)
        v[:, :w] = np.fmax(v[:, :w], z[:, j0:j0 + w])
    return np.fmax.reduce(v, axis=1)


def row_terms(z, m, exp):
    """(B, C): e_j = exp(fl(z_j - m))."""
    with np.errstate(all="ignore"):
        return exp(np.asarray(z, F) - np.asarray(m, F)[:, None])


def row_sum(z, m, exp):
    with np.errstate(all="ignore"):
        return butterfly(lane_sums(row_terms(z, m, exp)))


def row_stats(z, exp):
    m = row_max(z)
    return m, row_sum(z, m, exp)


def in_range(labels, C):
    labels = np.asarray(labels, np.int64)
    return (labels >= 0) & (labels < C)


def row_loss(z, labels, m, s, log):
    z = np.asarray(z, F)
    ok = in_range(labels, z.shape[1])
    zy = z[np.arange(z.shape[0]), np.where(ok, labels, 0)]
    with np.errstate(all="ignore"):
        loss = (log(np.asarray(s, F)) + m) - zy
    return np.where(ok, loss, F(np.nan)).astype(F)


def onehot(labels, C):
    """(B, C) float32 1 at the label, +0 elsewhere; a label outside [0, C) marks no column."""
    return (np.asarray(labels, np.int64)[:, None] == np.arange(C)[None, :]).astype(F)


def row_grad(z, labels, m, s, scale, exp):
    """`scale` is the ONE float32 every element is multiplied by (scale_of)."""
    z = np.asarray(z, F)
    with np.errstate(all="ignore"):
        p = row_terms(z, m, exp) / np.asarray(s, F)[:, None]
        return ((p - onehot(labels, z.shape[1])) * F(scale)).astype(F)


def leaf_losses(rows):
    """(L, k) -> (L,): ((+0 + r_0) + r_1) + ..."""
    with np.errstate(all="ignore"):
        return sum_in_row_order(np.asarray(rows, F))


def scale_of(a, b=None):
    """fl(scale * scale_dev[0]) of the backward entry (b None: no scale_dev, the host scale as it is), fl(scale_a * scale_b) of the leaves."""
    return F(a) if b is None else F(a) * F(b)


def forward(z, labels, exp, log):
    m, s = row_stats(z, exp)
    return row_loss(z, labels, m, s, log)


def backward(z, labels, scale, exp):
    m, s = row_stats(z, exp)
    return row_grad(z, labels, m, s, scale, exp)


def leaves(z, labels, L, k, scale_a, scale_b, exp, log):
    """(loss_leaf (L,), dz like z, the row losses (L, k))."""
    m, s = row_stats(z, exp)
    rows = row_loss(z, labels, m, s, log).reshape(L, k)
    return leaf_losses(rows), row_grad(z, labels, m, s, scale_of(scale_a, scale_b), exp), rows


# ---- the bound against float64 (module docstring) ---------------------------------------------------------------------------------------------------
def bounds(z, labels, scale):
    """(loss bound (B,), dz bound (B, C)) in float64, for rows of finite or -inf logits with a finite maximum; `scale` as row_grad takes it."""
    z64 = np.asarray(z, F).astype(np.float64)
    B, C = z64.shape
    T = (C + LANES - 1) // LANES + 6
    m = z64.max(1)
    with np.errstate(all="ignore"):
        d = z64 - m[:, None]
        e = np.exp(d)
        absd = np.where(e > 0, np.abs(d), 0.0)                   # a -inf column: e = 0 exactly, no error whatever its d
        s = e.sum(1)
        ds = U * (e * (absd + T)).sum(1) / s + C * TINY
        ok = in_range(labels, C)
        zy = z64[np.arange(B), np.where(ok, labels, 0)]
        loss = np.log(s) + m - zy
        loss_b = ds + U * (np.abs(np.log(s)) + np.abs(np.log(s) + m) + np.abs(loss))
        p = e / s[:, None]
        sc = abs(float(F(scale)))
        dz_b = sc * (p * (U * (absd + 2) + ds[:, None]) + 2 * U * np.abs(p - onehot(labels, C))) + 2 * TINY * (1 + sc)
    return loss_b, dz_b


# ---- the cases both test files walk: the smallest shapes that reach each path --------------------------------------------------------------------------
C_CASES = (1, 2, 63, 64, 65, 127, 128, 129, 191, 311, 464, 1000, 4099)      # lanes with no column, one trip, a ragged last trip, many trips
B_CASES = (1, 3, 4, 5, 7)                                                    # whole and ragged groups of the 4 rows a workgroup holds
B_CASES_C = (65, 311)
LEAF_CASES = ((1, 1, 65), (1, 5, 311), (3, 4, 129), (2, 7, 1000), (1, 8192, 3), (2, 4097, 3))        # (leaves, k, C); k = 8192: the cap, 32 KB of LDS
SCALE_DEV = 1.0 / 3.0
# (scale, scale_dev or None) of the backward entry, (scale_a, scale_b) of the leaves (None: 1): 1; 1 / k; negative; 0; the device scalar
# alone; both, fl(fl(x / 5) / 3) != fl(x * fl(1 / 15)); a subnormal product 2^-140; a negative pair
SCALES = ((1.0, None), (1.0 / 7.0, None), (-0.75, None), (0.0, None), (1.0, SCALE_DEV), (0.2, SCALE_DEV), (2.0 ** -100, 2.0 ** -40), (-1.0 / 3.0, 0.3))
FINITE_KINDS = ("normal", "spread", "equal", "ties", "masked")
NAN_KINDS = ("plus_inf", "nan", "all_minus_inf")
WHERE = ("max", "min", "else")


def kind_row(kind, C, rng):
    if kind == "normal":
        return (rng.standard_normal(C) * 3).astype(F)
    if kind == "spread":                                         # +-80: most terms underflow, some into the denormals
        return np.linspace(-80, 80, C).astype(F)[rng.permutation(C)]
    if kind == "equal":
        return np.full(C, 1.25, F)
    z = (rng.standard_normal(C) * 3).astype(F)
    if kind == "ties":                                           # the maximum in 3 columns (C >= 3), wherever they fall
        others = rng.permutation(np.delete(np.arange(C), z.argmax()))[:2]
        z[others] = z.max()
    elif kind == "masked":                                       # -inf in every third column (C >= 2), column 0 finite
        z[np.arange(C) % 3 == 1] = -np.inf
    elif kind == "plus_inf":
        z[C // 2] = np.inf
    elif kind == "nan":
        z[C // 2] = np.nan
    elif kind == "all_minus_inf":
        z[:] = -np.inf
    else:
        raise ValueError(kind)
    return z


def label_at(z, where, rng):
    """The label at the (first) maximum, at the (first) minimum -- a -inf column of a masked row -- a NaN column skipped, or at a finite column
    that holds neither (column 0 where there is none)."""
    if np.isnan(z).all():                                        # C = 1, the NaN row
        return 0
    if where == "max":
        return int(np.nanargmax(z))
    if where == "min":
        return int(np.nanargmin(z))
    rest = np.flatnonzero(np.isfinite(z) & (z != np.nanmax(z)) & (z != np.nanmin(z)))
    return int(rest[int(rng.integers(len(rest)))]) if len(rest) else 0


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def kind_rows(C):
    """(z (25, C), labels (25,) int32, names): every kind -- the finite ones, then the three that come out NaN throughout -- with its label at
    the maximum, at the minimum and elsewhere, and a row of zeros of alternating sign.  25 rows: six whole groups of four and a ragged one."""
    rng = np.random.default_rng(9000 + C)
    z, y, names = [], [], []
    for kind in FINITE_KINDS + NAN_KINDS:
        for where in WHERE:
            row = kind_row(kind, C, rng)
            z.append(row); y.append(label_at(row, where, rng)); names.append("%s/%s" % (kind, where))
    z.append(np.where(np.arange(C) % 2 == 0, F(-0.0), F(0.0)).astype(F)); y.append(C // 2); names.append("zeros")
    return _frozen(np.stack(z).astype(F), np.array(y, np.int32)) + (tuple(names),)


N_FINITE = len(FINITE_KINDS) * len(WHERE)


@functools.lru_cache(maxsize=None)
def batch_case(B, C):
    """B rows of kind_rows(C), a different choice per B, the last one a row that comes out NaN (B >= 3): the last row of a ragged group."""
    z, y, names = kind_rows(C)
    pick = [(5 * B + 7 * i) % N_FINITE for i in range(B)]
    if B >= 3:
        pick[-1] = N_FINITE + (4 * B) % (len(NAN_KINDS) * len(WHERE))
    return _frozen(np.ascontiguousarray(z[pick]), np.ascontiguousarray(y[pick])) + (tuple(names[i] for i in pick),)


@functools.lru_cache(maxsize=None)
def leaf_case(L, k, C):
    """(z (L * k, C), labels): rows of finite loss (no label on a -inf column, no NaN row) so that the order of the leaf's sum shows: N(0, 3)
    rows, every fifth one masked, every seventh a +-80 spread."""
    rng = np.random.default_rng(31 * L + 7 * k + C)
    n = L * k
    z = (rng.standard_normal((n, C)) * 3).astype(F)
    for r in range(0, n, 7):
        z[r] = kind_row("spread", C, rng)
    if C >= 2:
        z[np.arange(n) % 5 == 2, 1] = -np.inf
    y = rng.integers(0, C, n)
    y = np.where(np.isinf(z[np.arange(n), y]), 0, y).astype(np.int32)
    return _frozen(z, y)


def finite_rows(z, labels):
    """Rows the float64 bound speaks about: no NaN, no +inf, a finite maximum."""
    z = np.asarray(z, F)
    with np.errstate(all="ignore"):
        return ~np.isnan(z).any(1) & ~(z == np.inf).any(1) & np.isfinite(np.fmax.reduce(z, axis=1))
