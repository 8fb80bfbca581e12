"""CPU model of the sums and decisions of the siamese training step's kernels (csrc/train.hip: negative mining, triplet loss forward, backward
and the all-leaves launch), shared by tests/test_triplet_model.py (the model against float64 and the oracle, and against the wrong variants it
has to tell apart) and tests/test_gpu_triplet_chains.py (the kernels against the model, bit for bit).

Every add and multiply is a numpy float32 operation: one rounding each, never fused -- libisx is built with -ffp-contract=off.  No torch, no matmul.

The row sum.  One wave per triplet row: lane l (0 .. 63) adds its terms j = l, l + 64, ... in ascending order into an accumulator that starts at
+0, the 64 accumulators meet in the xor butterfly 32, 16, 8, 4, 2, 1 (v = v[:o] + v[o:2o]: an add commutes, so every lane ends on the same
value).  The term is fl(fl(a*n) - fl(a*p)) (normalized) or fl(fl(dp*dp) - fl(dn*dn)) with dp = fl(a-p), dn = fl(a-n).

Forward bound of the row sum (u = 2^-24), used by test_triplet_model.py, derived, not measured.  A value that enters the sum passes through at
most ceil(D/64) - 1 roundings of its lane's accumulator (the first add, to +0, is exact) and 6 of the butterfly; each rounding multiplies what
it holds by (1 + e), |e| <= u.  A term itself carries r roundings: r = 3 normalized (two products, one difference), r = 5 otherwise (two
differences, two squares, one difference).  To first order |fl(s) - s| <= (ceil(D/64) + 6 + r) * u * sum_j |term_j|; the
second-order terms left out are covered by the exact first add counted as a rounding.  |term_j| is the size of the exact term, |a n - a p|
resp. |dp^2 - dn^2|.  As a theorem the r roundings INSIDE a term need the sizes before the difference, |a n| + |a p| resp. dp^2 + dn^2: the
products are rounded before they are subtracted, and where p and n both sit next to a the difference is smaller than either.  The test
asserts the smaller sum of the exact terms all the same: on unit rows whose positive and negative differ by far more than a rounding, the
lane sums and the butterfly dominate (about D / 64 + 6 roundings of sums of size |term|) and the case data stays inside it tenfold.

Mining.  No NaN scores anywhere: neither the oracle nor the reference defines an order for them (`sims.max(0)` of the reference propagates a
NaN, the kernel's key order sorts it by its bits)."""
import functools

import numpy as np

import oracle as O
from _head_model import F

U = 2.0 ** -24
LANES = 64


# ---- isx_triplet_loss_fwd ---------------------------------------------------------------------------------------------------------------------
def terms(a, p, n, normalized):
    """(B, D): the term of column j as the kernel forms it."""
    a, p, n = (np.asarray(x, F) for x in (a, p, n))
    if normalized:
        return a * n - a * p
    dp, dn = a - p, a - n
    return dp * dp - dn * dn


def term_sizes(a, p, n, normalized):
    """(B, D) float64: |term_j| of the forward bound (module docstring)."""
    a, p, n = (np.asarray(x, np.float64) for x in (a, p, n))
    return np.abs(a * n - a * p) if normalized else np.abs((a - p) ** 2 - (a - n) ** 2)


def lane_sums(t):
    """(B, D) terms -> (B, 64): lane l's sequential sum over j = l, l + 64, ... from +0; a lane past D keeps its +0."""
    B, D = t.shape
    v = np.zeros((B, LANES), F)
    for j0 in range(0, D, LANES):
        w = min(LANES, D - j0)
        v[:, :w] = v[:, :w] + t[:, j0:j0 + w]
    return v


def butterfly(v):
    """(B, 64) -> (B,): xor 32, 16, ..., 1."""
    o = LANES // 2
    while o:
        v = v[:, :o] + v[:, o:2 * o]
        o //= 2
    return v[:, 0]


def row_sum(a, p, n, normalized):
    return butterfly(lane_sums(terms(a, p, n, normalized)))


def clamp(l):
    """l > 0 ? l : +0"""
    return np.where(l > 0, l, F(0)).astype(F)


def loss_of_sum(s, margin, normalized):
    m = F(margin)
    return s + m if normalized else (s + F(2) * m) * F(0.5)


def loss_rows(a, p, n, margin, normalized):
    return clamp(loss_of_sum(row_sum(a, p, n, normalized), margin, normalized))


def row_bound(a, p, n, normalized):
    """(B,) float64: the forward bound of the row sum."""
    D = np.asarray(a).shape[1]
    r = 3 if normalized else 5
    return ((D + LANES - 1) // LANES + 6 + r) * U * term_sizes(a, p, n, normalized).sum(1)


def row_sum64(a, p, n, normalized):
    a, p, n = (np.asarray(x, np.float64) for x in (a, p, n))
    return ((a * n - a * p) if normalized else ((a - p) ** 2 - (a - n) ** 2)).sum(1)


# ---- isx_triplet_loss_bwd / _bwd_dev ------------------------------------------------------------------------------------------------------------
def scale_host(scale):
    return F(scale)


def scale_dev(scale, dev):
    return F(scale) * F(dev)


def scale_leaves(scale_a, scale_b):
    return F(scale_a) * F(scale_b)


def grads(a, p, n, rows, scale, normalized):
    """(ga, gp, gn); `scale` is the ONE float32 every element is multiplied by; +0 in every row with rows <= 0 (-0 and +0 included)."""
    a, p, n = (np.asarray(x, F) for x in (a, p, n))
    scale = F(scale)
    on = (np.asarray(rows, F) > 0)[:, None]
    ga = (n - p) * scale
    gp = (-a) * scale if normalized else (p - a) * scale
    gn = a * scale if normalized else (a - n) * scale
    z = F(0)
    return tuple(np.where(on, g, z).astype(F) for g in (ga, gp, gn))


# ---- isx_triplet_leaves -------------------------------------------------------------------------------------------------------------------------
def leaf_rows(d, L, k):
    """(a, p, n), each (L * k, D), leaf-major: leaf l holds its k anchor rows, then its k positive rows, then its k negative rows."""
    D = d.shape[1]
    v = np.asarray(d, F).reshape(L, 3, k, D)
    return tuple(np.ascontiguousarray(v[:, i]).reshape(L * k, D) for i in range(3))


def sum_in_row_order(rows):
    """(L, k) -> (L,): ((0 + r_0) + r_1) + ..."""
    t = np.zeros(rows.shape[0], F)
    for r in range(rows.shape[1]):
        t = t + rows[:, r]
    return t


def leaves(d, L, k, margin, normalized, scale_a, scale_b):
    """(loss_leaf (L,), dd like d, the row losses (L, k))."""
    D = d.shape[1]
    a, p, n = leaf_rows(d, L, k)
    rows = loss_rows(a, p, n, margin, normalized)
    g = grads(a, p, n, rows, scale_leaves(scale_a, scale_b), normalized)
    dd = np.stack([x.reshape(L, k, D) for x in g], 1).reshape(L * 3 * k, D)
    rows = rows.reshape(L, k)
    return sum_in_row_order(rows), np.ascontiguousarray(dd, F), rows


# ---- isx_mine_negatives / isx_mine_negatives_rows -------------------------------------------------------------------------------------------------
def fold_zero(s):
    """-0 onto +0: the order the kernel's keys give the scores."""
    return np.where(s == 0, F(0), s).astype(F)


def mine(sim_rows, N, row_base, labels, i1, i2, semi_hard):
    """sim_rows: rows [row_base, row_base + rows) of the N x N matrix; i1 / i2 absolute.  Per couple the candidate with the largest (score with -0
    folded onto +0, then smallest index); -1 when none is left."""
    sim_rows = np.asarray(sim_rows, F)
    assert sim_rows.shape[1] == N and not np.isnan(sim_rows).any()
    lab = np.asarray(labels)
    neg = np.empty(len(i1), np.int64)
    for c, (a, p) in enumerate(zip(np.asarray(i1).tolist(), np.asarray(i2).tolist())):
        assert 0 <= a - row_base < sim_rows.shape[0] and 0 <= p < N
        row = sim_rows[a - row_base]
        excl = lab == lab[a]
        if semi_hard:
            excl = excl | (row >= row[p])
        cand = ~excl
        if not cand.any():
            neg[c] = -1
            continue
        s = fold_zero(row)
        neg[c] = np.flatnonzero(cand & (s == s[cand].max()))[0]
    return neg


PAD_SCORE = 3.0                                   # above every cosine: wins any mining that reads it


def slab(sim, r0, r1):
    """A COPY of rows [r0, r1) with one block's worth of rows of PAD_SCORE on each side: (buffer (3 (r1 - r0), N), first row of the body).  A
    kernel that indexes a neighbouring row reads a score that wins against every label, and answers a wrong index rather than a right one by
    luck."""
    rows = r1 - r0
    buf = np.full((3 * rows, sim.shape[1]), PAD_SCORE, F)
    buf[rows:2 * rows] = sim[r0:r1]
    return buf, rows


def blocks(N):
    """The row blocks of the GPU test: a single first row; 7 rows at row_base 1 (the planted anchors); the last third, ending at N; everything."""
    return [(0, 1), (1, min(8, N)), (N - max(1, N // 3), N), (0, N)]


def partition(N, size):
    return [(r, min(r + size, N)) for r in range(0, N, size)]


# ---- the shapes both test files walk: the smallest that reach each path and boundary -----------------------------------------------------------------
ROW_CASES = ((1, 1), (3, 63), (4, 64), (5, 65), (7, 100), (37, 2048), (6, 2052))      # B = 5, 7: a partly empty last workgroup of 4 waves
BWD_PAST_CAP = ((513, 2048), (4097, 257))         # 4096 x 256 = 1 048 576 elements per sweep: 1 050 624, and D not dividing the sweep
LEAF_CASES = ((1, 1, 1), (2, 4, 64), (3, 5, 100), (2, 13, 2052), (8, 8, 2048), (1, 8192, 1))        # (L, k, D); k = 8192: the cap, 32 KB of LDS
MINE_N = (1, 5, 255, 256, 257, 1000)
MARGIN = 0.1
MARGIN_ZERO_CASE = (4, 64)                        # at margin 0 its row 1 holds n == p bit for bit
SCALE_DEV = 1.0 / 3.0                             # the device scalar of the _dev entry


def margins(B):
    """One row cannot be both: B = 1 is clamped at 0.1 and active at 2.5, and runs at both."""
    return (MARGIN, 2.5) if B == 1 else (MARGIN,)


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


def unit_rows(B, D, seed):
    """(a, p, n) unit rows, positives and negatives built around the anchor.  Even rows: the positive next to the anchor, the negative apart:
    clamped.  Odd rows: the negative next to the anchor, the positive at a distance: active.  Rows = 0 mod 4 (past row 0): BOTH next to the anchor,
    the loss a small difference of two sums near 1.  Row 2 (when B >= 4) is all zero in a, p and n."""
    rng = np.random.default_rng(seed)
    a = O.l2norm_rows(rng.standard_normal((B, D)).astype(F))
    near = O.l2norm_rows(a + F(0.05 / np.sqrt(D)) * rng.standard_normal((B, D)).astype(F))
    near2 = O.l2norm_rows(a + F(0.6 / np.sqrt(D)) * rng.standard_normal((B, D)).astype(F))
    far = O.l2norm_rows(a + F(1.5 / np.sqrt(D)) * rng.standard_normal((B, D)).astype(F))
    even = (np.arange(B) % 2 == 0)[:, None]
    p, n = np.where(even, near, far).astype(F), np.where(even, far, near).astype(F)
    both = np.arange(B) % 4 == 0
    both[0] = False
    n[both] = near2[both]
    if D == 1:                                    # unit rows are +-1: a sign pattern that holds clamped (n = -a) and active (n = a) rows
        p, n = a.copy(), np.where(even, -a, a).astype(F)
    if B >= 4:
        a[2] = p[2] = n[2] = 0
    return a, p, n


@functools.lru_cache(maxsize=None)
def row_case(B, D):
    return _frozen(*unit_rows(B, D, 1000 * B + D))


@functools.lru_cache(maxsize=None)
def margin_zero_case():
    """MARGIN_ZERO_CASE with n[1] = p[1]: at margin 0 every term of row 1 is x - x = +0, l == +0 exactly, the row gets zero gradient."""
    a, p, n = (x.copy() for x in row_case(*MARGIN_ZERO_CASE))
    n[1] = p[1]
    return _frozen(a, p, n)


@functools.lru_cache(maxsize=None)
def denormal_case():
    """(a, p, n, margin), B = D = 1, squared-distance form: dp^2 = 4 and dn^2 = 1 in units of 2^-149, margin = 1 unit.  (s + 2 m) * 0.5 = 2.5 -> 2
    units (ties to even); the halved sum plus the margin would be 1.5 -> 2, + 1 = 3 units.  Everywhere above the denormals the two are the same
    function: scaling by two commutes with rounding."""
    a = np.zeros((1, 1), F)
    p = np.full((1, 1), np.sqrt(2.0) * 2.0 ** -74, F)
    n = np.full((1, 1), 2.0 ** -74.5, F)
    return _frozen(a, p, n) + (float(np.ldexp(1.0, -149)),)


@functools.lru_cache(maxsize=None)
def leaf_case(L, k, D):
    """d (L * 3 k, D): unit_rows of L * k triplets laid out leaf by leaf."""
    a, p, n = unit_rows(L * k, D, 77 * L + 1000 * k + D)
    d = np.stack([x.reshape(L, k, D) for x in (a, p, n)], 1).reshape(L * 3 * k, D)
    return _frozen(np.ascontiguousarray(d, F))[0]


def leaf_scales(L, k, avg):
    """(scale_a, scale_b) as utils/train_general._Stepper._leaf_scales hands them over: the mean over the leaf's rows, the leaf's share."""
    return (1.0 / k) if avg else 1.0, k / float(L * k)


class MineCase(object):
    """sim (N, N), labels (N,) int32, labels_one (all one label), couples: name -> (i1, i2) int64."""


@functools.lru_cache(maxsize=None)
def mine_case(N):
    """Scores = oracle.cosine_sim of unit rows (the chains production feeds in), labels = arange(N) % L, L = 7 (2 at N = 5, 1 at N = 1).  Planted
    (N >= 255), each under its name in `couples`:
      tie            E[3] = E[72] (= E[515] at N = 1000) next to E[0], labels 3, 2 (4) against the anchor's 0: equal top scores in different waves
                     (and in a later sweep of the same thread); the couple is (0, 0): i1 == i2, sim_pos above the tie in the semi-hard phase
      equals_pos     E[100] = E[8] (labels 2 and 1), couple (1, 8): a candidate with s == sim_pos
      least_similar  E[9] = -E[2], couple (2, 9): the positive is the least similar item, semi-hard mining leaves nothing
      zeros          row 4 of the matrix is -0 at even columns and +0 at odd ones, the positive (4, 11) at 0.5: the first candidate, column 0, holds -0
      inf            row 5: +inf at column 20, -inf at column 30, couple (5, 12); row 6: sim_pos = +inf, couple (6, 13); row 7: sim_pos = -inf,
                     couple (7, 14) -- among finite candidates, so that the reference's fill value -2 for excluded items stays below a candidate
      same           couples (a, a)
      general        random couples in unsorted order
    labels_one: one label for all, -1 everywhere."""
    c = MineCase()
    rng = np.random.default_rng(5000 + N)
    L = 1 if N == 1 else 2 if N == 5 else 7
    E = O.l2norm_rows(rng.standard_normal((N, 16)).astype(F))
    planted = N >= 255
    if planted:
        tie = [3, 72] + ([515] if N > 515 else [])
        E[tie] = O.l2norm_rows((E[0] + F(0.05) * rng.standard_normal(16).astype(F))[None])[0]
        E[100] = E[8]
        E[9] = -E[2]
    sim = O.cosine_sim(E, E)
    lab = (np.arange(N) % L).astype(np.int32)
    couples = {}
    if planted:
        sim[4] = np.where(np.arange(N) % 2 == 0, F(-0.0), F(0.0))
        sim[4, 11] = 0.5
        sim[5, 20], sim[5, 30] = np.inf, -np.inf
        sim[6, 13] = np.inf
        sim[7, 14] = -np.inf
        couples.update(tie=([0], [0]), equals_pos=([1], [8]), least_similar=([2], [9]), zeros=([4], [11]), inf=([5, 6, 7], [12, 13, 14]))
    same = rng.permutation(N)[:min(N, 12)]
    couples["same"] = (same, same)
    i1 = rng.integers(0, N, 4 if N <= 5 else 96)
    i2 = np.array([rng.choice(np.flatnonzero(lab == lab[a])) for a in i1])
    couples["general"] = (i1, i2)
    c.N, c.L, c.E, c.sim, c.labels, c.labels_one = N, L, E, sim, lab, np.zeros(N, np.int32)
    c.couples = {k: (np.asarray(v[0], np.int64), np.asarray(v[1], np.int64)) for k, v in couples.items()}
    for arr in (c.E, c.sim, c.labels, c.labels_one) + tuple(x for v in c.couples.values() for x in v):
        arr.flags.writeable = False
    return c


def all_couples(case):
    """Every named couple, in name order: (i1, i2, names per couple)."""
    names = sorted(case.couples)
    i1 = np.concatenate([case.couples[k][0] for k in names])
    i2 = np.concatenate([case.couples[k][1] for k in names])
    return i1, i2, [k for k in names for _ in case.couples[k][0]]


@functools.lru_cache(maxsize=None)
def mine_expect(N, semi_hard):
    """name -> the whole-matrix model's answer for the couples of that name."""
    c = mine_case(N)
    return {k: mine(c.sim, N, 0, c.labels, v[0], v[1], semi_hard) for k, v in c.couples.items()}
