"""CPU restatements for the evaluation-side kernels that tests/test_gpu_eval_guards.py launches on guarded buffers (csrc/rank.hip: DBA over
same-instance groups; csrc/region.hip: the class-max and the top-k locations of both layouts; csrc/classif.hip: the box-pool backward;
csrc/apshard.hip: average precision against a gallery sharded by rows), checked on their own in tests/test_eval_model.py.  Only numpy, the
oracle (the fma chain of its cosine_sim) and, for the sharded average precision, the project's own CPU restatement (utils/metrics.py).

dba_chain.  dba_group_kernel in fp32, one rounding per operation (libisx is built with -ffp-contract=off; hipcc rounds fp32 division and sqrtf
correctly by default, tests/_desc_model.py):
  scores       acc = fmaf(E[i][d], E[m][d], acc) from +0 over d = 0 .. D-1: the chain of the oracle's cosine_sim;
  ranking      canonical: score descending (-0 folded onto +0), item index ascending, the item itself excluded;
  weights      w_j = float32(float64(nn - j) / float64(nn + 1)), nn = the neighbours used;
  aggregation  agg = agg + E[best_j][d] * w_j for j = 0, 1, ...: a multiply, then an add;
  norm         ss: thread t of 256 adds agg[d]^2 over d = t, t + 256, ... from +0, the butterfly of each wave, the four wave sums in order
               (strided_partials, block_sum of tests/_desc_model.py); nrm = sqrtf(ss) + 1e-10f; out = agg / nrm;
  a singleton instance and k = 0 are copied unchanged.
The oracle's dba differs only in the norm (a float64 sum of squares): rtol 2e-6 is what tests/test_gpu_dropin.py allows between the two.

class_max.  The NaN rule of include/isx.h: a location with a NaN in any class has the canonical quiet NaN 0x7FC00000 as its maximum; every
other location the largest score, a zero as +0 (the ranking key folds -0 onto +0, and the emitted score is read back from the key)."""
import functools

import numpy as np

import _desc_model as dm
import oracle as O

F = np.float32
QNAN = np.uint32(0x7FC00000)
AP_MAXP = 2048


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays[0] if len(arrays) == 1 else arrays


def rank_keys(scores, idx):
    """Canonical ranking keys, larger = ranked earlier: (orderable score << 32) | ~index; -0 folded onto +0."""
    s = np.array(scores, dtype=F, copy=True)
    s[s == 0] = 0
    u = s.view(np.uint32)
    ob = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint64)
    return (ob << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(idx, dtype=np.uint64))


# ---- isx_dba_groups -------------------------------------------------------------------------------------------------------------------------------
def dba_groups_of(labels):
    """(order, grp_begin, grp_size, max_group) as the caller of isx_dba_groups builds them: the items sorted by (label, index); item i's
    instance is order[grp_begin[i] : grp_begin[i] + grp_size[i]]."""
    labels = np.asarray(labels)
    N = len(labels)
    order = np.lexsort((np.arange(N), labels)).astype(np.int32)
    begin, size = np.empty(N, np.int32), np.empty(N, np.int32)
    s = 0
    sl = labels[order]
    while s < N:
        e = s
        while e < N and sl[e] == sl[s]:
            e += 1
        begin[order[s:e]], size[order[s:e]] = s, e - s
        s = e
    return order, begin, size, int(size.max()) if N else 0


def dba_chain(emb, labels, k, eps_outside=True, denominator_plus=1, reverse_waves=False):
    """emb (N, D), labels (N,) -> (N, D).  The keyword arguments are the WRONG variants tests/test_eval_model.py tells the model apart from
    (no 1e-10 on the norm; nn instead of nn + 1 under the weights; the four wave sums added in reverse order)."""
    emb = np.ascontiguousarray(emb, F)
    N, D = emb.shape
    out = emb.copy()
    order, begin, size, _ = dba_groups_of(labels)
    done = np.zeros(N, bool)
    for i in range(N):
        if done[i]:
            continue
        g = order[begin[i]:begin[i] + size[i]].astype(np.int64)               # ascending item index
        done[g] = True
        n = len(g)
        nn = n - 1
        if 0 <= k < nn:
            nn = k
        if nn <= 0:
            continue
        E = emb[g]
        keys = rank_keys(O.cosine_sim(E, E), g[None, :].repeat(n, 0))
        keys[np.arange(n), np.arange(n)] = 0                                    # the item itself ranks last
        best = np.argsort(keys, axis=1)[:, ::-1][:, :nn]                         # keys are distinct: (score desc, index asc)
        w = np.array([F(np.float64(nn - j) / np.float64(nn + denominator_plus)) for j in range(nn)], F)
        agg = E.copy()
        for j in range(nn):
            agg = agg + E[best[:, j]] * w[j]
        part = dm.strided_partials(agg * agg, 256)
        if reverse_waves:
            wv = dm.wave_butterfly(part.reshape(n, 4, 64))
            ss = np.zeros(n, F)
            for q in (3, 2, 1, 0):
                ss = ss + wv[:, q]
        else:
            ss = dm.block_sum(part)
        nrm = dm._sqrt(ss) + F(1e-10) if eps_outside else dm._sqrt(ss)
        out[g] = dm._div(agg, nrm[:, None])
    return out


# ---- class-max, isx_region_topk, isx_best_location_desc (both layouts) --------------------------------------------------------------------------------
def class_max(cls, layout="nchw"):
    """cls (B, K, Hp, Wp) ["nchw"] or (B, Hp, Wp, K) ["nhwc"] -> (B, Hp, Wp) float32."""
    cls = np.asarray(cls, F)
    axis = {"nchw": 1, "nhwc": 3}[layout]
    nan = np.isnan(cls).any(axis)
    with np.errstate(all="ignore"):
        m = np.fmax.reduce(cls, axis=axis)                                       # the largest number; a NaN only where every class is one
    m = np.where(m == 0, F(0), m).astype(F)
    m.view(np.uint32)[nan] = QNAN
    return m


def region_topk(cls, k, layout="nchw"):
    """-> (flat_idx (B, k) int64, score (B, k) float32): the first min(k, Hp Wp) locations by (class-max descending, a NaN first, flat index
    ascending), then (-1, -inf)."""
    m = class_max(cls, layout)
    B = m.shape[0]
    m = m.reshape(B, -1)
    P = m.shape[1]
    idx = np.full((B, k), -1, np.int64)
    sc = np.full((B, k), -np.inf, F)
    for b in range(B):
        o = np.argsort(rank_keys(m[b], np.arange(P)))[::-1][:k]
        idx[b, :len(o)], sc[b, :len(o)] = o, m[b, o]
    return idx, sc


def oracle_region_topk(cls, k):
    """The oracle's per-image top-k of an NCHW batch in the kernels' output form: (B, k), padded with (-1, -inf)."""
    idx = np.full((cls.shape[0], k), -1, np.int64)
    sc = np.full((cls.shape[0], k), -np.inf, F)
    for b in range(cls.shape[0]):
        i, s = O.region_topk(cls[b], k)
        idx[b, :len(i)], sc[b, :len(i)] = i, s
    return idx, sc


def best_location(cls, layout="nchw"):
    """-> (B, 2) int64 (row, col): the largest class-max (a NaN above everything), ties to the smallest column, then the smallest row."""
    m = class_max(cls, layout)
    B, Hp, Wp = m.shape
    loc = np.empty((B, 2), np.int64)
    cols, rows = np.meshgrid(np.arange(Wp), np.arange(Hp))
    for b in range(B):
        i = int(np.argmax(rank_keys(m[b].reshape(-1), (cols * Hp + rows).reshape(-1))))
        loc[b] = i // Wp, i % Wp
    return loc


def to_nhwc(cls):
    return np.array(np.transpose(cls, (0, 2, 3, 1)), order="C")              # always a copy (a 1 x 1 map transposes to a view)


def nan_f32(negative=False, payload=0):
    return np.uint32((0xFFC00000 if negative else 0x7FC00000) | payload).view(F)


@functools.lru_cache(maxsize=None)
def topk_case(B, K, Hp, Wp, special):
    """(B, K, Hp, Wp) scores rounded to quarters (the index tie-break decides); `special`: the last image is one value everywhere, and image 0
    holds +-inf, +-0 and denormals at class 0 and at a later class (locations 0 .. min(P, 12) - 1, every other class of those far below)."""
    rng = np.random.default_rng(1000 * K + 10 * Hp + Wp + B)
    cls = (np.round(rng.standard_normal((B, K, Hp, Wp)) * 4) / 4).astype(F)
    if special:
        cls[B - 1] = F(0.25)
        vals = np.array([np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45], F)
        flat = cls[0].reshape(K, -1)
        for j in range(min(flat.shape[1], 12)):
            flat[:, j] = -np.inf if vals[j % 6] == -np.inf else F(-50)
            flat[0 if j < 6 else K - 1, j] = vals[j % 6]
    return _frozen(cls)


@functools.lru_cache(maxsize=None)
def nan_case(K, Hp, Wp):
    """(3, K, Hp, Wp), P = Hp Wp >= 12.  Image 0: a NaN at class 0 (location 7), at a middle class (location 2, negative, with a payload), at
    the last class (location 9), a location that is all NaN (4) and +inf at location 1: four NaN locations, ranked 2, 4, 7, 9 in front of the
    +inf.  Image 1: every location but the last has a NaN somewhere (more NaN locations than any k below P - 1).  Image 2: no NaN (the rule
    must not touch it), a -0 at class 0 over negative scores at location 3."""
    assert K >= 3 and Hp * Wp >= 12
    rng = np.random.default_rng(77 * K + Hp)
    cls = (np.round(rng.standard_normal((3, K, Hp, Wp)) * 4) / 4).astype(F)
    f = cls.reshape(3, K, -1)
    f[0, 0, 7] = nan_f32()
    f[0, K // 2, 2] = nan_f32(True, 0x1234)
    f[0, K - 1, 9] = nan_f32(True)
    f[0, :, 4] = nan_f32(False, 0x2BEEF)
    f[0, 1, 1] = np.inf
    P = Hp * Wp
    for p in range(P - 1):
        f[1, (p * 7) % K, p] = nan_f32(p % 2 == 1, p)
    f[2, :, 3] = F(-3)
    f[2, 0, 3] = -0.0
    return _frozen(cls)


# ---- isx_boxpool_s1_bwd_nhwc --------------------------------------------------------------------------------------------------------------------------
def boxpool_bwd_canonical(g, H, W, kh, kw, divide_inside=False):
    """g: (B, Ho, Wo, C) float32 numpy.  dx[b,i,j,c] = (sum over the windows covering (i, j): rows p ascending outside, columns q ascending
    inside, fp32 adds from +0) / (kh kw), one IEEE division.  divide_inside: the wrong variant that divides every term."""
    B, Ho, Wo, C = g.shape
    dx = np.empty((B, H, W, C), dtype=np.float32)
    div = np.float32(kh * kw)
    for i in range(H):
        for j in range(W):
            s = np.zeros((B, C), dtype=np.float32)
            for p in range(max(0, i - kh + 1), min(Ho - 1, i) + 1):
                for q in range(max(0, j - kw + 1), min(Wo - 1, j) + 1):
                    s = s + (g[:, p, q, :] / div if divide_inside else g[:, p, q, :])
            dx[:, i, j, :] = s if divide_inside else s / div
    return dx


# ---- average precision against a sharded gallery ---------------------------------------------------------------------------------------------------------
NONFINITE_BOUNDS = ((0, 1001), (1001, 1001), (1001, 1002), (1002, 3001))      # an empty shard, a shard of one row, bases off the 16-byte grid
BOUNDARY_BOUNDS = ((0, 2000), (2000, 4103), (4103, 6200))


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    """(sim (6, 3001), qlab, glab): 7 labels; 200 (r + 1) entries of row r are NaNs of both signs, infinities, zeros of both signs, denormals."""
    rng = np.random.default_rng(2049)
    M, N, L = 6, 3001, 7
    sim = rng.standard_normal((M, N)).astype(F)
    special = np.array([np.nan, np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45], F)
    special.view(np.uint32)[1] |= np.uint32(0x80000000)                          # -NaN: the sign bit forced
    for r in range(M):
        pos = rng.choice(N, size=200 * (r + 1), replace=False)
        sim[r, pos] = special[rng.integers(0, len(special), pos.size)]
    return _frozen(sim, (np.arange(M) % L).astype(np.int32), (np.arange(N) % L).astype(np.int32))


@functools.lru_cache(maxsize=None)
def boundary_case():
    """(sim (4, 6200) in eighths, qlab, glab): the queries have 2047, 2048, 2049 and 0 positives, placed by a random permutation."""
    rng = np.random.default_rng(6200)
    N = 6200
    sim = (np.round(rng.standard_normal((4, N)) * 8) / 8).astype(F)
    gl = np.full(N, 3, np.int32)
    perm = rng.permutation(N)
    gl[perm[:2047]] = 0
    gl[perm[2047:2047 + 2048]] = 1
    gl[perm[4095:4095 + 2049]] = 2
    return _frozen(sim, np.array([0, 1, 2, 4], np.int32), gl)


def shard_caps(counts):
    """The slots per shard the caller gathers: the largest count of any query on any shard, within [1, 2048]."""
    return max(1, min(int(max(int(c.max()) if c.size else 0 for c in counts)), AP_MAXP))


def sharded_ap_cpu(sim, qlab, glab, bounds, kth, steps=False):
    """The three steps of utils.metrics on CPU tensors, the two collectives done by hand.  -> ap (M,) float64; steps: also the per-shard
    (keys, count) list, keys_all, the per-shard histograms and n_lab, as numpy."""
    import torch
    from utils import metrics
    sim = np.asarray(sim, F)
    q = torch.from_numpy(np.asarray(qlab, np.int32).copy())
    shards = [(torch.from_numpy(sim[:, a:b].copy()), a, torch.from_numpy(np.asarray(glab[a:b], np.int32).copy())) for a, b in bounds]
    pos = [metrics.ap_shard_positives(s, a, q, g, AP_MAXP) for s, a, g in shards]
    cap = shard_caps([c.numpy() for _, c in pos])
    keys_all = torch.cat([k[:, :cap] for k, _ in pos], 1).contiguous()
    n_lab = sum(c for _, c in pos)
    hists = [metrics.ap_shard_hist(s, a, keys_all) for s, a, _ in shards]
    hist = sum(hists)
    ld = max(1, min(int(n_lab.max()), AP_MAXP))
    ap = metrics.ap_from_hist(hist[:, :ld].contiguous(), n_lab, kth).numpy()
    if steps:
        return ap, [(k.numpy().view(np.uint64), c.numpy()) for k, c in pos], keys_all.numpy().view(np.uint64), [h.numpy() for h in hists], n_lab.numpy()
    return ap


def oracle_ap(sim, qlab, glab, kth):
    return O.average_precision(O.rank_full(sim), qlab, glab, kth)
