"""CPU model of the two training kernels of the region descriptor (csrc/region_sum_kernel.hpp: isx_region_sum_l2_nhwc and
isx_region_sum_l2_bwd_nhwc), shared by tests/test_region_train_model.py (the model against float64 autograd, and against the readings it has
to tell apart) and tests/test_gpu_region_train.py (the kernels against the model, bit for bit).  It imports nothing from the library; the
pieces (strided partials, butterfly, block_sum, the window gather) are those of tests/_desc_model.py.

Every add, multiply, divide and square root is a numpy float32 operation: one rounding each, never fused.

The orders (include/isx.h states them).
  window sums   ss_w = sum v^2 and c_w = sum v g walk the window as its (a, b, c) row in float4 groups: thread t of 1024 owns the groups t,
                t + 1024, ... and adds the four products of each to its accumulator one by one from +0; butterfly per wave; the 16 wave sums in
                order.  (gather_nhwc_ss of _desc_model for the squares; window_dot here for the products.)
  rows          t_w = v / sqrt(n2_w) + (shift or +0) on the (c, a, b) row; the valid windows' terms added in ascending w, starting from the
                first one.
  dfmap         per pixel: +0, then + (n2_w g - v c_w) * inv_w over the valid windows covering it in ascending w, then + add (the images that
                have a map: every add_every-th; the others add nothing).

Maps are passed in their LOGICAL (B, C, Hf, Wf) shape; the memory layout of the kernel's operands does not enter the arithmetic.

Bounds against float64 (u = 2^-24), derived, not measured.
  rows   every term obeys row_bound of _desc_model at depth ss_depth("gather_nhwc", F) (the order of the sum of squares is that kernel's), plus
         one rounding for the Shift's add; the k - 1 adds of the window sum each round a partial sum no larger than sum_w |t_w|:
         |rows - rows64| <= sum_w row_bound_w + (k - 1) u sum_w |t64_w|.                                                        rows_bound()
  dfmap  a window's term is isx_l2norm_rows_bwd's formula: bwd_bound of _desc_model with kc = 1 + 4 ceil(F / 4096) + 6 + 16 roundings on
         the way to c_w and k2 = ss_depth + 1 to n2; a pixel covered by m windows adds m terms (+ add): (m + 1) u (sum_w |dv64_w| + |add|)
         on top of the terms' own bounds.                                                                                        dfmap_bound()"""
import numpy as np

from _desc_model import EPS, F, U, _div, _sqrt, block_sum, gather_nhwc_ss, gather_windows, row_bound, ss_depth

NT = 1024


def one_by_one(p, nt=NT):
    """(B, 4 n) products -> (B, nt): thread t owns the float4 groups t, t + nt, ... and adds their four products one by one, from +0."""
    q = np.asarray(p, F).reshape(p.shape[0], -1, 4)
    v = np.zeros((p.shape[0], nt), F)
    for j0 in range(0, q.shape[1], nt):
        w = min(nt, q.shape[1] - j0)
        for e in range(4):
            v[:, :w] = v[:, :w] + q[:, j0:j0 + w, e]
    return v


def window_dot(v_hwc, g_hwc):
    """c_w of every window row: (W, F) x (W, F) -> (W,)."""
    return block_sum(one_by_one(np.asarray(v_hwc, F) * np.asarray(g_hwc, F)))


def _positions(flat_idx, Wp):
    return [[(fi // Wp, fi % Wp) for fi in row] for row in np.asarray(flat_idx).tolist()]


def region_sum_l2(fmap, kh, kw, flat_idx, Wp, shift=None, eps=EPS, order=None):
    """fmap (B, C, Hf, Wf), flat_idx (B, k) -> (rows (B, F) in (c, a, b) order, n2 (B, k); a skipped window's n2 is +0).
    order: the sequence in which the windows are added (default ascending: the kernel's)."""
    B, k = flat_idx.shape
    v_chw, valid = gather_windows(fmap, kh, kw, flat_idx, Wp, "chw")
    v_hwc, _ = gather_windows(fmap, kh, kw, flat_idx, Wp, "hwc")
    n2 = gather_nhwc_ss(v_hwc) + F(eps)
    n2[~valid] = 0
    with np.errstate(all="ignore"):
        t = _div(v_chw, _sqrt(n2)[:, None]) + (np.asarray(shift, F) if shift is not None else F(0))
    rows = np.zeros((B, v_chw.shape[1]), F)
    for b in range(B):
        acc = None
        for w in (range(k) if order is None else order):
            if valid[b * k + w]:
                acc = t[b * k + w] if acc is None else acc + t[b * k + w]
        if acc is not None:
            rows[b] = acc
    return rows, n2.reshape(B, k)


def region_sum_l2_bwd(fmap, g, n2, kh, kw, flat_idx, Wp, add=None, order=None, add_first=False, add_every=1):
    """g (B, F), n2 (B, k) as the forward wrote it, add (B / add_every, C, Hf, Wf) -- the map of image b / add_every for the images b with
    b % add_every == 0, the others add nothing -- or None -> (dfmap (B, C, Hf, Wf), cw (B, k)).
    order / add_first: the readings the tests must tell apart (windows added in another order; the class term in front instead of last)."""
    fmap, g = np.asarray(fmap, F), np.asarray(g, F)
    B, C, Hf, Wf = fmap.shape
    k = flat_idx.shape[1]
    v_chw, valid = gather_windows(fmap, kh, kw, flat_idx, Wp, "chw")
    v_hwc, _ = gather_windows(fmap, kh, kw, flat_idx, Wp, "hwc")
    g_hwc = np.ascontiguousarray(g.reshape(B, C, kh, kw).transpose(0, 2, 3, 1)).reshape(B, -1)
    cw = window_dot(v_hwc, np.repeat(g_hwc, k, 0))
    cw[~valid] = 0
    n2f = np.asarray(n2, F).reshape(-1)
    pos = _positions(flat_idx, Wp)
    out = np.zeros(fmap.shape, F)
    has = np.arange(B) % add_every == 0
    if add is not None and add_first:
        out[has] = out[has] + np.asarray(add, F)
    for b in range(B):
        for w in (range(k) if order is None else order):
            i = b * k + w
            if not valid[i]:
                continue
            inv = _div(F(1), n2f[i] * _sqrt(n2f[i]))
            dv = ((n2f[i] * g[b] - v_chw[i] * cw[i]) * inv).reshape(C, kh, kw)
            r, c = pos[b][w]
            out[b, :, r:r + kh, c:c + kw] = out[b, :, r:r + kh, c:c + kw] + dv
    if add is not None and not add_first:
        out[has] = out[has] + np.asarray(add, F)
    return out, cw.reshape(B, k)


# ---- float64 -------------------------------------------------------------------------------------------------------------------------------------
def _terms64(fmap, kh, kw, flat_idx, Wp, shift, eps):
    v, valid = gather_windows(fmap, kh, kw, flat_idx, Wp, "chw")
    v = v.astype(np.float64)
    n2 = (v * v).sum(1) + float(F(eps))
    t = v / np.sqrt(n2)[:, None]
    if shift is not None:
        t = t + np.asarray(shift, np.float64)
    t[~valid] = 0
    return v, valid, n2, t


def region_sum_l2_64(fmap, kh, kw, flat_idx, Wp, shift=None, eps=EPS):
    B, k = flat_idx.shape
    return _terms64(fmap, kh, kw, flat_idx, Wp, shift, eps)[3].reshape(B, k, -1).sum(1)


def rows_bound(fmap, kh, kw, flat_idx, Wp, shift=None, eps=EPS):
    B, k = flat_idx.shape
    v, valid, n2, t = _terms64(fmap, kh, kw, flat_idx, Wp, shift, eps)
    y = v / np.sqrt(n2)[:, None]
    y[~valid] = 0
    per = row_bound(y, ss_depth("gather_nhwc", v.shape[1]), t)
    return per.reshape(B, k, -1).sum(1) + (k - 1) * U * np.abs(t).reshape(B, k, -1).sum(1)


def _dv64(fmap, g, kh, kw, flat_idx, Wp, eps):
    B, k = flat_idx.shape
    v, valid, n2, _ = _terms64(fmap, kh, kw, flat_idx, Wp, None, eps)
    gg = np.repeat(np.asarray(g, np.float64), k, 0)
    c = (v * gg).sum(1)
    inv = 1.0 / (n2 * np.sqrt(n2))
    dv = (n2[:, None] * gg - v * c[:, None]) * inv[:, None]
    Fdim = v.shape[1]
    k2 = ss_depth("gather_nhwc", Fdim) + 1
    kc = 1 + 4 * ((Fdim // 4 + NT - 1) // NT) + 6 + 16
    size = n2[:, None] * np.abs(gg) + np.abs(v) * np.abs(c)[:, None]
    bound = U * inv[:, None] * ((2.5 * k2 + 7) * size + np.abs(v) * (kc * np.abs(v * gg).sum(1))[:, None])
    dv[~valid] = 0
    bound[~valid] = 0
    return dv, bound, valid


def _scatter64(shape, terms, kh, kw, flat_idx, Wp, valid):
    B, C = shape[:2]
    k = flat_idx.shape[1]
    out = np.zeros(shape, np.float64)
    pos = _positions(flat_idx, Wp)
    for b in range(B):
        for w in range(k):
            if valid[b * k + w]:
                r, c = pos[b][w]
                out[b, :, r:r + kh, c:c + kw] += terms[b * k + w].reshape(C, kh, kw)
    return out


def region_sum_l2_bwd64(fmap, g, kh, kw, flat_idx, Wp, add=None, eps=EPS):
    dv, _, valid = _dv64(fmap, g, kh, kw, flat_idx, Wp, eps)
    out = _scatter64(np.shape(fmap), dv, kh, kw, flat_idx, Wp, valid)
    return out if add is None else out + np.asarray(add, np.float64)


def dfmap_bound(fmap, g, kh, kw, flat_idx, Wp, add=None, eps=EPS):
    dv, bound, valid = _dv64(fmap, g, kh, kw, flat_idx, Wp, eps)
    shape = np.shape(fmap)
    own = _scatter64(shape, bound, kh, kw, flat_idx, Wp, valid)
    mag = _scatter64(shape, np.abs(dv), kh, kw, flat_idx, Wp, valid)
    m = _scatter64(shape, np.ones_like(dv), kh, kw, flat_idx, Wp, valid)
    if add is not None:
        mag = mag + np.abs(np.asarray(add, np.float64))
    return own + (m + 1) * U * mag


# ---- the cases both test files walk ------------------------------------------------------------------------------------------------------------------
#        (B, Hf, Wf, C, kh, kw, k)
CASES = ((2, 5, 6, 8, 3, 2, 4), (1, 9, 9, 64, 7, 7, 6), (3, 14, 14, 260, 7, 7, 6), (1, 14, 14, 2048, 7, 7, 6), (2, 7, 7, 64, 7, 7, 1),
         (2, 6, 6, 4, 1, 1, 5))
SKIP_CASE = CASES[0]                               # its image 1 carries a -1 entry


def make_case(case, seed=0):
    """(fmap (B, C, Hf, Wf) post-ReLU with image 0 signed, flat_idx (B, k) NOT in position order -- overlapping windows where the map has room
    for k distinct ones, some pixels uncovered --, Wp, shift (F,), g (B, F), add like fmap).  SKIP_CASE: image 1's second entry is -1."""
    B, Hf, Wf, C, kh, kw, k = case
    rng = np.random.default_rng(1000003 * seed + 7919 * C + 131 * Hf + 17 * k + B)
    fmap = rng.standard_normal((B, C, Hf, Wf)).astype(F)
    fmap[1:] = np.maximum(fmap[1:], 0)
    Hp, Wp = Hf - kh + 1, Wf - kw + 1
    P = Hp * Wp
    idx = np.empty((B, k), np.int64)
    for b in range(B):
        if P >= k + 1:                                # distinct locations, one corner left out so that some pixels stay uncovered
            idx[b] = rng.permutation(P - 1)[:k]
        else:
            idx[b] = rng.integers(0, P, k)
        if k > 2 and np.all(np.diff(idx[b]) > 0):     # never in position order
            idx[b, :2] = idx[b, 1::-1]
    if case == SKIP_CASE:
        idx[1, 1] = -1
    Fdim = C * kh * kw
    shift = (F(0.1) * rng.standard_normal(Fdim)).astype(F)
    g = (rng.standard_normal((B, Fdim)) / np.sqrt(Fdim)).astype(F)
    add = (F(1e-3) * rng.standard_normal(fmap.shape)).astype(F)
    for a in (fmap, idx, shift, g, add):
        a.flags.writeable = False
    return fmap, idx, Wp, shift, g, add
