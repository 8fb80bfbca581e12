"""CPU model of the canonical sums of the trunk suffix's backward kernels (csrc/backward.hip, the non-FOLD path of csrc/wgrad_kernel.hpp, the
kEpiMaskedGrad epilogue of csrc/gemm.hip, the GRAD path of csrc/conv.hip), shared by tests/test_suffix_model.py (the model against float64, and
against the wrong orders it has to tell apart) and tests/test_gpu_suffix_chains.py (the kernels against the model, bit for bit).

Every dot product is _head_model.chains (oracle.cosine_sim): a k-ordered fp32 fmaf chain from +0, the chain the fp32 MFMA computes.  Every other
add and multiply is a numpy float32 operation: one rounding each, never fused -- libisx is built with -ffp-contract=off.  No torch, no matmul.
The orders are read off the kernels; the building blocks (split_ranges, src_rows, wgrad_from, fold_sum, fold_dot, ...) are public so that the
wrong variants of tests/test_suffix_model.py are the same code with one piece exchanged."""
import collections
import functools

import numpy as np

from _head_model import F, add_in_order, chains, inputs

BK = 32                                           # pixels per k-tile of wgrad_gemm_kernel
FOLD_ROW = 9 * (512 + 1)                          # kFoldRow of bn_fold_backward_kernel: floats of one staged row

# B images of H x W input pixels, taps = 1 (1x1, no padding) or 9 (3x3, padding 1), stride 1 or 2
Geom = collections.namedtuple("Geom", "B H W taps stride")


def out_hw(g):
    return (g.H - 1) // g.stride + 1, (g.W - 1) // g.stride + 1


def tap_offsets(taps):
    """(dh, dw) of tap 0 .. taps-1: tap = kh * 3 + kw, dh = kh - 1, dw = kw - 1."""
    return [(0, 0)] if taps == 1 else [(t // 3 - 1, t % 3 - 1) for t in range(9)]


def src_bhw(g, dh, dw):
    """(b, h, w) of the input pixel that output pixel p = (b, ho, wo) meets under tap (dh, dw): (ho * stride + dh, wo * stride + dw)."""
    Ho, Wo = out_hw(g)
    p = np.arange(g.B * Ho * Wo, dtype=np.int64)
    b, rem = p // (Ho * Wo), p % (Ho * Wo)
    return b, rem // Wo * g.stride + dh, rem % Wo * g.stride + dw


def src_rows(g, dh, dw):
    """Row of x (B * H * W rows) per output pixel, -1 outside the map."""
    b, h, w = src_bhw(g, dh, dw)
    return np.where((h >= 0) & (h < g.H) & (w >= 0) & (w < g.W), (b * g.H + h) * g.W + w, -1)


def gather_rows(x, src):
    """x[src] with a row of +0 for src == -1: the term becomes fma(dz, 0, acc)."""
    out = np.zeros((len(src), x.shape[1]), F)
    ok = src >= 0
    out[ok] = x[src[ok]]
    return out


# ---- isx_conv_wgrad_nhwc ---------------------------------------------------------------------------------------------------------------------
def split_ranges(K, S):
    """(kt_per, [(lo, hi) of split 0 .. S-1]) over the K pixels of one leaf: nk = ceil(K / 32) k-tiles, kt_per = ceil(nk / S) per split; lo == hi:
    an empty split."""
    nk = (K + BK - 1) // BK
    kt_per = (nk + S - 1) // S
    return kt_per, [(min(K, BK * s * kt_per), min(K, BK * (s + 1) * kt_per)) for s in range(S)]


# ---- the tile shape of isx_conv3x3_dgrad_nhwc ---------------------------------------------------------------------------------------------
# A restatement of pick_tile_cfg (csrc/gemm.hip) as host arithmetic.  The library does not export that function and the gradient entry has no tile
# hook, so NOTHING can check this restatement against the library: it is the source read into Python, in IEEE doubles as the C++ is (the
# efficiencies are floats there and widened to double in the division, as float(np.float32(.)) is here).
TILE_CFGS = ((2, 2, 4), (1, 2, 4), (2, 1, 4), (1, 1, 6))              # (tm, tn, resident workgroups per CU) of 128x128, 64x128, 128x64, 64x64
TILE_TAIL = (0.22, 0.25, 0.25, 0.15)
EFF_3X3 = tuple(float(np.float32(e)) for e in (0.90, 0.0, 0.865, 0.87))    # kEff3x3 of csrc/conv.hip
MASK_3X3 = 0xD                                                        # the convolutions have no 64x128 instance


def tile_times(M, N, eff=EFF_3X3, mask=MASK_3X3, wg_per_cu_128=4):
    """(4, ...) estimated times of the four tile shapes for M rows (an int or an int64 array) and N columns, split = 0; inf outside `mask`."""
    M = np.asarray(M, dtype=np.int64)
    out = np.full((4,) + M.shape, np.inf)
    for c, (tm, tn, wg) in enumerate(TILE_CFGS):
        if not (mask >> c) & 1:
            continue
        if c == 0:
            wg = wg_per_cu_128
        tiles = ((M + 64 * tm - 1) // (64 * tm)).astype(np.float64) * float((N + 64 * tn - 1) // (64 * tn))
        x = tiles / (256.0 * wg)
        t0 = TILE_TAIL[c]
        with np.errstate(divide="ignore", invalid="ignore"):
            rounds = x + np.where(x <= 0.7, t0, t0 * (0.7 / x) * (0.7 / x))
        per_cu = np.floor((tiles + 255.0) / 256.0) / wg
        rounds = np.where(rounds > per_cu, rounds, per_cu)
        out[c] = rounds * wg * (tm * tn) / eff[c]
    return out


def pick_tile_cfg(M, N, eff=EFF_3X3, mask=MASK_3X3, wg_per_cu_128=4):
    """Index into TILE_CFGS of the shape with the smallest estimated time; the first wins a tie (the C++ compares with <)."""
    return np.argmin(tile_times(M, N, eff, mask, wg_per_cu_128), axis=0)


def colsum(rows):
    """s = 0; s += row, in row order."""
    s = np.zeros(rows.shape[1], F)
    for r in rows:
        s = s + r
    return s


def wgrad_from(dz, x, srcs, leaves, S, pixels):
    """dw (len(leaves), S, Cout, taps, Cin) and db (len(leaves), S, Cout).  srcs: per tap the source row of every output pixel of the launch;
    pixels(l, s): the output pixels (rows of dz) of split s of leaf l in the order of the chain -- an empty list writes zeros."""
    Cout, Cin = dz.shape[1], x.shape[1]
    dw, db = np.zeros((len(leaves), S, Cout, len(srcs), Cin), F), np.zeros((len(leaves), S, Cout), F)
    for i, l in enumerate(leaves):
        for s in range(S):
            p = np.asarray(pixels(l, s), dtype=np.int64)
            if not len(p):
                continue
            a = np.ascontiguousarray(dz[p].T)
            for t, src in enumerate(srcs):
                dw[i, s, :, t, :] = chains(a, np.ascontiguousarray(gather_rows(x, src[p]).T))
            db[i, s] = colsum(dz[p])
    return dw, db


def wgrad_partials(dz, x, geom, leaves, S, which=None):
    """isx_conv_wgrad_nhwc.  dz: (B * Ho * Wo, Cout), x: (B * H * W, Cin); the B images are `leaves` consecutive groups, K = the output pixels of
    one.  dw[l][s][co][tap][ci] = the chain over the pixels p of split s of leaf l, ascending, of dz[p][co] * x[src(p, tap)][ci]; db[l][s][co]
    = s = 0; s += dz[p][co] over the same pixels.  which: the leaves to compute (default all), in that order."""
    Ho, Wo = out_hw(geom)
    assert geom.B % leaves == 0
    K = geom.B // leaves * Ho * Wo
    ranges = split_ranges(K, S)[1]
    srcs = [src_rows(geom, dh, dw) for dh, dw in tap_offsets(geom.taps)]
    if geom.taps == 1 and geom.stride == 1:
        assert np.array_equal(srcs[0], np.arange(geom.B * Ho * Wo))        # the kernel's `ident` shortcut
    return wgrad_from(dz, x, srcs, range(leaves) if which is None else which, S, lambda l, s: np.arange(l * K + ranges[s][0], l * K + ranges[s][1]))


# ---- isx_bn_fold_backward ------------------------------------------------------------------------------------------------------------------
def fold_lds_path(taps, Cin):
    return taps > 1 and taps * (Cin + 1) <= FOLD_ROW


def fold_sum(parts):
    """((p_0 + p_1) + p_2) + ... over the leading (split) axis."""
    return add_in_order(list(parts))


def block_dot(prod):
    """(..., K) products -> (...): block_sum<256> of the per-thread sums.  Thread t adds prod[t], prod[t + 256], ... from +0 (a thread past the
    end adds nothing: + 0 changes no bits here); each wave reduces with the xor butterfly 32, 16, 8, 4, 2, 1; the block sum is
    (((0 + wave0) + wave1) + wave2) + wave3."""
    K = prod.shape[-1]
    n = (K + 255) // 256
    p = np.zeros(prod.shape[:-1] + (n * 256,), F)
    p[..., :K] = prod
    p = p.reshape(prod.shape[:-1] + (n, 256))
    v = np.zeros(prod.shape[:-1] + (256,), F)
    for j in range(n):
        v = v + p[..., j, :]
    v = v.reshape(prod.shape[:-1] + (4, 64))
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    t = np.zeros(prod.shape[:-1], F)
    for w in range(4):
        t = t + v[..., w, 0]
    return t


def fold_dot(d, w, lds):
    """d: (..., Cout, taps, Cin) summed partials, w: (Cout, Cin, taps).  The products d_i * w_i (rounded) of one output channel go through
    block_dot with i over the parameter layout (ci, tap) on the LDS path and over the partial layout (tap, ci) on the direct path."""
    if lds:
        prod = np.swapaxes(d, -1, -2) * w
    else:
        prod = d * np.swapaxes(w, -1, -2)
    return block_dot(np.ascontiguousarray(prod).reshape(prod.shape[:-2] + (-1,)))


def fold_ggamma(dot, mean, dbs, istd):
    return (dot - mean * dbs) * istd


def fold_backward(dwp, db, w, scale, mean, istd, taps, prior=None):
    """dwp: (leaves, S, Cout, taps, Cin), db: (leaves, S, Cout), w: (Cout, Cin, taps) -> gw (leaves, Cout, Cin, taps), ggamma and gbeta
    (leaves, Cout); prior: the three they are added to (accumulate = 1)."""
    assert dwp.shape[3] == taps and w.shape[1:] == (dwp.shape[4], taps)
    d = fold_sum(np.moveaxis(dwp, 1, 0))
    dbs = fold_sum(np.moveaxis(db, 1, 0))
    gw = np.ascontiguousarray(np.swapaxes(d * scale[:, None, None], -1, -2))
    gg = fold_ggamma(fold_dot(d, w, fold_lds_path(taps, w.shape[1])), mean, dbs, istd)
    gb = dbs
    if prior is not None:
        gw, gg, gb = prior[0] + gw, prior[1] + gg, prior[2] + gb
    return gw, gg, gb


# ---- the input gradients ---------------------------------------------------------------------------------------------------------------------
def masked(v, mask):
    return v if mask is None else np.where(mask > 0, v, F(0))


def dgrad1x1(dz, wt, add=None, mask=None):
    """isx_conv1x1_dgrad_nhwc.  dz: (M, Cout), wt: (Cin, Cout): one chain over all of Cout, then + add, then the mask."""
    v = chains(dz, wt)
    if add is not None:
        v = v + add
    return masked(v, mask)


def dgrad3x3_rows(dz):
    """(B, H, W, Cout) -> (B * H * W, 9 * Cout): the zero-padded 3x3 neighbourhood of every pixel in (kh, kw, co) order."""
    B, H, W, C = dz.shape
    pad = np.zeros((B, H + 2, W + 2, C), F)
    pad[:, 1:H + 1, 1:W + 1] = dz
    return np.ascontiguousarray(np.concatenate([pad[:, kh:kh + H, kw:kw + W] for kh in range(3) for kw in range(3)], -1).reshape(B * H * W, 9 * C))


def dgrad3x3(dz, wt, mask=None):
    """isx_conv3x3_dgrad_nhwc.  dz: (B, H, W, Cout), wt: (Cin, 3, 3, Cout), mask: (B, H, W, Cin): one chain of 9 * Cout terms per output."""
    v = chains(dgrad3x3_rows(dz), wt.reshape(wt.shape[0], -1)).reshape(dz.shape[:3] + (wt.shape[0],))
    return masked(v, mask)


def col2im_s2(dcol, B, H, W, Cin, mask=None, order=None):
    """isx_conv3x3_s2_col2im_nhwc.  dcol: (B * Ho * Wo, 9, Cin); input pixel (h, w) adds, from +0, the taps (kh, kw) with (h + 1 - kh) and
    (w + 1 - kw) even and inside the output grid, in (kh, kw) order (order: another sequence of the nine (kh, kw))."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    d = dcol.reshape(B, Ho, Wo, 9, Cin)
    acc = np.zeros((B, H, W, Cin), F)
    h, w = np.arange(H), np.arange(W)
    for kh, kw in order or [(a, b) for a in range(3) for b in range(3)]:
        hn, wn = h + 1 - kh, w + 1 - kw
        hs, ws = h[(hn >= 0) & (hn % 2 == 0) & (hn // 2 < Ho)], w[(wn >= 0) & (wn % 2 == 0) & (wn // 2 < Wo)]
        if len(hs) and len(ws):
            acc[np.ix_(range(B), hs, ws)] = acc[np.ix_(range(B), hs, ws)] + d[np.ix_(range(B), (hs + 1 - kh) // 2, (ws + 1 - kw) // 2)][:, :, :, kh * 3 + kw]
    return masked(acc, None if mask is None else mask.reshape(acc.shape))


def relu_grad(dy, y):
    return np.where(y > 0, dy, F(0))


def mask_data(shape, seed):
    """Mixed-sign data with exact +0.0 and -0.0 planted (every 7th and every 11th element): both zero the gradient."""
    m = np.random.default_rng(seed).standard_normal(int(np.prod(shape))).astype(F)
    m[3::7] = F(0.0)
    m[5::11] = F(-0.0)
    return m.reshape(shape)


# ---- the shapes both test files walk: the smallest that reach each boundary ---------------------------------------------------------------------
# name -> (Geom, Cin, Cout, leaves, leaves the model computes or None for all)
WGRAD_CASES = {
    "1x1_105px": (Geom(3, 5, 7, 1, 1), 64, 128, 1, None),               # K = 105: no multiple of 32
    "1x1_short_and_empty_split": (Geom(1, 26, 50, 1, 1), 64, 64, 1, None),   # K = 1300: 41 k-tiles, 10 splits of 5; split 8 holds 20 pixels, split 9 none
    "1x1_stride2_odd": (Geom(2, 7, 5, 1, 2), 128, 64, 1, None),
    "3x3_W1": (Geom(2, 5, 1, 9, 1), 64, 64, 1, None),
    "3x3_H1": (Geom(1, 1, 37, 9, 1), 64, 64, 1, None),                   # two k-tiles
    "3x3_2x2": (Geom(3, 2, 2, 9, 1), 64, 64, 1, None),                   # every tap but the centre hits a border at every pixel
    "3x3_stride2_odd": (Geom(2, 7, 9, 9, 2), 64, 128, 1, None),
    "1x1_two_leaves": (Geom(4, 5, 7, 1, 1), 64, 64, 2, None),            # K = 70: leaf 1 starts inside a 32-pixel tile of the launch
    "1x1_stride2_two_leaves": (Geom(2, 7, 5, 1, 2), 128, 64, 2, None),
    "3x3_three_leaves": (Geom(3, 16, 17, 9, 1), 64, 64, 3, None),        # K = 272: 9 k-tiles, two splits of 5 and 4, the last tile 16 pixels
    # the smallest launches isx_conv_wgrad_nhwc sends to the 128x128 tile: (Cout / 128)(Cin / 128) taps leaves S >= 512
    "big_3x3": (Geom(29, 16, 17, 9, 1), 128, 128, 29, (0, 28)),          # K = 272, S = 2: 9 * 29 * 2 = 522 (28 leaves: 504)
    "big_1x1_stride2": (Geom(16, 61, 73, 1, 2), 256, 256, 16, (0, 15)),  # K = 31 * 37 = 1147: 36 k-tiles, S = 8 (7 x 5 tiles + 27 pixels): 4 * 16 * 8 = 512
}
WGRAD_BIG = ("big_3x3", "big_1x1_stride2")
LAYER4_SHAPES = ((1176, 1024, 512, 1), (1176, 512, 512, 9), (1176, 512, 2048, 1), (1176, 2048, 512, 1), (1176, 1024, 2048, 1), (4704, 1024, 512, 1),
                 (49, 512, 512, 9), (49, 2048, 512, 1), (196, 1024, 512, 1))      # (pixels of one leaf, Cin, Cout, taps)

FOLD_COUT = 8
# offset of the fold cases' seeds.  A case has 8 x leaves values of ggamma and gbeta: with some seeds a wrong variant of tests/test_suffix_model.py
# gives the same eight floats in one case or another (0, 1 and 2 do); with this one every variant shows in every case
FOLD_SEED = 3
FOLD_SHAPES = ((1, 64), (1, 100), (1, 2048), (9, 64), (9, 512), (9, 576))        # (taps, Cin): direct x 3, LDS, LDS at kFoldRow, direct
FOLD_CASES = tuple((taps, Cin, leaves, S) for taps, Cin in FOLD_SHAPES for leaves in (1, 3) for S in (1, 3))

DGRAD1_M = (1, 64, 65, 129)
DGRAD1_CIN = (64, 100, 128)                       # 100: a clipped last column tile
DGRAD1_COUT = (64, 80, 192)                       # 80: no multiple of 32 -- the unaligned loads, with a zero-filled last k-tile
# name -> (B, H, W, Cout, Cin, zero-upsampled from stride 2)
DGRAD3_CASES = {
    "W1": (2, 5, 1, 64, 64, False),
    "H1": (1, 1, 37, 64, 64, False),
    "2x2": (3, 2, 2, 64, 64, False),
    "9x8_three_row_tiles": (2, 9, 8, 64, 96, False),                     # 144 pixels; Cin = 96: a clipped second column tile
    "7x9_upsampled": (2, 7, 9, 64, 64, True),
}
COL2IM_CASES = ((2, 7, 9, 8), (1, 8, 6, 64), (2, 1, 5, 4), (1, 6, 1, 12), (3, 2, 2, 4))      # (B, H, W, Cin)
RELU_N = (8, 1028, 100000)                      # 8: two float4s, with one zero of each sign


# ---- shared, read-only cases ------------------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False
    return arrays


def wgrad_K(name):
    g, _, _, leaves, _ = WGRAD_CASES[name]
    Ho, Wo = out_hw(g)
    return g.B // leaves * Ho * Wo


@functools.lru_cache(maxsize=None)
def wgrad_inputs(name):
    """(dz (B Ho Wo, Cout), x (B H W, Cin))."""
    g, Cin, Cout, _, _ = WGRAD_CASES[name]
    Ho, Wo = out_hw(g)
    seed = 100 * sorted(WGRAD_CASES).index(name)
    return _frozen(inputs(g.B * Ho * Wo, Cout, seed), inputs(g.B * g.H * g.W, Cin, seed + 1))


@functools.lru_cache(maxsize=None)
def wgrad_case(name, S):
    """(dw, db) of the leaves the model computes (WGRAD_CASES) at S splits."""
    g, _, _, leaves, which = WGRAD_CASES[name]
    dz, x = wgrad_inputs(name)
    return _frozen(*wgrad_partials(dz, x, g, leaves, S, which))


@functools.lru_cache(maxsize=None)
def fold_params(taps, Cin, Cout=FOLD_COUT):
    """(w (Cout, Cin, taps), scale, mean, istd)."""
    rng = np.random.default_rng(31 * Cin + taps)
    # w * 2^-10 (exact) and db (fold_case) of plain normals * 32: <d, w> and mean * db come out at the same size, as they do in a trained layer -- with
    # the dot product decades above mean * db, (dot - mean * db) * istd and dot * istd - mean * db * istd gave the same eight floats in two cases
    w = inputs(Cout, Cin * taps, 17 * Cin + taps, special_rows=False).reshape(Cout, Cin, taps) * F(2.0 ** -10)
    istd = (1 / np.sqrt(0.5 + rng.random(Cout) + 1e-5)).astype(F)
    return _frozen(w, ((0.5 + rng.random(Cout)).astype(F) * istd).astype(F), rng.standard_normal(Cout).astype(F), istd)


@functools.lru_cache(maxsize=None)
def fold_case(taps, Cin, leaves, S):
    """(dwp, db, priors (gw, ggamma, gbeta), result without priors, result on the priors)."""
    seed = 1000 * Cin + 100 * taps + 10 * leaves + S + FOLD_SEED
    dwp = inputs(leaves * S * FOLD_COUT, taps * Cin, seed, special_rows=False).reshape(leaves, S, FOLD_COUT, taps, Cin)
    rng = np.random.default_rng(seed + FOLD_SEED)
    db = rng.standard_normal((leaves, S, FOLD_COUT)).astype(F) * F(32)
    prior = (rng.standard_normal((leaves, FOLD_COUT, Cin, taps)).astype(F), rng.standard_normal((leaves, FOLD_COUT)).astype(F),
             rng.standard_normal((leaves, FOLD_COUT)).astype(F))
    w, scale, mean, istd = fold_params(taps, Cin)
    plain = fold_backward(dwp, db, w, scale, mean, istd, taps)
    return _frozen(dwp, db) + (_frozen(*prior), _frozen(*plain), _frozen(*fold_backward(dwp, db, w, scale, mean, istd, taps, prior)))


@functools.lru_cache(maxsize=None)
def dgrad1_case(Cin, Cout):
    """(dz, wt, add, mask, chains) at the LARGEST M: output row m is a function of row m of dz alone, so a smaller case is the first M rows."""
    M = max(DGRAD1_M)
    # wt * 2^-10 (exact): the outputs are of the size (~ 30) at which tests/test_gpu_suffix.py's ABSOLUTE bound for this quantity (atol 1e-3 on sums
    # of 192 products of unit normals) means what it means there; columns scaled over four decades each way would put them at 3e4
    dz, wt = inputs(M, Cout, 3 * Cin + Cout, special_rows=False), inputs(Cin, Cout, 3 * Cin + Cout + 1, special_rows=False) * F(2.0 ** -10)
    add = np.random.default_rng(3 * Cin + Cout + 2).standard_normal((M, Cin)).astype(F)
    return _frozen(dz, wt, add, mask_data((M, Cin), 3 * Cin + Cout + 3), chains(dz, wt))


def dgrad1_want(Cin, Cout, M, with_add, with_mask):
    _, _, add, mask, v = dgrad1_case(Cin, Cout)
    v = v[:M] + add[:M] if with_add else v[:M]
    return masked(v, mask[:M] if with_mask else None)


@functools.lru_cache(maxsize=None)
def dgrad3_case(name):
    """(dz (B, H, W, Cout), wt (Cin, 3, 3, Cout), mask, unmasked result)."""
    B, H, W, Cout, Cin, up = DGRAD3_CASES[name]
    seed = 50 * sorted(DGRAD3_CASES).index(name) + 7
    dz = inputs(B * H * W, Cout, seed, special_rows=False).reshape(B, H, W, Cout)     # (a zero row would leave zero outputs: nothing for a mask to hide)
    if up:                                        # what a stride-2 layer hands in: its gradient on the even pixels, zeros between
        z = np.zeros_like(dz)
        z[:, ::2, ::2] = dz[:, ::2, ::2]
        dz = z
    wt = inputs(Cin, 9 * Cout, seed + 1, special_rows=False).reshape(Cin, 3, 3, Cout)
    return _frozen(dz, wt, mask_data((B, H, W, Cin), seed + 2), dgrad3x3(dz, wt))


@functools.lru_cache(maxsize=None)
def col2im_case(B, H, W, Cin):
    """(dcol, mask, unmasked result)."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    seed = 1000 * H + 10 * W + B
    # plain normals: with the columns scaled over logspace(-2, 2) the four taps of a pixel lie decades apart, the sum is its largest term in almost any
    # order and the (kw, kh) order changed under 1 % of the elements
    dcol = np.random.default_rng(seed).standard_normal((B * Ho * Wo, 9, Cin)).astype(F)
    return _frozen(dcol, mask_data((B, H, W, Cin), seed + 1), col2im_s2(dcol, B, H, W, Cin))


@functools.lru_cache(maxsize=None)
def relu_case(n):
    dy = np.random.default_rng(n).standard_normal(n).astype(F)
    y = mask_data((n,), n + 1)
    return _frozen(dy, y, relu_grad(dy, y))
