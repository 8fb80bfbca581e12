"""The fp16 search kernels (csrc/fast.hip: the scaled conversions, the three fp16 GEMM kernels in their eight instantiations, window / rescore /
compact / gather behind isx_cosine_topk_fast) called through the C ABI with buffers the TEST owns (tests/_guards.py): every output is a poisoned
body between sentinel guards, every operand sits between NaN guards, the workspace is exactly the size asked for between 4 KiB of a byte
pattern.  test_gpu_fast.py forces the same tile shapes through isx.ops, which allocates outputs and workspaces from torch's caching allocator:
a store past the last row of a 256-row tile, flag bytes that run over their slot, or an operand read past the last gallery row pass there.

Every GEMM case names the instantiation it means to reach and asserts it with the restated host arithmetic of _guards.py (f16_gemm_kernel,
topk_chunks) before launching; test_every_f16_gemm_instantiation_is_reached unions these plans (no GPU needed).

Which chunks filter.  run_topk_chunks (csrc/cosine.hip:84-114) runs the FIRST column chunk with the plain epilogue and shortens it to 8192
columns only from N = 32768 on (:88).  With a workspace of isx_cosine_topk_fast_workspace(...) bytes the shapes of this file (N <= 9000) are ONE
plain chunk: no FILTER instantiation runs.  The FILTER instantiations are reached with narrower workspaces whose chunk widths the cases state
(and topk_chunks confirms): ngrp = ceil(width / 32) of a filtered chunk, not of N, decides between the 8-byte and the byte-by-byte flag store.

Alignment (read before offsetting): rows_to_f16_kernel takes its 16-byte path only when D % 8 == 0 and x | h are 16-byte aligned (csrc/fast.hip:106),
amax_kernel only when x is (:58), both otherwise load and store element by element; norm2 / amax / gstats are written as single floats.  So
isx_rows_to_f16 and isx_gallery_to_f16 need nothing beyond the natural alignment of their element types, and no refusal was added.
isx_cosine_sim_f16 checks its 16-byte requirement on Qh | Gh itself; its score stores are scalar (any 4-byte aligned sim)."""
import contextlib

import numpy as np
import pytest
import torch

import _guards as G
import oracle as O

gpu = pytest.mark.gpu
F = np.float32
H = np.float16
NO_WS = (1 << 64) - 1                                   # (size_t)-1
ERR_WORKSPACE = -2

K128, K128F = "cosine_gemm_f16_kernel<false>", "cosine_gemm_f16_kernel<true>"
BIG, BIG_K = "cosine_gemm_f16_big_kernel<false,false>", "cosine_gemm_f16_big_kernel<false,true>"
BIGF, BIGF_K = "cosine_gemm_f16_big_kernel<true,false>", "cosine_gemm_f16_big_kernel<true,true>"
PP, PPF = "gemm_f16_pp_kernel<false>", "gemm_f16_pp_kernel<true>"


def _lib():
    from isx._lib import lib
    return lib(), torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def f16_tile(t):
    """isx_debug_set_f16_tile: 0 = 128x128, 1 = 256x256 (ping-pong when D % 64 == 0), 2 = 256x256 register-staged, -1 = automatic."""
    L = _lib()[0]
    try:
        L.isx_debug_set_f16_tile(t)
        yield
    finally:
        L.isx_debug_set_f16_tile(-1)


def _ok(rc, what=""):
    assert rc == 0, (what, rc, _lib()[0].isx_last_error())


def unit(rng, n, d):
    x = rng.standard_normal((n, d), dtype=F)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F)


# ---- models and bounds shared with tests/test_gpu_stream_order.py ------------------------------------------------------------------------------
def norm2_within(got, x, what=""):
    """norm2 of isx_rows_to_f16 is an upper bound of the exact sum of squares that D + 1 fp32 roundings and the kernel's own 1.000001 explain."""
    D = x.shape[1]
    exact = (x.astype(np.float64) ** 2).sum(1)
    got = np.asarray(got).astype(np.float64)
    assert (got >= exact * (1 - 1e-6)).all(), what
    assert (got <= exact * (1 + 2e-6 + (D + 2) * 2.0 ** -23)).all(), what


def gallery_f16_model(Gm):
    """(Gh, n2max, amax, lost) of isx_gallery_to_f16: power-of-two scaling into [2^13, 2^14), RNE, results below the fp16 normal range stored
    as +0; the largest squared norm, max |x| and the largest squared loss of a row."""
    amax = np.abs(Gm).max()
    scale = 2.0 ** (13 - np.floor(np.log2(amax)))
    want = (Gm * F(scale)).astype(H)
    want[np.abs(want.astype(F)) < 2.0 ** -14] = 0
    lost = ((Gm.astype(np.float64) - want.astype(np.float64) / scale) ** 2).sum(1).max()
    return want, (Gm.astype(np.float64) ** 2).sum(1).max(), amax, lost


def gstats_within(s, n2max, amax, lost, D, what=""):
    """gstats = {max squared norm (upper bound), max |x|, largest squared loss of a row (upper bound within 0.1 %), 0}."""
    assert s[1] == amax and s[3] == 0.0 and G.bits(s)[3] == 0, (what, s.tolist())
    assert n2max * (1 - 1e-6) <= s[0] <= n2max * (1 + 2e-6 + (D + 2) * 2.0 ** -23), (what, s.tolist(), n2max)
    assert lost <= s[2] <= lost * 1.001, (what, s.tolist(), lost)


def sim_f16_bound(q, g):
    """(float64 product, bound) of isx_cosine_sim_f16: fp16 products are exact in fp32, only the D accumulation steps round."""
    q64, g64 = q.astype(np.float64), g.astype(np.float64)
    return q64 @ g64.T, (np.abs(q64) @ np.abs(g64).T) * q.shape[1] * 2.0 ** -23 + 1e-30


# ---- 1. isx_rows_to_f16, isx_gallery_to_f16 --------------------------------------------------------------------------------------------------------
CONV_SHAPES = [(B, D) for B in (1, 5, 67) for D in (8, 200, 2056)]      # B = 5: a last block of one row; D = 200 / 2056: lanes idle / a fourth pass of lane 0


@gpu
@pytest.mark.parametrize("B,D", CONV_SHAPES)
def test_rows_to_f16(B, D):
    """h equals numpy's IEEE half conversion bit for bit (RNE, gradual underflow, +-65504, +-0), amax is exact, norm2 is an upper bound (the
    bound of test_rows_to_f16_matches_ieee_half) that D + 1 fp32 roundings and the kernel's own 1.000001 explain; x one float and h one half
    off their 256-byte boundaries take the element-wise loop."""
    L, st = _lib()
    rng = np.random.default_rng(20 + B * D)
    x = rng.standard_normal((B, D), dtype=F)
    x[0, :min(D, 50)] = rng.standard_normal(min(D, 50)).astype(F) * F(1e-6)          # fp16 subnormal range
    x[min(1, B - 1), :8] = [65504.0, -65504.0, 6.1e-5, 5.96e-8, 2.9e-8, 0.0, -0.0, 1.0009765625]
    want_h = x.astype(H)
    for ox, oh in ((0, 0), (1, 0), (0, 1), (1, 1)):
        what = ("offsets", ox, oh)
        gx = G.in_f32(x, 8 * D + 1024, ox)
        h, n2, am = G.out_f16((B, D), 8 * D + 1024, oh), G.out_f32((B,), 1024, ox), G.out_f32((B,), 1024, ox)
        with f16_tile(-1):
            _ok(L.isx_rows_to_f16(gx.ptr, B, D, h.ptr, n2.ptr, am.ptr, st), what)
        G.assert_clean([h, n2, am], [gx], what)
        G.assert_bits(h, want_h, what)
        G.assert_bits(am, np.abs(x).max(1), what)
        norm2_within(n2.host(), x, what)


@gpu
@pytest.mark.parametrize("N,D", CONV_SHAPES)
def test_gallery_to_f16(N, D):
    """Gh of exactly N * D * 2 bytes and gstats of exactly 16 bytes, both poisoned between guards, against the model of
    test_gallery_to_f16_scaling: power-of-two scaling into [2^13, 2^14), RNE, results below the fp16 normal range stored as +0;
    gstats = {max squared norm (upper bound), max |x|, largest squared loss of a row (upper bound within 0.1 %), 0}."""
    L, st = _lib()
    rng = np.random.default_rng(21 + N * D)
    Gm = unit(rng, N, D) * F(0.3)
    r = min(3, N - 1)
    Gm[r, 1:6] = F(1e-12) * np.arange(1, 6, dtype=F)                                  # below the fp16 normal range after scaling
    Gm[r, 6] = F(-1e-12)                                                              # and a negative one: flushed to +0
    want, n2max, amax, lost = gallery_f16_model(Gm)
    assert (want[r, 1:7].view(np.uint16) == 0).all()
    assert lost > 0
    for ox in (0, 1):
        gx = G.in_f32(Gm, 8 * D + 1024, ox)
        gh, gs = G.out_f16((N, D), 8 * D + 1024), G.out_f32((4,), 1024)
        assert gh.n * 2 == N * D * 2 and gs.n * 4 == 16
        with f16_tile(-1):
            _ok(L.isx_gallery_to_f16(gx.ptr, N, D, gh.ptr, gs.ptr, st), ox)
        G.assert_clean([gh, gs], [gx], ox)
        G.assert_bits(gh, want, ox)
        gstats_within(gs.host(), n2max, amax, lost, D, ox)


@gpu
def test_gallery_to_f16_of_no_rows():
    """N = 0: gstats is written as zeros, Gh is not touched."""
    L, st = _lib()
    gx = G.in_f32(np.ones((1, 8), F), 1024)
    gh, gs = G.out_f16((4, 8), 1024), G.out_f32((4,), 1024)
    for g_ptr, h_ptr in ((gx.ptr, gh.ptr), (None, None)):
        gs.raw().fill_(gs.poison)
        with f16_tile(-1):
            _ok(L.isx_gallery_to_f16(g_ptr, 0, 8, h_ptr, gs.ptr, st))
        G.assert_clean([gs], [gx])
        assert (G.bits(gs.host()) == 0).all()
        assert gh.unwritten() == gh.n and gh.guards_intact()


# ---- 2. isx_cosine_sim_f16 ---------------------------------------------------------------------------------------------------------------------
# (M, N, D) -> the instantiation meant under hooks 0 / 1 / 2 / -1
SIM_CASES = [
    ((1, 1, 8), (K128, BIG, BIG, K128)),                      # a single partial k-tile
    ((130, 257, 64), (K128, PP, BIG_K, K128)),                # ragged in both directions, one full k-tile
    ((257, 600, 200), (K128, BIG, BIG, K128)),                # D % HBK != 0: the not-FULLK register-staged kernel under hooks 1 and 2
    ((256, 512, 256), (K128, PP, BIG_K, K128)),               # only `interior` tiles of the ping-pong kernel
    ((513, 700, 192), (K128, PP, BIG_K, K128)),               # interior and edge tiles in one grid, three k-tiles
]
SIM_HOOKS = (0, 1, 2, -1)


def _sim_plan(case):
    (M, N, D), means = case
    got = tuple(G.f16_gemm_kernel(t, M, N, D, False) for t in SIM_HOOKS)
    assert got == means, (M, N, D, got, means)
    return set(got)


def test_sim_cases_reach_what_they_mean():
    for case in SIM_CASES:
        _sim_plan(case)
    (M, N, D), _ = SIM_CASES[3]
    assert M % G.GBM == 0 and N % G.GBN == 0 and D % G.HBK == 0            # interior tiles only
    (M, N, D), _ = SIM_CASES[4]
    assert M > 2 * G.GBM and N > 2 * G.GBN and M % G.GBM and N % G.GBN and D // G.HBK == 3


@gpu
@pytest.mark.parametrize("case", SIM_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_cosine_sim_f16(case):
    """sim poisoned between guards of 256 * N floats (every address a dead row of the last 256-row tile maps to), on its boundary and one
    float off it; Qh / Gh between 256 rows of half NaNs (16-byte aligned, as the entry requires), with rows of fp16 subnormals.  The four tile
    choices give the same bits, no NaN, and every score is within (|q| . |g|) D 2^-23 of the float64 product (the bound test_gpu_fast.py
    derives: fp16 products are exact in fp32, only the D accumulation steps round)."""
    L, st = _lib()
    (M, N, D), _ = case
    _sim_plan(case)
    rng = np.random.default_rng(M + N + D)
    q = rng.standard_normal((M, D)).astype(H)
    g = rng.standard_normal((N, D)).astype(H)
    q[0] = (rng.standard_normal(D) * 3e-6).astype(H)                          # subnormal halves
    g[0] = (rng.standard_normal(D) * 3e-6).astype(H)
    want, bound = sim_f16_bound(q, g)
    ins = [G.in_f16(q, 256 * D), G.in_f16(g, 256 * D)]
    assert (ins[0].ptr | ins[1].ptr) % 16 == 0
    first = None
    for off in (0, 1):
        for tile in SIM_HOOKS:
            what = ("tile", tile, "sim offset", off)
            sim = G.out_f32((M, N), 256 * N, off)
            with f16_tile(tile):
                _ok(L.isx_cosine_sim_f16(ins[0].ptr, M, ins[1].ptr, N, D, sim.ptr, st), what)
            G.assert_clean([sim], ins, what)
            got = sim.host()
            assert not np.isnan(got).any(), what
            if first is None:
                first = got
                assert (np.abs(got - want) <= bound).all(), (what, float((np.abs(got - want) / bound).max()))
                assert np.abs(got[0]).max() > 0 and (N == 1 or np.abs(got[1:, 0]).max() > 0)       # subnormal operands contributed
            else:
                G.assert_bits(got, first, what)


@gpu
def test_cosine_sim_f16_refuses_misaligned_operands():
    """Operands one half off a 16-byte boundary are refused and sim stays untouched."""
    L, st = _lib()
    q, g = np.ones((4, 8), H), np.ones((4, 8), H)
    for oq, og in ((1, 0), (0, 1)):
        ins = [G.in_f16(q, 1024, oq), G.in_f16(g, 1024, og)]
        sim = G.out_f32((4, 4), 1024)
        with f16_tile(-1):
            assert L.isx_cosine_sim_f16(ins[0].ptr, 4, ins[1].ptr, 4, 8, sim.ptr, st) != 0
        assert sim.unwritten() == sim.n and sim.guards_intact()


# ---- 3. isx_cosine_topk_fast -------------------------------------------------------------------------------------------------------------------
# (M, N, D, k), chunk widths of the narrow workspaces, the FILTER instantiation meant under hooks 0 / 1 / 2.
#   2432 = 9.5 tiles of 256: filtered chunks of 2432, 2432 and 1704 columns, ngrp = 76 and 54 (no multiples of 8: flag bytes one by one), every tile
#          ragged in M, the last one of a chunk ragged in N
#   2816 = 11 tiles: three chunks, ngrp = 88 = 8 * 11: the 8-byte flag store in the interior tiles of rows 0..255, the byte stores in rows 256..299
#   2944 = 11.5 tiles: ngrp = 92 (interior tiles that must NOT take the 8-byte store), then a last chunk of 2560 columns with ngrp = 80
TOPK_CASES = [
    ((37, 9000, 64, 10), (2432,), (K128F, PPF, BIGF_K)),
    ((300, 8448, 128, 100), (2816, 2944), (K128F, PPF, BIGF_K)),
    ((37, 9000, 72, 10), (2432,), (K128F, BIGF, BIGF)),                    # D % HBK != 0: the filter in the not-FULLK register-staged kernel
]
TOPK_HOOKS = (0, 1, 2)
IDX_BASE = 11


def _ws_bytes(M, N, D, k, cached, nc):
    """Workspace bytes under which the approximate pass runs chunks of nc columns (nc = None: the size the library recommends; 128: the minimum
    the entry accepts)."""
    chunk_at, total = G.fast_layout(M, N, D, k, not cached)
    fixed = G.topk_fixed_bytes(M, G.fast_kl(k))
    if nc is None:
        return total
    if nc == 128:
        return chunk_at + fixed + G.topk_chunk_bytes(M, 128)
    return chunk_at + fixed + 4 * M * (nc + 128)


def _topk_plan(case, cached):
    """{(workspace chunk width, hook): set of instantiations}; asserts the chunks and the instantiations the case means."""
    (M, N, D, k), ncs, means = case
    kl = G.fast_kl(k)
    assert N > 4 * kl and k <= 128 and D % 8 == 0                            # fast_applicable (csrc/fast.hip:942)
    chunk_at, _ = G.fast_layout(M, N, D, k, not cached)
    plan = {}
    for nc in (None, 128) + tuple(ncs):
        chunks = G.topk_chunks(M, N, kl, _ws_bytes(M, N, D, k, cached, nc) - chunk_at, True)
        if nc is None:
            assert chunks == [(0, N, False)]                                 # N < 32768: one plain chunk
        else:
            assert [w for _, w, _ in chunks[:-1]] == [nc] * (len(chunks) - 1) and len(chunks) >= 3 and not chunks[0][2] and all(c[2] for c in chunks[1:]), chunks
        for t in TOPK_HOOKS:
            plan[nc, t] = {G.f16_gemm_kernel(t, M, w, D, f) for _, w, f in chunks}
            if nc is not None:
                assert means[t] in plan[nc, t], (nc, t, plan[nc, t])
    return plan


def test_topk_cases_reach_what_they_mean():
    for cached in (True, False):
        for case in TOPK_CASES:
            _topk_plan(case, cached)
    ngrp = lambda M, N, k, nc: [(w + 31) // 32 for _, w, f in G.topk_chunks(M, N, G.fast_kl(k), G.topk_fixed_bytes(M, G.fast_kl(k)) + 4 * M * (nc + 128), True) if f]
    assert ngrp(37, 9000, 10, 2432) == [76, 76, 54]
    assert ngrp(300, 8448, 100, 2816) == [88, 88] and 88 % 8 == 0 and 300 > G.GBM and 2816 % G.GBN == 0
    assert ngrp(300, 8448, 100, 2944) == [92, 80] and 2944 % G.GBN == 128
    assert ngrp(37, 9000, 10, 128)[-1] == (9000 % 128 + 31) // 32                # chunks narrower than a 256-column tile: flag bytes 4..7 of a row are not this chunk's


def _search(L, st, shape, Q, Gm, cached_regions, nbytes, tile, want, what, oout=0):
    M, N, D, k = shape
    qg = [G.in_f32(Q, 256 * D), G.in_f32(Gm, 256 * D)]
    gh, gs = cached_regions
    cached = gh is not None
    assert L.isx_cosine_topk_fast_fallback_offset(M, N, D, k, int(cached)) != NO_WS, "the shape must take the fp16 filter path"
    ws = G.workspace(nbytes)
    ts, ti = G.out_f32((M, k), 256 * k, oout), G.out_i64((M, k), 256 * k, oout)
    with f16_tile(tile):
        _ok(L.isx_cosine_topk_fast(qg[0].ptr, M, qg[1].ptr, N, D, k, IDX_BASE, G.ptr(gh), G.ptr(gs), ts.ptr, ti.ptr, ws.ptr, nbytes, st), what)
        fb = L.isx_debug_fast_fallback_rows(ws.ptr, M, N, D, k, int(cached))
    G.assert_clean([ts, ti], qg, what)
    assert ws.guards_intact(), ("store outside the workspace", what)
    assert gh is None or (gh.guards_intact() and gs.guards_intact()), ("cached gallery image touched", what)
    assert fb >= 0, what
    G.assert_bits(ts, want[0], what)
    np.testing.assert_array_equal(ti.host(), want[1], err_msg=str(what))
    return fb


def _cached_gallery(L, st, Gm, cached):
    if not cached:
        return None, None
    N, D = Gm.shape
    gx = G.in_f32(Gm, 256 * D)
    gh, gs = G.out_f16((N, D), 256 * D), G.out_f32((4,), 1024)
    with f16_tile(-1):
        _ok(L.isx_gallery_to_f16(gx.ptr, N, D, gh.ptr, gs.ptr, st), "isx_gallery_to_f16")
    G.assert_clean([gh, gs], [gx])
    return gh, gs


@gpu
@pytest.mark.parametrize("cached", [True, False])
@pytest.mark.parametrize("case", TOPK_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_cosine_topk_fast(case, cached):
    """Bit for bit the oracle's lists (duplicate gallery rows: the index tie-break decides; idx_base != 0) under the three tile choices, with the
    workspace the library recommends (one plain chunk), with the narrow ones of TOPK_CASES (filtered chunks) and, under the ping-pong hook, with
    the smallest one the entry accepts (128-column chunks) and one byte less (ISX_ERR_WORKSPACE, outputs untouched)."""
    L, st = _lib()
    shape, ncs, _ = case
    M, N, D, k = shape
    plan = _topk_plan(case, cached)
    rng = np.random.default_rng(N + k + D)
    Q, Gm = unit(rng, M, D), unit(rng, N, D)
    Gm[N // 2] = Gm[3]
    Gm[N - 1] = Gm[3]
    want = O.cosine_topk(Q, Gm, k, idx_base=IDX_BASE)
    regions = _cached_gallery(L, st, Gm, cached)
    assert _ws_bytes(M, N, D, k, cached, None) == L.isx_cosine_topk_fast_workspace(M, N, D, k, int(cached))
    for nc in (None,) + tuple(ncs):
        for tile in TOPK_HOOKS:
            _search(L, st, shape, Q, Gm, regions, _ws_bytes(M, N, D, k, cached, nc), tile, want, ("chunks of", nc, "tile", tile, sorted(plan[nc, tile])),
                    oout=int(nc is not None))
    minimum = _ws_bytes(M, N, D, k, cached, 128)
    _search(L, st, shape, Q, Gm, regions, minimum, 1, want, ("the minimum workspace", minimum, sorted(plan[128, 1])))
    qg = [G.in_f32(Q, 256 * D), G.in_f32(Gm, 256 * D)]
    ws = G.workspace(minimum - 1)
    ts, ti = G.out_f32((M, k), 256 * k), G.out_i64((M, k), 256 * k)
    with f16_tile(1):
        rc = L.isx_cosine_topk_fast(qg[0].ptr, M, qg[1].ptr, N, D, k, IDX_BASE, G.ptr(regions[0]), G.ptr(regions[1]), ts.ptr, ti.ptr, ws.ptr, minimum - 1, st)
    assert rc == ERR_WORKSPACE, rc
    torch.cuda.synchronize()
    assert ts.unwritten() == ts.n and ti.unwritten() == ti.n and ts.guards_intact() and ti.guards_intact()
    assert ws.guards_intact() and ws.unwritten() == ws.n


# Fallback rows: the construction of test_dense_clusters_take_the_exact_fallback (8 centres, 1e-4 perturbations, k = 20) shrunk to 9 queries x 1024
# rows x 64.  On the CPU (the conversion and the error bound of csrc/fast.hip restated in numpy, approximate scores in float64) between 108 and 271
# scores of every query lie inside the window of the 20th best, against KL = 96 candidates kept: all 9 rows fall back.  At N = 512 the same
# model finds 54..71 (< 96): no fallback.
FALLBACK_SHAPE = (9, 1024, 64, 20)


def fallback_case():
    """(Q, G) of FALLBACK_SHAPE: 8 centres, 1e-4 perturbations, two duplicates of row 3."""
    M, N, D, k = FALLBACK_SHAPE
    rng = np.random.default_rng(7)
    c = unit(rng, 8, D)
    Gm = c[rng.integers(0, 8, N)] + F(1e-4) * rng.standard_normal((N, D), dtype=F)
    Gm = (Gm / np.linalg.norm(Gm, axis=1, keepdims=True)).astype(F)
    Gm[N // 2] = Gm[3]
    Gm[N - 1] = Gm[3]
    return unit(rng, M, D), Gm


@gpu
@pytest.mark.parametrize("cached", [True, False])
def test_fallback_rows_write_through_the_row_map(cached):
    L, st = _lib()
    M, N, D, k = FALLBACK_SHAPE
    assert G.f16_gemm_kernel(1, M, N, D, False) == PP
    Q, Gm = fallback_case()
    want = O.cosine_topk(Q, Gm, k, idx_base=IDX_BASE)
    regions = _cached_gallery(L, st, Gm, cached)
    for nc in (None, 256):
        fb = _search(L, st, FALLBACK_SHAPE, Q, Gm, regions, _ws_bytes(M, N, D, k, cached, nc), 1, want, ("dense clusters, chunks of", nc), oout=1)
        assert fb > 0


@gpu
@pytest.mark.parametrize("cached", [True, False])
def test_non_finite_query_row(cached):
    """One +inf in one query row: max |Q| is not finite, no row may use the fp16 scores, every row takes the exact search.  The row's scores are
    +-inf (no NaN: the gallery holds no zero): its list is ten +inf ties in index order."""
    L, st = _lib()
    shape = M, N, D, k = 37, 9000, 64, 10
    assert G.f16_gemm_kernel(1, M, N, D, False) == PP
    rng = np.random.default_rng(5)
    Q, Gm = unit(rng, M, D), unit(rng, N, D)
    Gm[N // 2] = Gm[3]
    Gm[N - 1] = Gm[3]
    Q[3, 7] = np.inf
    assert (Gm[:, 7] != 0).all()
    want = O.cosine_topk(Q, Gm, k, idx_base=IDX_BASE)
    assert np.isinf(want[0][3]).all() and not np.isnan(want[0]).any()
    regions = _cached_gallery(L, st, Gm, cached)
    for nc in (None, 2432):
        fb = _search(L, st, shape, Q, Gm, regions, _ws_bytes(M, N, D, k, cached, nc), 1, want, ("+inf in a query row, chunks of", nc))
        assert fb == M


# ---- 0. every instantiation is named by a case ----------------------------------------------------------------------------------------------
def test_every_f16_gemm_instantiation_is_reached():
    reached = set()
    for case in SIM_CASES:
        reached |= _sim_plan(case)
    for case in TOPK_CASES:
        for cached in (True, False):
            for names in _topk_plan(case, cached).values():
                reached |= names
    assert len(G.F16_GEMMS) == 8 and reached == set(G.F16_GEMMS), sorted(set(G.F16_GEMMS) - reached)
