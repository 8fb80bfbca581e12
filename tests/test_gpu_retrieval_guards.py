"""The retrieval kernels (score GEMM, top-k, merge, full ranking, average precision, masked sums) called through the C ABI with buffers the
TEST owns (tests/_guards.py): every output is a poisoned body between sentinel guards, every operand sits between NaN (labels: impossible-label)
guards, every workspace is EXACTLY the size the header documents with 4 KiB of a byte pattern on both sides, and every result equals the
oracle bit for bit.  test_gpu_parity.py checks the same operations through isx.ops, which allocates outputs and workspaces itself: a store
past the declared region, a workspace overrun (isx_rank_full pads N to a power of two) or an element never written passes there.

Alignment: every operand and every output also runs one ELEMENT past its 256-byte boundary.  By the entries' host code and kernels (read
before offsetting): the GEMMs dispatch on the alignment of Q | G (csrc/gemm.hip launch_gemm_any) and store scores one by one; the selection
kernels decide their float4 scan from the row pointer (csrc/select.hip: select_groups_kernel per row, launch_select for k > 256);
isx_average_precision_sim picks its float4 instance from N % 4 and the alignment of sim | glab (csrc/rank.hip); isx_cosine_topk_fast runs the
fp32 search when Q | G | Gh is off a 16-byte boundary; the merge, ranking, sorted-AP and masked-sum kernels and every output store are
scalar.  Only the workspaces must be aligned (256 bytes; isx_rank_full: 16), which the entries check and the header's workspace contract
implies."""
import contextlib
import math

import numpy as np
import pytest
import torch

import _guards as G
import oracle as O

pytestmark = pytest.mark.gpu

F = np.float32
NO_WS = (1 << 64) - 1                                   # (size_t)-1


def _lib():
    from isx._lib import lib
    return lib(), torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def gemm_cfg(c):
    L = _lib()[0]
    try:
        L.isx_debug_set_gemm_cfg(c)
        yield
    finally:
        L.isx_debug_set_gemm_cfg(-1)


def _ok(rc, what=""):
    assert rc == 0, (what, rc, _lib()[0].isx_last_error())


def unit(rng, n, d):
    return O.l2norm_rows(rng.standard_normal((n, d), dtype=F))


def a256(v):
    return (v + 255) // 256 * 256


# ---- isx_cosine_sim ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,D", [(1, 1, 1), (33, 129, 17), (65, 130, 464), (129, 65, 64)])
def test_cosine_sim(M, N, D):
    """Every tile shape; D = 64: the ALIGNED loads, D = 464: the clipped k-tail of 16-byte aligned rows and, one float off the boundary, the
    scalar branch of load_tile for D % 4 == 0; D = 17 / 1: the scalar branch with a ragged k-tail.  The plain stores of the score epilogue take
    any 4-byte alignment of sim."""
    L, st = _lib()
    rng = np.random.default_rng(M * N + D)
    Q, Gm = unit(rng, M, D), unit(rng, N, D)
    want = O.cosine_sim(Q, Gm)
    for oin, oout in ((0, 0), (1, 1), (0, 1), (1, 0)):
        ins = [G.in_f32(Q, 128 * D, oin), G.in_f32(Gm, 128 * D, oin)]
        for cfg in (-1, 0, 1, 2, 3):
            sim = G.out_f32((M, N), 128 * N, oout)
            with gemm_cfg(cfg):
                _ok(L.isx_cosine_sim(ins[0].ptr, M, ins[1].ptr, N, D, sim.ptr, st), ("gemm cfg", cfg, "offsets", oin, oout))
            G.assert_clean([sim], ins, ("gemm cfg", cfg, "offsets", oin, oout))
            G.assert_bits(sim, want, ("gemm cfg", cfg, "offsets", oin, oout))


# ---- isx_cosine_topk / isx_cosine_topk_fast -----------------------------------------------------------------------------------------------------
def _topk_outputs(M, k, off=0):
    return G.out_f32((M, k), 128 * k, off), G.out_i64((M, k), 128 * k, off)


@pytest.mark.parametrize("M,N,D,k", [(4, 50, 16, 100), (37, 1000, 64, 10), (5, 8300, 16, 10)])
def test_cosine_topk_workspaces(M, N, D, k):
    """k > N (padding entries), one chunk, N > 8192 (bootstrap + filtering chunks).  The workspace at exactly the documented minimum (chunks of
    min(N, 128) columns with carry merging) and at exactly isx_cosine_topk_workspace(...)."""
    L, st = _lib()
    rng = np.random.default_rng(N + k)
    Q, Gm = unit(rng, M, D), unit(rng, N, D)
    if N > 40:
        Gm[N // 2] = Gm[3]
        Gm[N - 1] = Gm[3]
    want_s, want_i = O.cosine_topk(Q, Gm, k, idx_base=11)
    nc = min(N, 128)
    minimum = a256(M * k * 8) + a256(M * 4) + a256(M * ((nc + 31) // 32)) + M * nc * 4
    recommended = L.isx_cosine_topk_workspace(M, N, D, k)
    assert minimum <= recommended
    for oin, oout in ((0, 0), (1, 1), (0, 1), (1, 0)):       # Q / G off the boundary: the scalar loads of the plain and the filter GEMM
        ins = [G.in_f32(Q, 128 * D, oin), G.in_f32(Gm, 128 * D, oin)]
        for nbytes in (minimum, recommended):
            what = ("workspace", nbytes, "offsets", oin, oout)
            ws = G.workspace(nbytes)
            ts, ti = _topk_outputs(M, k, oout)
            _ok(L.isx_cosine_topk(ins[0].ptr, M, ins[1].ptr, N, D, k, 11, ts.ptr, ti.ptr, ws.ptr, nbytes, st), what)
            G.assert_clean([ts, ti], ins, what)
            assert ws.guards_intact(), ("store outside the workspace", what)
            G.assert_bits(ts, want_s, what)
            np.testing.assert_array_equal(ti.host(), want_i)
    ins = [G.in_f32(Q, 128 * D), G.in_f32(Gm, 128 * D)]
    ws = G.workspace(minimum - 1)
    ts, ti = _topk_outputs(M, k)
    assert L.isx_cosine_topk(ins[0].ptr, M, ins[1].ptr, N, D, k, 11, ts.ptr, ti.ptr, ws.ptr, minimum - 1, st) == -2      # ISX_ERR_WORKSPACE: the minimum IS the minimum
    assert ts.unwritten() == ts.n and ti.unwritten() == ti.n and ws.guards_intact()


@pytest.mark.parametrize("cached", [True, False])
def test_cosine_topk_fast_workspace(cached):
    """The fp16 filter + exact re-scoring, with the gallery image cached by the caller and converted into the workspace; the workspace is
    exactly isx_cosine_topk_fast_workspace(...)."""
    L, st = _lib()
    M, N, D, k = 16, 4096, 64, 10
    rng = np.random.default_rng(N + k + D)
    Q, Gm = unit(rng, M, D), unit(rng, N, D)
    Gm[N // 2] = Gm[3]
    want_s, want_i = O.cosine_topk(Q, Gm, k, idx_base=5)
    assert L.isx_cosine_topk_fast_fallback_offset(M, N, D, k, int(cached)) != NO_WS, "the shape must take the fp16 filter path"
    ins = [G.in_f32(Q, 128 * D), G.in_f32(Gm, 128 * D)]
    gh = gs = None
    if cached:
        gh, gs = G.Region("u8", (N * D * 2,), 4096), G.out_f32((4,), 1024)
        _ok(L.isx_gallery_to_f16(ins[1].ptr, N, D, gh.ptr, gs.ptr, st), "isx_gallery_to_f16")
        G.assert_clean([gs], ins)
        assert gh.guards_intact()
    nbytes = L.isx_cosine_topk_fast_workspace(M, N, D, k, int(cached))
    off_q = [G.in_f32(Q, 128 * D, 1), G.in_f32(Gm, 128 * D, 1)]     # Q | G off a 16-byte boundary: the entry hands the call to the fp32 search
    for qg, oout in ((ins, 0), (ins, 1), (off_q, 0), (off_q, 1)):
        what = ("Q / G offset", int(qg is off_q), "output offset", oout)
        assert ((qg[0].ptr | qg[1].ptr) % 16 == 0) == (qg is ins)
        ws = G.workspace(nbytes)
        ts, ti = _topk_outputs(M, k, oout)
        _ok(L.isx_cosine_topk_fast(qg[0].ptr, M, qg[1].ptr, N, D, k, 5, G.ptr(gh), G.ptr(gs), ts.ptr, ti.ptr, ws.ptr, nbytes, st), what)
        G.assert_clean([ts, ti], qg, what)
        assert ws.guards_intact() and (gh is None or (gh.guards_intact() and gs.guards_intact())), what
        if qg is ins:
            assert L.isx_debug_fast_fallback_rows(ws.ptr, M, N, D, k, int(cached)) >= 0, what
        G.assert_bits(ts, want_s, what)
        np.testing.assert_array_equal(ti.host(), want_i)


# ---- isx_topk_rows / isx_topk_merge -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,k", [(3, 300, 64), (2, 100003, 7), (2, 5, 8), (2, 2048, 300)])
def test_topk_rows(M, N, k):
    """N = 300 / 2048 (N % 4 == 0): the float4 scans on the boundary, the scalar ones one float off it; odd N: rows of both kinds in one launch;
    k = 300: the workgroup-per-row kernel behind launch_select, k <= 256 the wave-per-row one."""
    L, st = _lib()
    rng = np.random.default_rng(N + k)
    sim = rng.standard_normal((M, N), dtype=F)
    sim[:, N // 3] = sim[:, 1]
    want_s, want_i = O.topk_rows(sim, k, idx_base=3)
    for oin, oout in ((0, 0), (1, 1), (0, 1), (1, 0)):
        gs = G.in_f32(sim, 4096, oin)
        ts, ti = _topk_outputs(M, k, oout)
        _ok(L.isx_topk_rows(gs.ptr, M, N, k, 3, ts.ptr, ti.ptr, st), (oin, oout))
        G.assert_clean([ts, ti], [gs], (oin, oout))
        G.assert_bits(ts, want_s, (oin, oout))
        np.testing.assert_array_equal(ti.host(), want_i)


@pytest.mark.parametrize("P,M,k", [(3, 9, 1), (8, 9, 512)])
def test_topk_merge(P, M, k):
    L, st = _lib()
    rng = np.random.default_rng(P * k)
    N, D = 4000, 32
    Q, Gm = unit(rng, M, D), unit(rng, N, D)
    Gm[100] = Gm[3900]
    bounds = np.linspace(0, N, P + 1).astype(int)
    parts = [O.cosine_topk(Q, Gm[a:b], k, idx_base=a) for a, b in zip(bounds[:-1], bounds[1:])]
    S, I = np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])
    want_s, want_i = O.topk_merge(S, I)
    np.testing.assert_array_equal(want_i, O.cosine_topk(Q, Gm, k)[1])
    for off in (0, 1):
        ins = [G.in_f32(S, 4096, off), G.in_i64(I, 4096, off)]
        ts, ti = _topk_outputs(M, k, off)
        _ok(L.isx_topk_merge(ins[0].ptr, ins[1].ptr, P, M, k, ts.ptr, ti.ptr, st), off)
        G.assert_clean([ts, ti], ins, off)
        G.assert_bits(ts, want_s, off)
        np.testing.assert_array_equal(ti.host(), want_i)


# ---- isx_rank_full, isx_average_precision, isx_average_precision_sim ----------------------------------------------------------------------------
def _rank_case(M, N):
    rng = np.random.default_rng(N)
    sim = (np.round(rng.random((M, N)) * 50) / 50).astype(F) if N < 100 else rng.standard_normal((M, N), dtype=F)
    if N > 10:
        sim[:, 7] = sim[:, 2]
    return sim


def _rank(sim, off=0):
    L, st = _lib()
    M, N = sim.shape
    gs = G.in_f32(sim, 4096, off)
    nbytes = L.isx_rank_full_workspace(M, N)
    ws = G.workspace(nbytes)
    ranked = G.out_i64((M, N), max(4096, N), off)             # N padded to a power of two: fewer than N slots past the end of a row
    _ok(L.isx_rank_full(gs.ptr, M, N, ranked.ptr, ws.ptr, nbytes, st), "isx_rank_full")
    G.assert_clean([ranked], [gs])
    assert ws.guards_intact(), "store outside the workspace"
    return ranked


@pytest.mark.parametrize("M,N", [(1, 1), (5, 24), (3, 4096), (4, 4097), (2, 70000)])
def test_rank_full(M, N):
    """One LDS sort (N <= 4096 after padding) and the global bitonic network above it; N = 4097 pads to 8192, 70 000 to 131 072: the padded
    slots must land neither behind `ranked` nor behind the workspace of exactly isx_rank_full_workspace(M, N) bytes."""
    sim = _rank_case(M, N)
    want = O.rank_full(sim)
    for off in (0, 1):
        np.testing.assert_array_equal(_rank(sim, off).host(), want)


@pytest.mark.parametrize("M,N", [(5, 24), (4, 4097)])
def test_average_precision(M, N):
    L, st = _lib()
    sim = _rank_case(M, N)
    want_ranked = O.rank_full(sim)
    Lb = max(1, N // 10)
    gl = (np.arange(N) % Lb).astype(np.int32)
    ql = (np.arange(M) % (Lb + 1)).astype(np.int32)
    ql[M - 1] = Lb                                           # a label absent from the gallery: NaN
    wants = {kth: O.average_precision(want_ranked, ql, gl, kth) for kth in (1, 2, 3)}
    # (sim | ranked, labels, ap) offsets.  N = 24: the float4 instance of the sort-free kernel when sim AND glab are on the boundary, the scalar
    # one with N % 4 == 0 when either is off it; N = 4097: scalar throughout
    for osrc, olab, oout in ((0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        ranked = G.in_i64(want_ranked, 4096, osrc)
        gsim, gq, gg = G.in_f32(sim, 4096, osrc), G.in_i32(ql, 1024, olab), G.in_i32(gl, 4096, olab)
        for kth in (1, 2, 3):
            want = wants[kth]
            assert np.isnan(want[M - 1]) and not np.isnan(want).all()
            for name in ("isx_average_precision", "isx_average_precision_sim"):
                what = (name, kth, "offsets", osrc, olab, oout)
                ap = G.out_f64((M,), 1024, oout)
                src = ranked if name == "isx_average_precision" else gsim
                _ok(getattr(L, name)(src.ptr, M, N, gq.ptr, gg.ptr, kth, ap.ptr, st), what)
                G.assert_clean([ap], [gsim, gq, gg, ranked], what)
                got = ap.host()
                np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
                ok = ~np.isnan(want)
                G.assert_bits(got[ok], want[ok], what)


# ---- isx_masked_sums --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(1, 1), (20, 777), (3, 4097)])
def test_masked_sums_every_row(M, N):
    """Every one of the 2 M outputs against math.fsum of the same fp32 values.  The bound N 2^-52 sum_j |sim_ij| follows from N float64 adds
    in ANY order (each rounds by at most 2^-53 of a partial sum that never exceeds sum_j |sim_ij|): it is not a measured tolerance."""
    L, st = _lib()
    rng = np.random.default_rng(N + M)
    sim = rng.standard_normal((M, N), dtype=F)
    nlab = 5
    gl = (np.arange(N) % nlab).astype(np.int32)
    ql = (np.arange(M) % nlab).astype(np.int32)
    ql[M - 1] = nlab                                         # absent from the gallery: the masked sum is empty
    rows = [[float(v) for v in sim[i]] for i in range(M)]
    refs = [(N * 2.0 ** -52 * math.fsum(abs(v) for v in row), math.fsum(v for v, l in zip(row, gl) if l == ql[i]), math.fsum(row)) for i, row in enumerate(rows)]
    for off in (0, 1):
        ins = [G.in_f32(sim, 4096, off), G.in_i32(ql, 1024, off), G.in_i32(gl, 4096, off)]
        out = G.out_f64((M, 2), 1024, off)
        _ok(L.isx_masked_sums(ins[0].ptr, M, N, ins[1].ptr, ins[2].ptr, out.ptr, st), off)
        G.assert_clean([out], ins, off)
        got = out.host()
        for i, (bound, pos, allv) in enumerate(refs):
            assert abs(got[i, 0] - pos) <= bound and abs(got[i, 1] - allv) <= bound, (off, i, got[i].tolist(), pos, allv, bound)
        assert got[M - 1, 0] == 0.0
