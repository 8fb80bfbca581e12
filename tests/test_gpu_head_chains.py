"""The descriptor head's training kernels (csrc/head.hip, the FOLD path of csrc/wgrad_kernel.hpp) pinned to their documented sums, BIT FOR BIT,
through the C ABI: every comparison is array_equal / torch.equal against tests/_head_model.py (oracle.cosine_sim's k-ordered fmaf chains and
unfused numpy float32 arithmetic).  tests/test_head_model.py shows that the model is the operation (float64) and that, on the data used here,
a cut at another boundary, another order of the partials, groups of another size, another order of the rows or an optimizer term in another
place would change the bits.  The shapes are the smallest that reach each launch variant and each boundary (lists in _head_model.py)."""
import functools

import numpy as np
import pytest
import torch

import _head_model as model

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
NAN = float("nan")


def _lib():
    from isx._lib import check, lib
    return lib(), check, torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()          # a copy: the shared cases stay read-only


def _host(t):
    return t.cpu().numpy()


def _guarded(rows, cols):
    """(rows + 2, cols) of the sentinel; the kernel gets rows [1, rows + 1)."""
    return torch.full((rows + 2, cols), SENTINEL, device="cuda")


def _guards_intact(buf):
    return bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all())


def _pad64(m):
    return (m + 63) // 64 * 64


def test_split_and_group_rules_are_the_librarys():
    L = _lib()[0]
    for K in model.FWD_K + (model.FWD_CAP[2], 2048, 4064, 4096, 65536, 67584, 100352):
        assert model.splits(K)[0] == L.isx_head_linear_splits(K), K
    for N in sorted({n for n, _ in model.DGRAD_NK} | set(model.FWD_N) | {64, 128, 2048, 480}):
        assert model.groups(N) == L.isx_head_groups(N), N


# ---- isx_head_linear_fwd / isx_head_linear_fwd_rows -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fwd_dev(K):
    x, w, bias = model.fwd_case(K)[:3]
    return _dev(x), _dev(w), _dev(bias)


def _fwd_transposed(x, w, b):
    """isx_head_linear_fwd on x transposed; the padding columns M .. Mp-1 hold 1e30 ("any finite values"), the workspace NaN."""
    L, check, st = _lib()
    (M, K), N = x.shape, w.shape[0]
    Mp = _pad64(M)
    xT = torch.full((K, Mp), 1e30, device="cuda")
    xT[:, :M] = x.t()
    ws = torch.full((L.isx_head_linear_splits(K) * Mp * N,), NAN, device="cuda")
    buf = _guarded(M, N)
    check(L.isx_head_linear_fwd(xT.data_ptr(), M, Mp, K, w.data_ptr(), N, b.data_ptr() if b is not None else None, buf[1:].data_ptr(), ws.data_ptr(),
                                ws.numel() * 4, st), "isx_head_linear_fwd")
    assert _guards_intact(buf)
    return buf[1:M + 1]


def _fwd_rows(x, w, b):
    L, check, st = _lib()
    (M, K), N = x.shape, w.shape[0]
    nbytes = L.isx_head_linear_rows_workspace(M, K, N)
    assert nbytes % 4 == 0 and nbytes >= L.isx_head_linear_splits(K) * M * N * 4
    ws = torch.full((nbytes // 4,), NAN, device="cuda")
    buf = _guarded(M, N)
    check(L.isx_head_linear_fwd_rows(x.data_ptr(), M, K, w.data_ptr(), N, b.data_ptr() if b is not None else None, buf[1:].data_ptr(), ws.data_ptr(),
                                     nbytes, st), "isx_head_linear_fwd_rows")
    assert _guards_intact(buf)
    return buf[1:M + 1]


def _check_forward(M, N, K, with_bias):
    L = _lib()[0]
    assert model.splits(K)[0] == L.isx_head_linear_splits(K)
    bias_np, y = model.fwd_case(K)[2], model.fwd_case(K)[4]
    want = y[:M, :N] + bias_np[None, :N] if with_bias else y[:M, :N]
    X, W, B = _fwd_dev(K)
    x, w, b = X[:M].clone(), W[:N].clone(), (B[:N].clone() if with_bias else None)     # clones: nothing of the larger case lies behind the rows
    got_t, got_r = _fwd_transposed(x, w, b), _fwd_rows(x, w, b)
    for entry, got in (("isx_head_linear_fwd", got_t), ("isx_head_linear_fwd_rows", got_r)):
        g = _host(got)
        assert np.array_equal(g, want), (entry, int((g != want).sum()), float(np.abs(g - want).max()))
    assert torch.equal(got_t, got_r)


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("M", model.FWD_M)
@pytest.mark.parametrize("N", model.FWD_N)
@pytest.mark.parametrize("K", model.FWD_K)
def test_head_linear_forward_is_the_split_chain(K, N, M, with_bias):
    """y = ((p_0 + p_1) + ...) + bias with p_s the chain over the k of split s (model.splits): both entries, on the same data, against the
    model and against each other.  Both entries run at every M: the transposed one reaches TM = 1 with several row tiles at M = 193 and 320, the
    row-major one two 192-row tiles there."""
    _check_forward(M, N, K, with_bias)


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
def test_head_linear_forward_at_the_cap_of_32_splits(with_bias):
    M, N, K = model.FWD_CAP
    S, kt_per, ranges = model.splits(K)
    assert (S, kt_per, (ranges[-1][1] - ranges[-1][0]) // 32) == (32, 67, 40)
    _check_forward(M, N, K, with_bias)


# ---- isx_head_linear_dgrad / isx_head_linear_dgrad_parts ------------------------------------------------------------------------------------
def _dyT(dy):
    M, N = dy.shape
    t = torch.zeros((N, _pad64(M)), device="cuda")
    t[:, :M] = _dev(dy).t()
    return t


def _dgrad(dyT, w, K):
    L, check, st = _lib()
    N, Mp = dyT.shape
    buf = _guarded(Mp, K)
    check(L.isx_head_linear_dgrad(dyT.data_ptr(), Mp, N, w.data_ptr(), K, buf[1:].data_ptr(), st), "isx_head_linear_dgrad")
    assert _guards_intact(buf)
    return buf[1:Mp + 1]


def _dgrad_parts(dyT, w, Ng, groups, K):
    L, check, st = _lib()
    Mp = dyT.shape[1]
    assert dyT.shape[0] == w.shape[0] == Ng * groups and dyT.is_contiguous() and w.is_contiguous()
    buf = _guarded(groups * Mp, K)
    check(L.isx_head_linear_dgrad_parts(dyT.data_ptr(), Mp, Ng, groups, w.data_ptr(), K, buf[1:].data_ptr(), st), "isx_head_linear_dgrad_parts")
    assert _guards_intact(buf)
    return buf[1:groups * Mp + 1].view(groups, Mp, K)


@pytest.mark.parametrize("N,K,M", model.DGRAD_CASES)
def test_head_dgrad_is_the_fold_of_its_group_chains(N, K, M):
    """dx = ((0 + c_0) + c_1) + ... over isx_head_groups(N) groups; the rows past M of the zero-padded dy^T come out zero."""
    dy, w, _, want = model.dgrad_case(N, K, M)
    assert model.groups(N) == _lib()[0].isx_head_groups(N)
    got = _host(_dgrad(_dyT(dy), _dev(w), K))
    assert np.array_equal(got[:M], want), (int((got[:M] != want).sum()), float(np.abs(got[:M] - want).max()))
    assert not got[M:].any()


@pytest.mark.parametrize("N,K,M", [c for c in model.DGRAD_CASES if model.groups(c[0]) == 8])
def test_head_dgrad_parts_are_the_group_chains_and_add_up_to_dgrad(N, K, M):
    """parts[g] = the chain of group g; a rank's call on ITS slice of dy^T and w (P = 2, 4, 8) gives the bits of those groups in the full call;
    ShardedHead.backward's sum of the pieces (pieces[0].clone(), += in order) is isx_head_linear_dgrad's result on the same data."""
    dy, w, want_parts, want = model.dgrad_case(N, K, M)
    Ng = N // 8
    dyT, wd = _dyT(dy), _dev(w)
    full = _dgrad_parts(dyT, wd, Ng, 8, K)
    got = _host(full)
    for g in range(8):
        assert np.array_equal(got[g, :M], want_parts[g]), (g, int((got[g, :M] != want_parts[g]).sum()))
    assert not got[:, M:].any()
    for P in (2, 4, 8):
        per = 8 // P
        for r in range(P):
            mine = _dgrad_parts(dyT[r * per * Ng:(r + 1) * per * Ng], wd[r * per * Ng:(r + 1) * per * Ng], Ng, per, K)
            assert torch.equal(mine, full[r * per:(r + 1) * per]), (P, r)
    dx = full[0].clone()
    for g in range(1, 8):
        dx += full[g]
    assert torch.equal(dx, _dgrad(dyT, wd, K))
    assert np.array_equal(_host(dx)[:M], want)


def test_head_dgrad_parts_of_five_groups_of_96():
    Ng, G, K, M = model.PARTS_EXTRA
    dy, w, want = model.parts_extra_case()
    got = _host(_dgrad_parts(_dyT(dy), _dev(w), Ng, G, K))
    for g in range(G):
        assert np.array_equal(got[g, :M], want[g]), g
    assert not got[:, M:].any()


# ---- isx_head_sgd_step ----------------------------------------------------------------------------------------------------------------------
def _sgd(dy, x, R, N, K, w, mom, first, lr, momentum, dampening, weight_decay, nesterov):
    L, check, st = _lib()
    check(L.isx_head_sgd_step(dy.data_ptr() if dy is not None else None, x.data_ptr() if x is not None else None, R, N, K, w.data_ptr(),
                              mom.data_ptr() if mom is not None else None, first, lr, momentum, dampening, weight_decay, nesterov, st), "isx_head_sgd_step")


@pytest.mark.parametrize("N,K", model.SGD_NK)
@pytest.mark.parametrize("R", model.SGD_R)
def test_head_sgd_gradient_is_one_chain_over_the_rows(N, K, R):
    """w = 0, lr = -1, no momentum, no decay: w - lr * g = 0 + g, the weight gradient itself.  R = 0: null dy and x, a zero gradient."""
    dy, x, want = model.rows_case(N, K, R)
    w = torch.zeros((N, K), device="cuda")
    _sgd(_dev(dy) if R else None, _dev(x) if R else None, R, N, K, w, None, 1, -1.0, 0.0, 0.0, 0.0, 0)
    got = _host(w)
    assert np.array_equal(got, want), (int((got != want).sum()), float(np.abs(got - want).max()))


@pytest.mark.parametrize("hyper", model.SGD_SETS, ids=[s[0] for s in model.SGD_SETS])
@pytest.mark.parametrize("N,K,R", model.SGD_UPDATE_NKR)
def test_head_sgd_update_is_the_unfused_fp32_formula(N, K, R, hyper):
    """Three consecutive steps (first = 1, 0, 0) against model.sgd_step on the model's gradient: w and the momentum buffer after every step.  The
    buffer starts as NaN: the first step must not read it."""
    _, lr, mom, damp, wd, nest = hyper
    w_np, buf_np = model.sgd_w0(N, K), None
    w = _dev(w_np)
    buf = torch.full((N, K), NAN, device="cuda") if mom else None
    for step in range(3):
        dy, x, g = model.rows_case(N, K, R, seed=step)
        _sgd(_dev(dy), _dev(x), R, N, K, w, buf, 1 if step == 0 else 0, lr, mom, damp, wd, nest)
        w_np, buf_np = model.sgd_step(w_np, buf_np, g, step == 0, lr, mom, damp, wd, nest)
        got = _host(w)
        assert np.array_equal(got, w_np), ("w", step, int((got != w_np).sum()), float(np.abs(got - w_np).max()))
        if mom:
            got = _host(buf)
            assert np.array_equal(got, buf_np), ("momentum", step, int((got != buf_np).sum()), float(np.abs(got - buf_np).max()))


def test_head_sgd_step_on_a_shard_leaves_the_other_rows_alone():
    """Rows [64, 128) of a (192, K) weight and momentum, called as isx/shard_head.py sgd_update_rows calls it (the row slices' pointers, N = 64,
    dy = this shard's columns made contiguous): the shard's rows are the model's, all other rows keep their bits."""
    lo, hi, N, K, R = 64, 128, 192, 128, 24
    _, lr, mom, damp, wd, nest = model.SGD_SETS[3]
    w_np = model.sgd_w0(N, K)
    buf_np = model.inputs(N, K, 6, special_rows=False)
    w, buf = _dev(w_np), _dev(buf_np)
    w0, buf0 = w.clone(), buf.clone()
    ws_np, bs_np = w_np[lo:hi], None
    for step in range(2):
        dy, x, _ = model.rows_case(N, K, R, seed=step)
        dY = _dev(dy)[:, lo:hi].contiguous()
        _sgd(dY, _dev(x), R, hi - lo, K, w[lo:hi], buf[lo:hi], 1 if step == 0 else 0, lr, mom, damp, wd, nest)
        ws_np, bs_np = model.sgd_step(ws_np, bs_np, model.wgrad_rows(dy[:, lo:hi], x), step == 0, lr, mom, damp, wd, nest)
        assert np.array_equal(_host(w[lo:hi]), ws_np) and np.array_equal(_host(buf[lo:hi]), bs_np), step
        for t, t0 in ((w, w0), (buf, buf0)):
            assert torch.equal(t[:lo].view(torch.int32), t0[:lo].view(torch.int32)) and torch.equal(t[hi:].view(torch.int32), t0[hi:].view(torch.int32)), step


# ---- isx_colsum_leaves ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaves,R,C", model.COLSUM_CASES)
def test_colsum_leaves_adds_the_rows_in_order(leaves, R, C):
    L, check, st = _lib()
    x, want = model.colsum_case(leaves, R, C)
    buf = _guarded(leaves, C)
    xd = _dev(x) if R else None
    check(L.isx_colsum_leaves(xd.data_ptr() if R else None, leaves, R, C, buf[1:].data_ptr(), st), "isx_colsum_leaves")
    assert _guards_intact(buf)
    got = _host(buf[1:leaves + 1])
    assert np.array_equal(got, want)
    if R == 0:
        assert not got.any()
