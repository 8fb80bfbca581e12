"""The kernels of the siamese training step (csrc/train.hip: negative mining, triplet loss forward, backward, all leaves in one launch) pinned to
their documented sums and decisions, BIT FOR BIT, through the C ABI: every comparison of a result is array_equal / torch.equal -- on the bit
patterns, so that a zero of the wrong sign shows -- against tests/_triplet_model.py (unfused numpy float32 arithmetic in the kernels' order).
tests/test_triplet_model.py shows that the model is the operation (float64, the oracle, the reference's CPU mining) and that, on the data used
here, another order of the sum, a fused or factored term, `>=` at the clamp, a scale applied in two steps, another tie rule or a wrong reading of
a row block would change the bits.  The shapes are the smallest that reach each path and boundary (lists in _triplet_model.py).

Every output is a body of NaN (int64: a poison value) between guards of 256 sentinels; the guards are checked after every launch."""
import functools

import numpy as np
import pytest
import torch

import _triplet_model as model

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = -12345.0
NAN = float("nan")
GUARD = 256
POISON = -(1 << 62)
FORMS = pytest.mark.parametrize("normalized", [True, False], ids=["normalized", "distance"])


def _lib():
    from isx._lib import check, lib
    return lib(), check, torch.cuda.current_stream().cuda_stream


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.array(a, dtype=dtype)).cuda()               # a copy: the shared cases stay read-only


def _guarded(*shape):
    """(buffer, body): GUARD floats of the sentinel, the body of `shape` filled with NaN, GUARD floats of the sentinel."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    buf[GUARD:GUARD + n] = NAN
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guarded_i64(n):
    buf = torch.full((n + 2 * GUARD,), int(SENTINEL), device="cuda", dtype=torch.int64)
    buf[GUARD:GUARD + n] = POISON
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf):
    s = int(SENTINEL) if buf.dtype == torch.int64 else SENTINEL
    return bool((buf[:GUARD] == s).all()) and bool((buf[-GUARD:] == s).all())


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def _assert_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


# ---- isx_triplet_loss_fwd ---------------------------------------------------------------------------------------------------------------------
def _fwd(a, p, n, margin, normalized):
    L, check, st = _lib()
    B, D = a.shape
    buf, rows = _guarded(B)
    check(L.isx_triplet_loss_fwd(a.data_ptr(), p.data_ptr(), n.data_ptr(), B, D, margin, 1 if normalized else 0, rows.data_ptr(), st), "isx_triplet_loss_fwd")
    assert _guards_intact(buf)
    return rows


@FORMS
@pytest.mark.parametrize("B,D", model.ROW_CASES)
def test_triplet_forward_is_the_lane_and_butterfly_sum(B, D, normalized):
    a, p, n = model.row_case(B, D)
    da, dp, dn = _dev(a), _dev(p), _dev(n)
    for margin in model.margins(B):
        want = model.loss_rows(a, p, n, margin, normalized)
        assert B == 1 or ((want == 0).any() and (want > 0).any())
        _assert_bits(_fwd(da, dp, dn, margin, normalized), want, ("loss_rows", margin))


@FORMS
def test_triplet_forward_at_margin_zero_gives_plus_zero_where_n_is_p(normalized):
    a, p, n = model.margin_zero_case()
    want = model.loss_rows(a, p, n, 0.0, normalized)
    got = _fwd(_dev(a), _dev(p), _dev(n), 0.0, normalized)
    _assert_bits(got, want, "loss_rows")
    assert _bits(got.cpu().numpy())[1] == 0 and want[3] > 0


def test_triplet_forward_halves_after_adding_the_margin():
    """(s + 2 margin) * 0.5 among the denormals, the only place where it is another function than s * 0.5 + margin."""
    a, p, n, margin = model.denormal_case()
    want = model.loss_rows(a, p, n, margin, False)
    assert float(want[0]) == 2 * np.ldexp(1.0, -149)
    _assert_bits(_fwd(_dev(a), _dev(p), _dev(n), margin, False), want, "loss_rows")


# ---- isx_triplet_loss_bwd / isx_triplet_loss_bwd_dev ----------------------------------------------------------------------------------------------
def _bwd(a, p, n, rows, scale, normalized, scale_dev=None):
    L, check, st = _lib()
    B, D = a.shape
    outs = [_guarded(B, D) for _ in range(3)]
    ptrs = [o[1].data_ptr() for o in outs]
    if scale_dev is None:
        check(L.isx_triplet_loss_bwd(a.data_ptr(), p.data_ptr(), n.data_ptr(), rows.data_ptr(), B, D, scale, 1 if normalized else 0, ptrs[0], ptrs[1], ptrs[2], st),
              "isx_triplet_loss_bwd")
    else:
        check(L.isx_triplet_loss_bwd_dev(a.data_ptr(), p.data_ptr(), n.data_ptr(), rows.data_ptr(), B, D, scale, scale_dev.data_ptr(), 1 if normalized else 0,
                                         ptrs[0], ptrs[1], ptrs[2], st), "isx_triplet_loss_bwd_dev")
    assert all(_guards_intact(o[0]) for o in outs)
    return [o[1] for o in outs]


def _check_backward(a, p, n, rows, normalized):
    """Both entries on the same data, ALL rows, the mask being the model's (rows > 0): the host scale 1 / B, and 1 / B times the device scalar."""
    B = a.shape[0]
    da, dp, dn, dr = _dev(a), _dev(p), _dev(n), _dev(rows)
    sd = _dev([model.SCALE_DEV])
    for entry, got, scale in (("isx_triplet_loss_bwd", _bwd(da, dp, dn, dr, 1.0 / B, normalized), model.scale_host(1.0 / B)),
                              ("isx_triplet_loss_bwd_dev", _bwd(da, dp, dn, dr, 1.0 / B, normalized, sd), model.scale_dev(1.0 / B, model.SCALE_DEV))):
        want = model.grads(a, p, n, rows, scale, normalized)
        for name, g, w in zip(("g_anchor", "g_pos", "g_neg"), got, want):
            _assert_bits(g, w, (entry, name))


@FORMS
@pytest.mark.parametrize("B,D", model.ROW_CASES)
def test_triplet_backward_is_the_unfused_formula_on_all_rows(B, D, normalized):
    a, p, n = model.row_case(B, D)
    for margin in model.margins(B):
        _check_backward(a, p, n, model.loss_rows(a, p, n, margin, normalized), normalized)


@FORMS
def test_triplet_backward_gives_the_row_with_zero_loss_no_gradient(normalized):
    a, p, n = model.margin_zero_case()
    rows = model.loss_rows(a, p, n, 0.0, normalized)
    assert _bits(rows)[1] == 0
    _check_backward(a, p, n, rows, normalized)


@FORMS
@pytest.mark.parametrize("B,D", model.BWD_PAST_CAP)
def test_triplet_backward_past_the_grid_cap(B, D, normalized):
    """More than 4096 x 256 elements: the grid-stride loop takes its second sweep, b = i / D past it."""
    a, p, n = model.row_case(B, D)
    rows = model.loss_rows(a, p, n, model.MARGIN, normalized)
    assert (rows[-(B * D - 4096 * 256) // D - 1:] > 0).any() and (rows == 0).any()          # active rows inside the second sweep
    _check_backward(a, p, n, rows, normalized)


@FORMS
def test_triplet_backward_decides_on_loss_rows_above_zero(normalized):
    """Hand-made loss_rows: -0, +0 and the negative numbers are off, the smallest denormal is on -- whatever the forward kernel would have given."""
    a, p, n = model.row_case(7, 100)
    tiny = np.ldexp(1.0, -149)
    rows = np.array([-0.0, 0.0, tiny, 1.0, -tiny, np.ldexp(1.0, -126), -1.0], F)
    assert [bool(r > 0) for r in rows] == [False, False, True, True, False, True, False]
    _check_backward(a, p, n, rows, normalized)


# ---- isx_triplet_leaves -----------------------------------------------------------------------------------------------------------------------
def _leaves(d, L, k, D, margin, normalized, sa, sb):
    lib, check, st = _lib()
    lbuf, loss = _guarded(L)
    dbuf, dd = _guarded(L * 3 * k, D)
    check(lib.isx_triplet_leaves(d.data_ptr(), L, k, D, margin, 1 if normalized else 0, sa, sb, loss.data_ptr(), dd.data_ptr(), st), "isx_triplet_leaves")
    assert _guards_intact(lbuf) and _guards_intact(dbuf)
    return loss, dd


@pytest.mark.parametrize("avg", [True, False], ids=["mean", "sum"])
@FORMS
@pytest.mark.parametrize("L,k,D", model.LEAF_CASES)
def test_triplet_leaves_are_the_row_kernels_leaf_by_leaf(L, k, D, normalized, avg):
    """dd and loss_leaf against the model; L leaves in one launch against the same leaves one by one; the leaf loss against the TripletLoss module's
    value (before its `* share`) that it replaces in the log: both are fp32 sums of the same k non-negative rows in different orders -- 2 (k - 1)
    roundings -- and the mean's `/ k` is one more: |difference| <= (2 (k - 1) + 1) * 2^-24 * sum(rows) [/ k]."""
    from model.custom_modules import TripletLoss
    d = model.leaf_case(L, k, D)
    sa, sb = model.leaf_scales(L, k, avg)
    want_loss, want_dd, rows = model.leaves(d, L, k, model.MARGIN, normalized, sa, sb)
    dev = _dev(d)
    loss, dd = _leaves(dev, L, k, D, model.MARGIN, normalized, sa, sb)
    _assert_bits(dd, want_dd, "dd")
    _assert_bits(loss, want_loss, "loss_leaf")
    for l in range(L):
        leaf = dev[3 * k * l:3 * k * (l + 1)]
        if L > 1:
            loss1, dd1 = _leaves(leaf.clone(), 1, k, D, model.MARGIN, normalized, sa, sb)
            assert torch.equal(loss1.view(torch.int32), loss[l:l + 1].view(torch.int32)) and torch.equal(dd1.view(torch.int32), dd[3 * k * l:3 * k * (l + 1)].view(torch.int32)), l
        module = float(TripletLoss(model.MARGIN, avg, normalized)(leaf[:k], leaf[k:2 * k], leaf[2 * k:]))
        total = float(rows[l].astype(np.float64).sum())
        mine, bound = float(want_loss[l]), (2 * (k - 1) + 1) * model.U * total
        if avg:
            mine, bound = mine / k, bound / k
        assert abs(module - mine) <= bound, (l, module, mine, bound)


# ---- isx_mine_negatives / isx_mine_negatives_rows -----------------------------------------------------------------------------------------------
def _mine(sim_ptr, N, lab, i1, i2, semi, block=None):
    """block = (row_base, rows): isx_mine_negatives_rows on the rows behind sim_ptr; None: the whole matrix."""
    L, check, st = _lib()
    n = int(i1.numel())
    buf, neg = _guarded_i64(n)
    if block is None:
        check(L.isx_mine_negatives(sim_ptr, N, lab.data_ptr(), i1.data_ptr(), i2.data_ptr(), n, semi, neg.data_ptr(), st), "isx_mine_negatives")
    else:
        check(L.isx_mine_negatives_rows(sim_ptr, N, block[0], block[1], lab.data_ptr(), i1.data_ptr(), i2.data_ptr(), n, semi, neg.data_ptr(), st),
              "isx_mine_negatives_rows")
    assert _guards_intact(buf)
    return neg.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _mine_dev(N):
    c = model.mine_case(N)
    return _dev(c.sim), _dev(c.labels, np.int32), _dev(c.labels_one, np.int32)


@pytest.mark.parametrize("semi", [1, 0], ids=["semi_hard", "hard"])
@pytest.mark.parametrize("N", model.MINE_N)
def test_mining_on_the_whole_matrix(N, semi):
    """Every named case: ties in different waves, s == sim_pos, nothing left, signed zeros, infinities, i1 == i2, unsorted couples; one label for
    all gives -1 everywhere."""
    c = model.mine_case(N)
    sim, lab, lab_one = _mine_dev(N)
    for name, (i1, i2) in sorted(c.couples.items()):
        got = _mine(sim.data_ptr(), N, lab, _dev(i1, np.int64), _dev(i2, np.int64), semi)
        assert np.array_equal(got, model.mine_expect(N, semi)[name]), name
    i1, i2, _ = model.all_couples(c)
    got = _mine(sim.data_ptr(), N, lab_one, _dev(i1, np.int64), _dev(i2, np.int64), semi)
    assert np.array_equal(got, model.mine(c.sim, N, 0, c.labels_one, i1, i2, semi)) and (got == -1).all()


@pytest.mark.parametrize("semi", [1, 0], ids=["semi_hard", "hard"])
def test_mining_on_the_golden_matrix(golden, semi):
    g = golden("training.npz")
    sim, lab, i1, i2 = g["mine_sim"], g["mine_labels"], g["mine_i1"], g["mine_i2"]
    N = sim.shape[0]
    dsim = _dev(sim)
    got = _mine(dsim.data_ptr(), N, _dev(lab, np.int32), _dev(i1, np.int64), _dev(i2, np.int64), semi)
    assert np.array_equal(got, model.mine(sim, N, 0, lab, i1, i2, semi)) and np.array_equal(got, g["neg_semi%d" % semi])


@pytest.mark.parametrize("semi", [1, 0], ids=["semi_hard", "hard"])
@pytest.mark.parametrize("N", [n for n in model.MINE_N if n >= 5])
def test_mining_on_row_blocks(N, semi):
    """A single first row, 7 rows at row_base 1, the last third, everything: the couples whose anchor falls in the block, shuffled, on a COPY of the
    block with a block's worth of rows of 3.0 on either side -- the model's answer, and the whole-matrix kernel's for the same couples."""
    c = model.mine_case(N)
    sim, lab, _ = _mine_dev(N)
    i1, i2, _ = model.all_couples(c)
    rng = np.random.default_rng(N + semi)
    for r0, r1 in model.blocks(N):
        sel = rng.permutation(np.flatnonzero((i1 >= r0) & (i1 < r1)))
        assert len(sel), (r0, r1)
        a, b = _dev(i1[sel], np.int64), _dev(i2[sel], np.int64)
        buf, pad = model.slab(c.sim, r0, r1)
        dbuf = _dev(buf)
        got = _mine(dbuf[pad:].data_ptr(), N, lab, a, b, semi, block=(r0, r1 - r0))
        assert np.array_equal(got, model.mine(c.sim[r0:r1], N, r0, c.labels, i1[sel], i2[sel], semi)), (r0, r1)
        assert np.array_equal(got, _mine(sim.data_ptr(), N, lab, a, b, semi)), (r0, r1)
        assert bool((dbuf[:pad] == model.PAD_SCORE).all()) and bool((dbuf[2 * pad:] == model.PAD_SCORE).all())


def test_mining_wrapper_refuses_an_anchor_outside_the_block():
    from isx import ops
    from isx._lib import IsxError
    N = 257
    sim, lab, _ = _mine_dev(N)
    for i1 in ([3, 10], [2, 3]):
        with pytest.raises(IsxError):
            ops.mine_negatives(sim[3:10].contiguous(), lab, _dev(i1, np.int64), _dev([3, 3], np.int64), 1, row_base=3)
    got = ops.mine_negatives(sim[3:10].contiguous(), lab, _dev([3, 9], np.int64), _dev([10, 16], np.int64), 0, row_base=3)
    c = model.mine_case(N)
    assert np.array_equal(got.cpu().numpy(), model.mine(c.sim, N, 0, c.labels, [3, 9], [10, 16], 0))


@pytest.mark.parametrize("semi", [True, False], ids=["semi_hard", "hard"])
@pytest.mark.parametrize("N", [100, 257])
def test_epoch_mining_over_budget_takes_the_row_blocks(N, semi):
    """train.siamese_descriptor.mine_epoch_negatives with the matrix over budget (SimilarityRows: 9-row blocks computed on demand) against the
    same function on the whole isx_cosine_sim matrix, and against the model on the host copy of that matrix."""
    import utils.metrics as M
    from isx import ops
    from train.siamese_descriptor import mine_epoch_negatives
    from utils.train_siamese import SimilarityRows
    c = model.mine_case(N)
    i1, i2, _ = model.all_couples(c)
    ds = [(None, int(l), None) for l in c.labels]
    couples = [(int(c.labels[a]), (int(a), int(b)), (None, None)) for a, b in zip(i1, i2)]
    E = _dev(c.E)
    full = ops.cosine_sim(E, E)
    old = M.SIM_BUDGET_BYTES
    try:
        M.SIM_BUDGET_BYTES = 4 * N * 9
        assert len(M.row_blocks(N, N)) == (N + 8) // 9
        blocked = mine_epoch_negatives(SimilarityRows(E), ds, couples, semi)
    finally:
        M.SIM_BUDGET_BYTES = old
    whole = mine_epoch_negatives(full, ds, couples, semi)
    assert torch.equal(blocked, whole)
    assert np.array_equal(whole.numpy(), model.mine(full.cpu().numpy(), N, 0, c.labels, i1, i2, semi))


# ---- empty problems ---------------------------------------------------------------------------------------------------------------------------
def test_empty_problems_launch_nothing():
    L, check, st = _lib()
    x = torch.zeros((4, 8), device="cuda")
    lab = torch.zeros((4,), device="cuda", dtype=torch.int32)
    idx = torch.zeros((4,), device="cuda", dtype=torch.int64)
    ibuf, neg = _guarded_i64(4)
    check(L.isx_mine_negatives(x.data_ptr(), 4, lab.data_ptr(), idx.data_ptr(), idx.data_ptr(), 0, 1, neg.data_ptr(), st), "isx_mine_negatives")
    check(L.isx_mine_negatives_rows(x.data_ptr(), 4, 1, 2, lab.data_ptr(), idx.data_ptr(), idx.data_ptr(), 0, 1, neg.data_ptr(), st), "isx_mine_negatives_rows")
    outs = [_guarded(4, 8) for _ in range(4)]
    o = [b[1].data_ptr() for b in outs]
    sd = torch.ones((1,), device="cuda")
    check(L.isx_triplet_loss_fwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), 0, 8, 0.1, 1, o[0], st), "isx_triplet_loss_fwd")
    check(L.isx_triplet_loss_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 0, 8, 1.0, 1, o[1], o[2], o[3], st), "isx_triplet_loss_bwd")
    check(L.isx_triplet_loss_bwd_dev(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 0, 8, 1.0, sd.data_ptr(), 1, o[1], o[2], o[3], st), "isx_triplet_loss_bwd_dev")
    check(L.isx_triplet_leaves(x.data_ptr(), 0, 1, 8, 0.1, 1, 1.0, 1.0, o[0], o[1], st), "isx_triplet_leaves")
    torch.cuda.synchronize()
    assert _guards_intact(ibuf) and bool((neg == POISON).all())
    for buf, body in outs:
        assert _guards_intact(buf) and bool(torch.isnan(body).all())
