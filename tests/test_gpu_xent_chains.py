"""The softmax cross-entropy kernels of the classifier tail (csrc/classif.hip: isx_softmax_xent_fwd, isx_softmax_xent_bwd,
isx_softmax_xent_leaves) pinned to their documented sums, BIT FOR BIT, through the C ABI, against tests/_xent_model.py: unfused numpy float32
arithmetic in the kernels' order around the device's own expf and logf, which the model reads through the test hook isx_debug_expf_logf (they
are not correctly rounded; the hook itself is held to the 4 ulps tests/test_gpu_classif.py grants them, a sanity check, not a pin).  A NaN is
compared as a NaN whatever its payload; everything else on the bit patterns, so that a zero of the wrong sign shows.
tests/test_xent_model.py shows that the model is cross-entropy and that, on the data used here, another order of the sum, another grouping of
the loss, a factored probability or a scale applied in two steps would change the bits.  The shapes are the smallest that reach each path (lists
in _xent_model.py).  The tail's two neighbours, isx_linear_wgrad_leaves and isx_gap_bwd_nhwc, follow at their edges.

Every output is a body of NaN between guards of 256 sentinels; the guards are checked after every launch."""
import numpy as np
import pytest
import torch

import _xent_model as model
from test_gpu_triplet_chains import GUARD, _bits, _dev, _guarded, _guards_intact, _lib

pytestmark = pytest.mark.gpu

F = np.float32
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31


def _hook(x, want_exp=True, want_log=True):
    """(expf(x), logf(x)) of the device for a float32 array; None for an output not asked for."""
    L, check, st = _lib()
    x = np.ascontiguousarray(x, F)
    n = x.size
    dx = _dev(x.reshape(-1))
    outs = [_guarded(n) if w else None for w in (want_exp, want_log)]
    check(L.isx_debug_expf_logf(dx.data_ptr(), n, *[o[1].data_ptr() if o else None for o in outs], st), "isx_debug_expf_logf")
    assert all(_guards_intact(o[0]) for o in outs if o)
    return [o[1].cpu().numpy().reshape(x.shape) if o else None for o in outs]


EXP = model.through_unique_bits(lambda d: _hook(d, want_log=False)[0])
LOG = model.through_unique_bits(lambda s: _hook(s, want_exp=False)[1])


def _assert_bits(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    want = np.asarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    bad = (np.isnan(got) != nan) | (~nan & (_bits(got) != _bits(want)))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


def _same_bits(a, b):
    """Two results of the device: the same bits, NaN payloads included."""
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the hook ---------------------------------------------------------------------------------------------------------------------------------------
def test_hook_gives_the_devices_expf_and_logf():
    e, l = _hook(np.array([0.0, -0.0, -np.inf, np.nan, 1.0], F))
    assert _bits(e[:3]).tolist() == [0x3F800000, 0x3F800000, 0] and np.isnan(e[3])         # expf(+-0) = 1, expf(-inf) = +0
    assert _bits(l[4:5])[0] == 0 and np.isnan(l[3]) and np.isnan(l[2]) and np.isneginf(l[0])    # logf(1) = +0
    e_only, none = _hook(np.array([0.0], F), want_log=False)
    assert none is None and e_only[0] == 1
    rng = np.random.default_rng(12)
    xe = np.concatenate([np.linspace(-104, 0, 4001), -rng.random(2000) * 104]).astype(F)
    xl = np.concatenate([np.linspace(1, 2, 1001), 2.0 ** (rng.random(4000) * 24), [2.0 ** 24]]).astype(F)
    ge, gl = _hook(xe, want_log=False)[0], _hook(xl, want_exp=False)[1]
    we, wl = model.exp_ref(xe), model.log_ref(xl)
    # in units of the float32 spacing at the correctly rounded value (among the denormals: 2^-149)
    de = np.abs(ge.astype(np.float64) - we) / np.spacing(np.maximum(np.abs(we), F(2.0 ** -126)))
    dl = np.abs(gl.astype(np.float64) - wl) / np.spacing(np.maximum(np.abs(wl), F(2.0 ** -126)))
    denormal = (we > 0) & (we < 2.0 ** -126)
    print("isx_debug_expf_logf against float64 rounded: expf %.0f ulp over %d arguments in [-104, 0] (%d denormal results, %d of them zero on "
          "the device), logf %.0f ulp over %d arguments in [1, 2^24]" % (de.max(), xe.size, int(denormal.sum()), int((ge[denormal] == 0).sum()), dl.max(), xl.size))
    assert de.max() <= 4 and dl.max() <= 4


# ---- the three entries ------------------------------------------------------------------------------------------------------------------------------
def _fwd(z, y, B, C):
    L, check, st = _lib()
    buf, rows = _guarded(B)
    check(L.isx_softmax_xent_fwd(z.data_ptr(), y.data_ptr(), B, C, rows.data_ptr(), st), "isx_softmax_xent_fwd")
    assert _guards_intact(buf)
    return rows


def _bwd(z, y, B, C, scale, scale_dev=None):
    L, check, st = _lib()
    buf, dz = _guarded(B, C)
    sd = _dev([scale_dev]) if scale_dev is not None else None
    check(L.isx_softmax_xent_bwd(z.data_ptr(), y.data_ptr(), B, C, scale, sd.data_ptr() if sd is not None else None, dz.data_ptr(), st), "isx_softmax_xent_bwd")
    assert _guards_intact(buf)
    return dz


def _leaves(z, y, L_, k, C, sa, sb):
    L, check, st = _lib()
    lbuf, loss = _guarded(L_)
    dbuf, dz = _guarded(L_ * k, C)
    check(L.isx_softmax_xent_leaves(z.data_ptr(), y.data_ptr(), L_, k, C, sa, sb, loss.data_ptr(), dz.data_ptr(), st), "isx_softmax_xent_leaves")
    assert _guards_intact(lbuf) and _guards_intact(dbuf)
    return loss, dz


def _check_rows(z, y):
    """Forward, backward at every scale (host alone, scale_dev alone, both) and the leaves entry (the batch as ONE leaf, and as leaves of one
    row) against the model; every row alone against the same row in its batch."""
    B, C = z.shape
    dz_, dy_ = _dev(z), _dev(y, np.int32)
    m, s = model.row_stats(z, EXP)
    want_rows = model.row_loss(z, y, m, s, LOG)
    rows = _fwd(dz_, dy_, B, C)
    _assert_bits(rows, want_rows, "loss_rows")
    grads = {}
    for a, b in model.SCALES:
        scale = model.scale_of(a, b)
        want = model.row_grad(z, y, m, s, scale, EXP)
        grads[a, b] = _bwd(dz_, dy_, B, C, a, b)
        _assert_bits(grads[a, b], want, ("isx_softmax_xent_bwd", a, b))
        one = 1.0 if b is None else b
        loss1, g1 = _leaves(dz_, dy_, 1, B, C, a, one)                          # one leaf of B rows
        lossB, gB = _leaves(dz_, dy_, B, 1, C, a, one)                          # B leaves of one row
        assert _same_bits(g1, grads[a, b]) and _same_bits(gB, grads[a, b]), (a, b)
        _assert_bits(loss1, model.leaf_losses(want_rows[None, :]), ("loss_leaf, one leaf", a, b))
        _assert_bits(lossB, model.leaf_losses(want_rows[:, None]), ("loss_leaf, leaves of one row", a, b))
    a, b = 0.2, model.SCALE_DEV
    for r in range(B):
        assert _same_bits(_fwd(dz_[r:r + 1].clone(), dy_[r:r + 1].clone(), 1, C), rows[r:r + 1]), r
        assert _same_bits(_bwd(dz_[r:r + 1].clone(), dy_[r:r + 1].clone(), 1, C, a, b), grads[a, b][r:r + 1]), r


@pytest.mark.parametrize("C", model.C_CASES)
def test_rows_of_every_kind_are_the_model(C):
    z, y, _ = model.kind_rows(C)
    _check_rows(z, y)


@pytest.mark.parametrize("C", model.B_CASES_C)
@pytest.mark.parametrize("B", model.B_CASES)
def test_whole_and_ragged_groups_of_four_rows(B, C):
    z, y, _ = model.batch_case(B, C)
    _check_rows(z, y)


@pytest.mark.parametrize("L,k,C", model.LEAF_CASES)
def test_leaves_are_the_row_kernels_leaf_by_leaf(L, k, C):
    """dlogits and loss_leaf against the model; the gradient bits of isx_softmax_xent_bwd with the same product; the leaf loss = the model's
    ordered sum of the rows isx_softmax_xent_fwd gives; every leaf alone against the same leaf among its siblings."""
    z, y = model.leaf_case(L, k, C)
    dz_, dy_ = _dev(z), _dev(y, np.int32)
    rows = _fwd(dz_, dy_, L * k, C)
    for sa, sb in ((1.0 / k, 1.0 / L), (0.2, model.SCALE_DEV)):
        want_loss, want_dz, want_rows = model.leaves(z, y, L, k, sa, sb, EXP, LOG)
        loss, dz = _leaves(dz_, dy_, L, k, C, sa, sb)
        _assert_bits(dz, want_dz, ("dlogits", sa, sb))
        _assert_bits(loss, want_loss, ("loss_leaf", sa, sb))
        _assert_bits(rows, want_rows.reshape(-1), "loss_rows")
        _assert_bits(loss, model.leaf_losses(rows.cpu().numpy().reshape(L, k)), "loss_leaf of the forward entry's rows")
        assert _same_bits(dz, _bwd(dz_, dy_, L * k, C, sa, sb))
        for l in range(L if L > 1 else 0):
            sl = slice(l * k, (l + 1) * k)
            loss1, dz1 = _leaves(dz_[sl].clone(), dy_[sl].clone(), 1, k, C, sa, sb)
            assert _same_bits(loss1, loss[l:l + 1]) and _same_bits(dz1, dz[sl]), l


def test_one_float_off_a_16_byte_boundary():
    """Logits and both outputs one float past an aligned address: the bits of the aligned call."""
    L, check, st = _lib()
    B, C = 5, 129
    z, y, names = model.kind_rows(C)
    pick = [names.index(n) for n in ("spread/max", "spread/else", "ties/else", "masked/min", "masked/else")]     # rows whose sum shows its order
    z, y = np.ascontiguousarray(z[pick]), np.ascontiguousarray(y[pick])
    dz_, dy_ = _dev(z), _dev(y, np.int32)
    off = torch.empty(B * C + 1, device="cuda")
    zo = off[1:].view(B, C)
    zo.copy_(dz_)
    assert dz_.data_ptr() % 16 == 0 and zo.data_ptr() % 16 == 4
    rbuf = torch.full((B + 2 * GUARD + 1,), -12345.0, device="cuda")
    gbuf = torch.full((B * C + 2 * GUARD + 1,), -12345.0, device="cuda")
    rows, grad = rbuf[GUARD + 1:GUARD + 1 + B], gbuf[GUARD + 1:GUARD + 1 + B * C].view(B, C)
    rows.fill_(float("nan")); grad.fill_(float("nan"))
    assert rows.data_ptr() % 16 == 4 and grad.data_ptr() % 16 == 4
    check(L.isx_softmax_xent_fwd(zo.data_ptr(), dy_.data_ptr(), B, C, rows.data_ptr(), st), "isx_softmax_xent_fwd")
    check(L.isx_softmax_xent_bwd(zo.data_ptr(), dy_.data_ptr(), B, C, 0.2, None, grad.data_ptr(), st), "isx_softmax_xent_bwd")
    for buf, n in ((rbuf, B), (gbuf, B * C)):
        assert bool((buf[:GUARD + 1] == -12345.0).all()) and bool((buf[GUARD + 1 + n:] == -12345.0).all())
    assert _same_bits(rows, _fwd(dz_, dy_, B, C)) and _same_bits(grad, _bwd(dz_, dy_, B, C, 0.2))
    _assert_bits(rows, model.forward(z, y, EXP, LOG), "loss_rows")
    _assert_bits(grad, model.backward(z, y, model.scale_of(0.2), EXP), "dlogits")
    loss, dl = _leaves(zo, dy_, 1, B, C, 0.2, 1.0)
    assert _same_bits(dl, grad)


def test_out_of_range_labels():
    """C, -1, INT32_MAX, INT32_MIN next to good labels: the gradient row is the model's plain p * scale, the row loss and the leaf loss are
    NaN, the good rows and the good leaf are what they are without the bad ones, and nothing is written outside (the guards)."""
    C, k = 65, 4
    z = np.ascontiguousarray(model.kind_rows(C)[0][:2 * k])
    y = np.array([3, C, -1, 7, 0, 1, 2, 64], np.int32)
    bad = ~model.in_range(y, C)
    assert bad.tolist() == [False, True, True, False] + [False] * 4
    for labels in (y, np.where(bad, [I32_MAX, I32_MIN] * k, y).astype(np.int32)):
        dz_, dy_ = _dev(z), _dev(labels, np.int32)
        m, s = model.row_stats(z, EXP)
        want = model.row_grad(z, labels, m, s, model.scale_of(0.2, model.SCALE_DEV), EXP)
        plain = (model.row_terms(z, m, EXP) / s[:, None]) * model.scale_of(0.2, model.SCALE_DEV)
        assert np.array_equal(_bits(want[bad]), _bits(plain[bad]))
        _assert_bits(_bwd(dz_, dy_, 2 * k, C, 0.2, model.SCALE_DEV), want, "isx_softmax_xent_bwd")
        loss, dl = _leaves(dz_, dy_, 2, k, C, 0.2, model.SCALE_DEV)
        _assert_bits(dl, want, "isx_softmax_xent_leaves")
        rows = model.row_loss(z, labels, m, s, LOG)
        assert np.isnan(rows[bad]).all() and np.isfinite(rows[~bad]).all()
        _assert_bits(_fwd(dz_, dy_, 2 * k, C), rows, "loss_rows")
        want_leaf = model.leaf_losses(rows.reshape(2, k))
        assert np.isnan(want_leaf[0]) and np.isfinite(want_leaf[1])
        _assert_bits(loss, want_leaf, "loss_leaf")


def test_empty_problems_launch_nothing():
    L, check, st = _lib()
    z = torch.zeros((4, 8), device="cuda")
    y = torch.zeros((4,), device="cuda", dtype=torch.int32)
    outs = [_guarded(4, 8) for _ in range(3)]
    o = [b[1].data_ptr() for b in outs]
    check(L.isx_softmax_xent_fwd(z.data_ptr(), y.data_ptr(), 0, 8, o[0], st), "isx_softmax_xent_fwd")
    check(L.isx_softmax_xent_bwd(z.data_ptr(), y.data_ptr(), 0, 8, 1.0, None, o[1], st), "isx_softmax_xent_bwd")
    check(L.isx_softmax_xent_leaves(z.data_ptr(), y.data_ptr(), 0, 4, 8, 1.0, 1.0, o[0], o[1], st), "isx_softmax_xent_leaves")
    check(L.isx_debug_expf_logf(z.data_ptr(), 0, o[2], o[2], st), "isx_debug_expf_logf")
    torch.cuda.synchronize()
    for buf, body in outs:
        assert _guards_intact(buf) and bool(torch.isnan(body).all())


# ---- the tail's two neighbours ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,R,N,K", [(1, 1, 1, 4), (2, 3, 18, 260), (3, 5, 311, 8)])
def test_linear_wgrad_leaves_at_its_edges(L, R, N, K):
    """N = 1, 18, 311: the last group of four classes holds 1, 2 and 3; K = 4, 8, 260: one thread, two, and a second block of 256 columns with
    one thread in it.  dw[l] = oracle.cosine_sim(dy_l^T, x_l^T), the row-ordered fma chain from +0, bit for bit; the guards stand behind the
    last leaf."""
    import oracle as O
    lib, check, st = _lib()
    rng = np.random.default_rng(100 * N + K)
    dy, x = rng.standard_normal((L * R, N)).astype(F), rng.standard_normal((L * R, K)).astype(F)
    buf, dw = _guarded(L, N, K)
    ddy, dx = _dev(dy), _dev(x)
    check(lib.isx_linear_wgrad_leaves(ddy.data_ptr(), dx.data_ptr(), L, R, N, K, dw.data_ptr(), st), "isx_linear_wgrad_leaves")
    assert _guards_intact(buf)
    got = dw.cpu().numpy()
    for l in range(L):
        want = O.cosine_sim(np.ascontiguousarray(dy[l * R:(l + 1) * R].T), np.ascontiguousarray(x[l * R:(l + 1) * R].T))
        assert np.array_equal(_bits(got[l]), _bits(want)), (l, float(np.abs(got[l] - want).max()))


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 4), (3, 2, 5, 12), (43, 7, 7, 4096)])
def test_gap_bwd_nhwc_at_its_edges(B, H, W, C):
    """One float4; a map of 10 pixels with 3 float4 per pixel; 43 x 49 x 1024 = 2 157 568 float4, past the 8192 x 256 of one sweep of the grid.
    Every element is ONE IEEE division g / (H W)."""
    lib, check, st = _lib()
    assert (B * H * W * C // 4 > 8192 * 256) == (B == 43)
    rng = np.random.default_rng(B)
    g = rng.standard_normal((B, C)).astype(F)
    if B == 3:
        g[0, :4] = [0.0, -0.0, np.inf, 2.0 ** -140]
    buf, dx = _guarded(B, H * W, C)
    dg = _dev(g)
    check(lib.isx_gap_bwd_nhwc(dg.data_ptr(), B, H, W, C, dx.data_ptr(), st), "isx_gap_bwd_nhwc")
    assert _guards_intact(buf)
    want = _dev(g / F(H * W))
    assert _same_bits(dx, want.view(B, 1, C).expand(B, H * W, C))
