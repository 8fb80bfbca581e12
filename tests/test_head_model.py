"""tests/_head_model.py, the CPU model the descriptor head's kernels are pinned to in tests/test_gpu_head_chains.py, checked on its own:

  * against float64, at the tolerances tests/test_gpu_head.py holds the kernels to: the model is the operation, not a copy of the kernel;
  * against the plausible WRONG orders of summation, on the data of every shape the GPU test runs: where the canonical result and a wrong order
    give the same bits, a bit-exact test says nothing about that order.  The share of differing elements is printed (pytest -s);
  * sharded: the parts of P = 2, 4, 8 ranks are the unsharded parts, and ShardedHead.backward's in-order sum of them is dgrad.

A wrong order is only asked to show where it is another expression: a + b = b + a bit for bit, so two partials added in reverse order, or two
rows summed from +0 in reverse order, are NOT another order; such cases are left out below, each with its reason."""
import numpy as np
import pytest

import _head_model as model

F = np.float32


def _rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max()) / (float(np.abs(b).max()) + 1e-30)


def _share(name, case, canon, wrong):
    diff = float(np.mean(canon != wrong))
    print("%-34s %-28s %6.2f %% of %d elements differ" % (name, case, 100 * diff, canon.size))
    assert not np.array_equal(canon, wrong), (name, case)
    return diff


_FWD_ALL_K = model.FWD_K + (model.FWD_CAP[2],)


def _fwd_shapes(K):
    if K == model.FWD_CAP[2]:
        return [model.FWD_CAP[:2]]
    return [(M, N) for M in model.FWD_M for N in model.FWD_N]


# ---- the model against float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", _FWD_ALL_K)
def test_linear_fwd_against_float64(K):
    x, w, bias, _, y = model.fwd_case(K)
    x, w, bias, y = x[:64], w[:64], bias[:64], y[:64, :64]
    assert np.array_equal(model.linear_fwd(x, w), y)                           # the corner of the shared case is the case
    got = model.linear_fwd(x, w, bias)
    assert np.array_equal(got, y + bias[None, :])
    assert _rel(got, x.astype(np.float64) @ w.astype(np.float64).T + bias.astype(np.float64)) <= 2e-6
    assert _rel(y, x.astype(np.float64) @ w.astype(np.float64).T) <= 2e-6


@pytest.mark.parametrize("N,K,M", model.DGRAD_CASES)
def test_dgrad_against_float64(N, K, M):
    dy, w, _, dx = model.dgrad_case(N, K, M)
    assert np.array_equal(model.dgrad(dy, w), dx)
    assert _rel(dx, dy.astype(np.float64) @ w.astype(np.float64)) <= 5e-6


@pytest.mark.parametrize("N,K", model.SGD_NK)
@pytest.mark.parametrize("R", model.SGD_R)
def test_wgrad_rows_against_float64(N, K, R):
    dy, x, g = model.rows_case(N, K, R)
    assert g.shape == (N, K)
    if R == 0:
        assert not g.any()
    else:
        assert _rel(g, dy.astype(np.float64).T @ x.astype(np.float64)) <= 2e-6


@pytest.mark.parametrize("leaves,R,C", model.COLSUM_CASES)
def test_colsum_leaves_against_float64(leaves, R, C):
    x, s = model.colsum_case(leaves, R, C)
    assert s.shape == (leaves, C)
    assert _rel(s, x.astype(np.float64).reshape(leaves, R, C).sum(1)) <= 2e-6


def test_sgd_step_against_float64():
    """Three steps of every hyperparameter set against the same formulas in float64 (torch.optim.SGD's: _single_tensor_sgd)."""
    N, K, R = 64, 128, 24
    for name, lr, mom, damp, wd, nest in model.SGD_SETS:
        w = model.sgd_w0(N, K)
        w64, buf, buf64 = w.astype(np.float64), None, None
        for step in range(3):
            g = model.rows_case(N, K, R, seed=step)[2]
            w, buf = model.sgd_step(w, buf, g, step == 0, lr, mom, damp, wd, nest)
            g64 = g.astype(np.float64) + wd * w64
            if mom:
                buf64 = g64 if step == 0 else mom * buf64 + (1 - damp) * g64
                g64 = g64 + mom * buf64 if nest else buf64
            w64 = w64 - lr * g64
            assert _rel(w, w64) <= 1e-6, (name, step)
            assert (buf is None) == (mom == 0) and (buf is None or _rel(buf, buf64) <= 1e-6), (name, step)


# ---- the model discriminates ---------------------------------------------------------------------------------------------------------------
def _floor_ranges(K):
    """Splits cut at floor((K / 32) / S) k-tiles, the last split taking the rest."""
    S = model.splits(K)[0]
    per = (K // 32) // S
    return [(32 * s * per, K if s == S - 1 else 32 * (s + 1) * per) for s in range(S)]


@pytest.mark.parametrize("K", _FWD_ALL_K)
def test_forward_orders_show_in_the_data(K):
    """One chain without splits (S >= 2), splits cut at floor instead of ceil (where the two differ: 133 tiles in 2, 2117 tiles in 32), partials
    added in reverse order (S >= 3; two partials commute).  K = 32 and 2016 are one chain by definition: nothing to tell apart, only the split
    rule itself, which the GPU test compares with isx_head_linear_splits."""
    x, w, _, parts, y = model.fwd_case(K)
    S, kt_per, ranges = model.splits(K)
    assert ranges[0][0] == 0 and ranges[-1][1] == K and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])) and all(lo < hi for lo, hi in ranges)
    assert S == (1, 1, 2, 3, 32)[_FWD_ALL_K.index(K)]
    wrong = {}
    if S >= 2:
        wrong["one chain without splits"] = model.chains(x, w)
    if _floor_ranges(K) != ranges:
        wrong["splits cut at floor"] = model.add_in_order(model.linear_partials(x, w, _floor_ranges(K)))
    if S >= 3:
        wrong["partials in reverse order"] = model.add_in_order(list(parts[::-1]))
    assert sorted(wrong) == {32: [], 2016: [], 4256: ["one chain without splits", "splits cut at floor"],
                             6144: ["one chain without splits", "partials in reverse order"],
                             67744: ["one chain without splits", "partials in reverse order", "splits cut at floor"]}[K]
    for name, bad in wrong.items():
        _share(name, "fwd K=%d %dx%d" % ((K,) + y.shape), y, bad)
        low = min(float(np.mean(y[:M, :N] != bad[:M, :N])) for M, N in _fwd_shapes(K))
        print("%-34s %-28s lowest share over the %d (M, N) cases: %.2f %%" % (name, "fwd K=%d" % K, len(_fwd_shapes(K)), 100 * low))
        for M, N in _fwd_shapes(K):
            assert not np.array_equal(y[:M, :N], bad[:M, :N]), (name, K, M, N)


def test_part_sizes_show_in_the_data():
    """The parts call with 5 groups of 96 features against 3 groups of 160 over the same features."""
    dy, w, parts = model.parts_extra_case()
    _share("3 groups of 160, not 5 of 96", "parts N=480 K=%d M=%d" % model.PARTS_EXTRA[2:], model.fold(parts), model.fold(model.dgrad_parts(dy, w, 160)))


@pytest.mark.parametrize("N,K,M", [c for c in model.DGRAD_CASES if model.groups(c[0]) == 8])
def test_dgrad_orders_show_in_the_data(N, K, M):
    """4 groups instead of 8, the group sums added in reverse order, one chain over all N -- for the G = 8 shapes (G = 1 is one chain)."""
    dy, w, parts, dx = model.dgrad_case(N, K, M)
    case = "dgrad N=%d K=%d M=%d" % (N, K, M)
    _share("4 groups instead of 8", case, dx, model.fold(model.dgrad_parts(dy, w, N // 4)))
    _share("groups in reverse order", case, dx, model.fold(parts[::-1]))
    _share("one chain without groups", case, dx, model.dgrad_parts(dy, w, N)[0])


@pytest.mark.parametrize("N,K", model.SGD_NK)
@pytest.mark.parametrize("R", [r for r in model.SGD_R if r >= 2])
def test_wgrad_row_order_shows_in_the_data(N, K, R):
    """Rows summed in reverse order.  R = 0 and 1 have one order.  (Two rows already differ: the first product of a chain is rounded, the second
    is fused into the add.)"""
    dy, x, g = model.rows_case(N, K, R)
    _share("rows in reverse order", "wgrad N=%d K=%d R=%d" % (N, K, R), g, model.wgrad_rows(dy[::-1], x[::-1]))


@pytest.mark.parametrize("leaves,R,C", [c for c in model.COLSUM_CASES if c[1] >= 3])
def test_colsum_row_order_shows_in_the_data(leaves, R, C):
    """Rows summed in reverse order; (0 + a) + b = (0 + b) + a: up to two rows there is one order."""
    x, s = model.colsum_case(leaves, R, C)
    rev = np.ascontiguousarray(x.reshape(leaves, R, C)[:, ::-1]).reshape(leaves * R, C)
    _share("rows in reverse order", "colsum %dx%dx%d" % (leaves, R, C), s, model.colsum_leaves(rev, leaves, R))


def _sgd_decay_after(w, buf, g, first, lr, momentum, dampening, weight_decay, nesterov):
    """WRONG: the momentum buffer sees the gradient without the decay term, which joins the update behind it."""
    lr, momentum, dampening, weight_decay = F(lr), F(momentum), F(dampening), F(weight_decay)
    upd = g
    if momentum != 0:
        buf = g.copy() if first else momentum * buf + (F(1) - dampening) * g
        upd = g + momentum * buf if nesterov else buf
    return w - lr * (upd + weight_decay * w), buf


def _sgd_decay_decoupled(w, buf, g, first, lr, momentum, dampening, weight_decay, nesterov):
    """WRONG: the step without decay, then the weight shrunk by lr * weight_decay * w."""
    w1, buf = model.sgd_step(w, buf, g, first, lr, momentum, dampening, 0.0, nesterov)
    return w1 - (F(lr) * F(weight_decay)) * w, buf


def _sgd_damp_first(w, buf, g, first, lr, momentum, dampening, weight_decay, nesterov):
    """WRONG: the first step's buffer is (1 - dampening) * g instead of g."""
    if not first or momentum == 0:
        return model.sgd_step(w, buf, g, first, lr, momentum, dampening, weight_decay, nesterov)
    if weight_decay != 0:
        g = g + F(weight_decay) * w
    buf = (F(1) - F(dampening)) * g
    return w - F(lr) * (g + F(momentum) * buf if nesterov else buf), buf


@pytest.mark.parametrize("N,K,R", model.SGD_UPDATE_NKR)
def test_sgd_orders_show_in_the_data(N, K, R):
    """Weight decay applied behind the momentum update (two readings of it; the first needs a momentum to be another expression) and dampening
    applied on the first step (needs a dampening): the weight after the three steps of the GPU test differs."""
    for name, lr, mom, damp, wd, nest in model.SGD_SETS:
        wrongs = []
        if wd and mom:
            wrongs.append(("decay behind the momentum update", _sgd_decay_after))
        if wd:
            wrongs.append(("decay decoupled from the gradient", _sgd_decay_decoupled))
        if damp:
            wrongs.append(("dampening on the first step", _sgd_damp_first))
        for what, step_fn in wrongs:
            w = bad = model.sgd_w0(N, K)
            buf = bad_buf = None
            for step in range(3):
                g = model.rows_case(N, K, R, seed=step)[2]
                w, buf = model.sgd_step(w, buf, g, step == 0, lr, mom, damp, wd, nest)
                bad, bad_buf = step_fn(bad, bad_buf, g, step == 0, lr, mom, damp, wd, nest)
            _share(what, "sgd %s N=%d K=%d" % (name, N, K), w, bad)
    # every set is told apart from its neighbours by at least one of the above or by its own hyperparameters: the five sets give five weights
    finals = []
    for name, lr, mom, damp, wd, nest in model.SGD_SETS:
        w, buf = model.sgd_w0(N, K), None
        for step in range(3):
            w, buf = model.sgd_step(w, buf, model.rows_case(N, K, R, seed=step)[2], step == 0, lr, mom, damp, wd, nest)
        finals.append(w)
    assert all(not np.array_equal(a, b) for i, a in enumerate(finals) for b in finals[i + 1:])


# ---- sharding in the model -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,M", [c for c in model.DGRAD_CASES if model.groups(c[0]) == 8])
def test_sharded_parts_add_up_to_dgrad(N, K, M):
    """Rank r of P computes the chains of ITS consecutive groups from its slice of dy and w; concatenated in rank order they are the unsharded
    parts, and ShardedHead.backward's sum (pieces[0].clone(), then += in order) is dgrad: 0 + c_0 and c_0 differ at most in the sign of a zero."""
    dy, w, parts, dx = model.dgrad_case(N, K, M)
    Ng = N // 8
    for P in (2, 4, 8):
        per = 8 // P * Ng
        pieces = np.concatenate([model.dgrad_parts(dy[:, r * per:(r + 1) * per], w[r * per:(r + 1) * per], Ng) for r in range(P)], 0)
        assert np.array_equal(pieces, parts), P
        tot = pieces[0].copy()
        for g in range(1, 8):
            tot += pieces[g]
        assert np.array_equal(tot, dx), P
