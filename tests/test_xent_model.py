"""tests/_xent_model.py, the CPU model the cross-entropy kernels of csrc/classif.hip are pinned to in tests/test_gpu_xent_chains.py, checked on
its own, with correctly rounded exp and log:

  * against F.cross_entropy and its autograd in float64, inside the bound derived in the model's docstring: the model is the operation, not a
    copy of the kernel; the rows with non-finite logits are NaN, infinite and finite where torch's are;
  * against the plausible WRONG readings, on exactly the data the GPU test runs: where the model and a wrong reading give the same bits, a
    bit-exact test says nothing about that reading.  The cases that tell each reading apart are printed (pytest -s)."""
import numpy as np
import torch
import torch.nn.functional as TF

import _xent_model as model
from _triplet_model import LANES, butterfly, lane_sums
from test_triplet_model import _bits, _butterfly_up, _sequential, _told_apart

F = np.float32
EXP, LOG = model.exp_ref, model.log_ref


def row_sets():
    """(name, z, labels) of every row batch of the GPU test."""
    for C in model.C_CASES:
        yield ("C=%d" % C,) + model.kind_rows(C)[:2]
    for C in model.B_CASES_C:
        for B in model.B_CASES:
            yield ("B=%d C=%d" % (B, C),) + model.batch_case(B, C)[:2]


def leaf_sets():
    for L, k, C in model.LEAF_CASES:
        yield ("%dx%dx%d" % (L, k, C), L, k) + model.leaf_case(L, k, C)


def _same(a, b):
    """Bit for bit, a NaN equal to a NaN."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)])


def _canon(x):
    """NaNs onto one pattern, so that _told_apart counts bits of numbers only."""
    x = np.array(x, F)
    x[np.isnan(x)] = np.nan
    return x


def test_case_lists_reach_what_they_claim():
    assert {c for c in model.C_CASES if c < 64} and {63, 64, 65, 127, 128, 129} <= set(model.C_CASES) and max(model.C_CASES) > 64 * 64
    assert sorted(b % 4 for b in model.B_CASES) == [0, 1, 1, 3, 3]
    assert max(k for _, k, _ in model.LEAF_CASES) == 8192 and any(k % 4 and k > 4096 for _, k, _ in model.LEAF_CASES)
    for C in model.C_CASES:
        z, y, names = model.kind_rows(C)
        assert len(names) == 25 and len(names) % 4 and z.shape == (25, C) and ((y >= 0) & (y < C)).all()
        for r, name in enumerate(names):
            kind, _, where = name.partition("/")
            if where == "max" and not np.isnan(z[r]).all():
                assert z[r, y[r]] == np.nanmax(z[r]), name
            if where == "min" and not np.isnan(z[r]).all():
                assert z[r, y[r]] == np.nanmin(z[r]), name
            if where == "else" and C >= 3 and kind not in ("equal", "all_minus_inf"):
                assert np.nanmin(z[r]) < z[r, y[r]] < np.nanmax(z[r]), name
            if kind == "ties":
                assert (z[r] == z[r].max()).sum() == min(3, C)
            if kind == "masked" and C >= 2:
                assert np.isneginf(z[r]).any() and np.isfinite(z[r, 0])
        for r in range(model.N_FINITE, 24):
            want = model.NAN_KINDS[(r - model.N_FINITE) // 3]
            assert names[r].startswith(want) and {"plus_inf": np.isposinf(z[r]).sum() == 1, "nan": np.isnan(z[r]).sum() == 1, "all_minus_inf": np.isneginf(z[r]).all()}[want]
        assert names[24] == "zeros" and not z[24].any() and np.signbit(z[24, 0]) and (C == 1 or not np.signbit(z[24, 1]))
    for C in model.B_CASES_C:
        for B in model.B_CASES:
            z, y, names = model.batch_case(B, C)
            assert z.shape == (B, C) and (B < 3 or names[-1].split("/")[0] in model.NAN_KINDS)
    assert len({model.batch_case(B, 65)[2][-1].split("/")[0] for B in model.B_CASES if B >= 3}) == 3
    e = EXP(np.array([-80, -90, -100, -104, -160], F))
    assert 0 < e[1] < 2.0 ** -126 and e[4] == 0                  # the +-80 spread reaches the denormals and zero
    # the pair of scales whose product is not the two multiplies in turn
    x = np.linspace(0.1, 1.0, 64).astype(F)
    assert ((x * F(0.2)) * F(model.SCALE_DEV) != x * model.scale_of(0.2, model.SCALE_DEV)).any()
    tiny = model.scale_of(2.0 ** -100, 2.0 ** -40)
    assert 0 < tiny < 2.0 ** -126 and model.scale_of(0.5) == F(0.5)


# ---- the model against float64 ------------------------------------------------------------------------------------------------------------------
def _torch64(z, y, scale):
    zt = torch.from_numpy(np.array(z, np.float64)).requires_grad_(True)
    rows = TF.cross_entropy(zt, torch.from_numpy(np.array(y, np.int64)), reduction="none")
    (rows.sum() * float(scale)).backward()
    return rows.detach().numpy(), zt.grad.numpy()


def test_model_is_cross_entropy_inside_the_derived_bound():
    """Losses and gradients of every finite row of every batch, at the scales 1, 1 / 7, -0.75 and the pairs; the share of the bound used is
    printed and lies in (0, 1]."""
    worst_l = worst_g = 0.0
    compared = 0
    for name, z, y in row_sets():
        fin = model.finite_rows(z, y)
        m, s = model.row_stats(z, EXP)
        loss = model.row_loss(z, y, m, s, LOG)
        for a, b in model.SCALES:
            scale = model.scale_of(a, b)
            loss64, dz64 = _torch64(z, y, scale)
            loss_b, dz_b = model.bounds(z, y, scale)
            dz = model.row_grad(z, y, m, s, scale, EXP)
            ok = fin & np.isfinite(loss64)
            assert np.isfinite(loss[ok]).all() and np.isfinite(dz[fin]).all() and np.isfinite(dz64[fin]).all(), name
            with np.errstate(invalid="ignore"):
                el = np.abs(loss.astype(np.float64) - loss64)[ok]
            eg = np.abs(dz.astype(np.float64) - dz64)[fin]
            assert (el <= loss_b[ok]).all(), (name, float((el / loss_b[ok]).max()))
            assert (eg <= dz_b[fin]).all(), (name, a, b, float((eg / dz_b[fin]).max()))
            if ok.any():
                worst_l = max(worst_l, float((el / loss_b[ok]).max()))
            worst_g = max(worst_g, float((eg / dz_b[fin]).max()))
            compared += int(fin.sum())
    print("largest error / bound: loss %.3f, gradient %.3f, %d rows" % (worst_l, worst_g, compared))
    assert 0 < worst_l <= 1 and 0 < worst_g <= 1 and compared > 1000


def test_leaf_model_is_the_sum_of_cross_entropy_rows():
    """The leaf loss against the float64 sum: the rows' bounds plus k - 1 roundings of the running sum of non-negative rows."""
    for name, L, k, z, y in leaf_sets():
        loss, dz, rows = model.leaves(z, y, L, k, 1.0 / k, 1.0 / L, EXP, LOG)
        scale = model.scale_of(1.0 / k, 1.0 / L)
        loss64, dz64 = _torch64(z, y, scale)
        loss_b, dz_b = model.bounds(z, y, scale)
        assert np.isfinite(rows).all() and (rows >= 0).all(), name
        total = loss64.reshape(L, k).sum(1)
        bound = loss_b.reshape(L, k).sum(1) + k * model.U * total
        assert (np.abs(loss.astype(np.float64) - total) <= bound).all(), name
        assert (np.abs(dz.astype(np.float64) - dz64) <= dz_b).all(), name
        assert _same(dz, model.backward(z, y, scale, EXP)) and _same(rows.reshape(-1), model.forward(z, y, EXP, LOG))


def test_non_finite_rows_are_what_float64_cross_entropy_gives():
    """+inf, NaN, only -inf: NaN throughout.  A -inf column: exact zeros, a zero with the sign of the scale in dz; the label on it: +inf."""
    seen = set()
    for name, z, y in row_sets():
        for a, b in model.SCALES:
            scale = model.scale_of(a, b)
            loss64, dz64 = _torch64(z, y, scale)
            loss, dz = model.forward(z, y, EXP, LOG), model.backward(z, y, scale, EXP)
            assert np.array_equal(np.isnan(loss), np.isnan(loss64)) and np.array_equal(np.isposinf(loss), np.isposinf(loss64)), name
            assert not np.isneginf(loss).any() and not np.isinf(dz).any(), name
            assert np.array_equal(np.isnan(dz), np.isnan(dz64)), name
            nan_rows = ~model.finite_rows(z, y)
            assert np.isnan(loss[nan_rows]).all() and np.isnan(dz[nan_rows]).all() and not np.isnan(loss[~nan_rows]).any() and not np.isnan(dz[~nan_rows]).any(), name
            masked = np.isneginf(z) & ~nan_rows[:, None] & (model.onehot(y, z.shape[1]) == 0)
            if masked.any():
                assert (dz[masked] == 0).all() and (np.signbit(dz[masked]) == bool(np.signbit(scale))).all(), (name, a, b)
                seen.add(bool(np.signbit(scale)))
            on_mask = ~nan_rows & np.isneginf(z[np.arange(len(y)), y])
            assert np.isposinf(loss[on_mask]).all() and (dz[on_mask, y[on_mask]] == -scale).all(), name
    assert seen == {True, False}


# ---- the model discriminates ---------------------------------------------------------------------------------------------------------------------
def _blocks(t):
    """WRONG: lane i owns the contiguous columns [i * w, (i + 1) * w), w = ceil(C / 64)."""
    B, C = t.shape
    w = (C + LANES - 1) // LANES
    v = np.zeros((B, LANES), F)
    for i in range(LANES):
        for j in range(i * w, min((i + 1) * w, C)):
            v[:, i] = v[:, i] + t[:, j]
    return butterfly(v)


def _tree(t):
    """WRONG: a pairwise tree over the columns (rows of a 2-D array: over axis 1)."""
    t = np.asarray(t, F)
    while t.shape[1] > 1:
        n = t.shape[1]
        head = t[:, 0:n - n % 2:2] + t[:, 1:n:2]
        t = np.concatenate([head, t[:, n - 1:]], 1) if n % 2 else head
    return t[:, 0]


def _wave_order(rows):
    """WRONG: the leaf's rows added as the four waves computed them: 0, 4, 8, ..., then 1, 5, ..."""
    k = rows.shape[1]
    order = [r for w in range(4) for r in range(w, k, 4)]
    t = np.zeros(rows.shape[0], F)
    for r in order:
        t = t + rows[:, r]
    return t


def test_row_sum_orders_show_in_the_data():
    seq, blk, up, tree = [], [], [], []
    with np.errstate(all="ignore"):
        for name, z, y in row_sets():
            m = model.row_max(z)
            t = model.row_terms(z, m, EXP)
            s = _canon(model.row_sum(z, m, EXP))
            seq.append((name, s, _canon(_sequential(t))))
            blk.append((name, s, _canon(_blocks(t))))
            up.append((name, s, _canon(_butterfly_up(lane_sums(t)))))
            tree.append((name, s, _canon(_tree(t))))
    for what, pairs in (("a sequential sum over j", seq), ("lanes owning contiguous blocks", blk), ("butterfly 1, 2, ..., 32", up), ("a pairwise tree over the columns", tree)):
        assert len(_told_apart(what, pairs)) >= 4


def test_loss_groupings_show_in_the_data():
    a, b = [], []
    with np.errstate(all="ignore"):
        for name, z, y in row_sets():
            m, s = model.row_stats(z, EXP)
            zy = z[np.arange(len(y)), y]
            good = _canon(model.row_loss(z, y, m, s, LOG))
            a.append((name, good, _canon(LOG(s) + (m - zy))))
            b.append((name, good, _canon(-((zy - m) - LOG(s)))))
    assert len(_told_apart("log s + (m - z_label)", a)) >= 4
    assert len(_told_apart("-(z_label - m - log s)", b)) >= 4


def test_gradient_readings_show_in_the_data():
    """At scale 1 / 7 (and the pair (0.2, 1 / 3) for the two multiplies)."""
    logp, recip, dist, twice = [], [], [], []
    with np.errstate(all="ignore"):
        for name, z, y in row_sets():
            m, s = model.row_stats(z, EXP)
            scale = model.scale_of(1.0 / 7.0)
            good = _canon(model.row_grad(z, y, m, s, scale, EXP))
            oh = model.onehot(y, z.shape[1])
            e = model.row_terms(z, m, EXP)
            logp.append((name, good, _canon((EXP((z - m[:, None]) - LOG(s)[:, None]) - oh) * scale)))
            recip.append((name, good, _canon((e * (F(1) / s)[:, None] - oh) * scale)))
            p = e / s[:, None]
            dist.append((name, good, _canon(p * scale - oh * scale)))
            pair = _canon(model.row_grad(z, y, m, s, model.scale_of(0.2, model.SCALE_DEV), EXP))
            twice.append((name, pair, _canon(((p - oh) * F(0.2)) * F(model.SCALE_DEV))))
    assert len(_told_apart("p = exp(z - m - log s)", logp)) >= 4
    assert len(_told_apart("p = exp(z - m) * (1 / s)", recip)) >= 4
    assert len(_told_apart("p * scale - onehot * scale", dist)) >= 4
    assert len(_told_apart("the scale applied as two multiplies", twice)) >= 4


def test_a_maximum_that_propagates_nan_shows_in_m_and_nowhere_else():
    """np.maximum instead of fmaxf: m of the NaN row changes -- row_max tells the two apart -- and nothing a kernel WRITES does: the NaN column
    puts a NaN into s either way, the row is NaN throughout.  Asserted, so that nobody reads the bit-exact GPU test as pinning fmaxf."""
    pairs, hits = [], 0
    for name, z, y in row_sets():
        good = model.row_max(z)
        with np.errstate(all="ignore"):
            bad = np.maximum.reduce(z, axis=1)
            pairs.append((name, _canon(good), _canon(bad)))
            s_bad = butterfly(lane_sums(EXP(z - bad[:, None])))
            assert _same(model.row_loss(z, y, bad, s_bad, LOG), model.forward(z, y, EXP, LOG)), name
            assert _same(model.row_grad(z, y, bad, s_bad, F(1), EXP), model.backward(z, y, F(1), EXP)), name
        nan_row = np.isnan(z).any(1)
        assert np.isnan(bad[nan_row]).all() and not np.isnan(good).any()                  # C = 1: the NaN is the row, m stays -inf
        hits += int(nan_row.sum())
    assert len(_told_apart("the maximum propagating a NaN (m only)", pairs)) >= 4 and hits >= len(model.C_CASES)
    assert np.isneginf(model.row_max(np.full((1, 5), -np.inf, F)))[0] and model.row_max(np.array([[np.nan, -3.0]], F))[0] == -3


def test_leaf_loss_orders_show_in_the_data():
    tree, wave = [], []
    for name, L, k, z, y in leaf_sets():
        loss, _, rows = model.leaves(z, y, L, k, 1.0, 1.0, EXP, LOG)
        tree.append((name, loss, _tree(rows)))
        wave.append((name, loss, _wave_order(rows)))
    assert len(_told_apart("leaf loss as a pairwise tree", tree)) >= 2
    hits = _told_apart("leaf loss in wave order", wave)
    assert any(h.startswith("1x8192x3") for h in hits) and any(h.startswith("2x4097x3") for h in hits)


def test_lookup_through_unique_bits_is_the_function():
    x = np.array([[0.0, -0.0, 1.5, 1.5], [-np.inf, np.nan, 1.5, -3.0]], F)
    calls = []
    got = model.through_unique_bits(lambda v: (calls.append(v.size), model.exp_ref(v))[1])(x)
    assert _same(got, model.exp_ref(x)) and calls == [6]                                       # +0 and -0 are two patterns
