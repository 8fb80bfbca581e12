"""tests/_triplet_model.py, the CPU model the kernels of csrc/train.hip are pinned to in tests/test_gpu_triplet_chains.py, checked on its own:

  * against float64 and oracle.triplet_loss, inside the forward bound derived in the model's docstring: the model is the operation, not a copy
    of the kernel.  No row of the case data is too close to the clamp to be compared: the share left out is asserted to be 0;
  * against the plausible WRONG variants, on exactly the data the GPU test runs: where the model and a wrong variant give the same bits, a
    bit-exact test says nothing about that variant.  The cases that tell each variant apart are printed (pytest -s);
  * mining: against oracle.mine_negatives, against the CPU branch of train.siamese_descriptor._mine_block block by block, blocked against whole,
    and against the wrong readings of the row block;
  * the argument checks of the six entry points, which need no GPU."""
import numpy as np
import pytest
import torch

import _triplet_model as model
import oracle as O

F = np.float32
U = model.U


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def row_sets():
    """(name, a, p, n, margin) of every forward case of the GPU test."""
    for B, D in model.ROW_CASES:
        for m in model.margins(B):
            yield ("%dx%d m=%g" % (B, D, m),) + model.row_case(B, D) + (m,)
    yield ("margin 0 %dx%d" % model.MARGIN_ZERO_CASE,) + model.margin_zero_case() + (0.0,)


def test_case_lists_reach_what_they_claim():
    assert [b % 4 for b, _ in model.ROW_CASES if b in (5, 7)] == [1, 3]                      # a partly empty last workgroup
    assert all(b * d > 4096 * 256 for b, d in model.BWD_PAST_CAP) and (4096 * 256) % model.BWD_PAST_CAP[1][1] != 0
    assert max(k for _, k, _ in model.LEAF_CASES) == 8192
    a, p, n = model.margin_zero_case()
    assert _same_bits(n[1], p[1]) and not _same_bits(n[0], p[0])
    for B, D in model.ROW_CASES:
        a, p, n = model.row_case(B, D)
        if B >= 4:
            assert not a[2].any() and not p[2].any() and not n[2].any()
        rest = np.arange(B) != 2 if B >= 4 else np.ones(B, bool)
        for x in (a, p, n):
            assert np.allclose((x[rest].astype(np.float64) ** 2).sum(1), 1.0, atol=1e-6)


# ---- the model against float64 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalized", [True, False], ids=["normalized", "distance"])
def test_row_sums_lie_inside_the_forward_bound(normalized):
    worst = 0.0
    for name, a, p, n, _ in row_sets():
        s, s64, bound = model.row_sum(a, p, n, normalized), model.row_sum64(a, p, n, normalized), model.row_bound(a, p, n, normalized)
        err = np.abs(s.astype(np.float64) - s64)
        print("%-22s %-10s max error / bound = %.3f" % (name, "normalized" if normalized else "distance", float((err / np.maximum(bound, 1e-300)).max())))
        assert (err <= bound).all(), name
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    assert 0 < worst <= 1


@pytest.mark.parametrize("avg", [True, False], ids=["mean", "sum"])
@pytest.mark.parametrize("normalized", [True, False], ids=["normalized", "distance"])
def test_loss_rows_and_gradients_agree_with_the_oracle(normalized, avg):
    """On the rows whose float64 |l| exceeds the bound -- ALL rows: the share left out is 0 on the chosen seeds.  (A row with n == p bit for bit has
    terms x - x = +0 in fp32 and 0 in float64: its sum is exact whatever the bound says, and it is compared too -- row 1 of the margin-0 case.)  The loss within the bound plus the
    roundings of fl(fl32(s) + margin) on either side; the `on` masks equal; the gradients, the same three fp32 operations per element on both
    sides, equal."""
    left_out = total = clamped = active = 0
    for name, a, p, n, margin in row_sets():
        B = a.shape[0]
        _, rows_o, ga, gp, gn = O.triplet_loss(a, p, n, margin, normalized, avg)
        m64 = float(F(margin))
        s64, bound = model.row_sum64(a, p, n, normalized), model.row_bound(a, p, n, normalized)
        l64 = s64 + m64 if normalized else (s64 + 2 * m64) / 2
        bound_l = bound if normalized else bound / 2
        ok = (np.abs(l64) > bound_l) | (_bits(n) == _bits(p)).all(1)
        left_out, total = left_out + int((~ok).sum()), total + B
        rows = model.loss_rows(a, p, n, margin, normalized)
        assert np.array_equal((rows > 0)[ok], (rows_o > 0)[ok]) and np.array_equal((rows > 0)[ok], (l64 > 0)[ok]), name
        tol = bound_l + 4 * U * (np.abs(s64) + np.abs(l64))
        assert (np.abs(rows.astype(np.float64) - rows_o)[ok] <= tol[ok]).all(), name
        assert (np.abs(rows.astype(np.float64) - np.maximum(l64, 0))[ok] <= tol[ok]).all(), name
        got = model.grads(a, p, n, rows, F(1) / F(B) if avg else F(1), normalized)
        for g, want in zip(got, (ga, gp, gn)):
            assert np.array_equal(g[ok], want[ok]), name
        assert (rows == 0).any() and (rows > 0).any() or B == 1, name                        # clamped and active rows in every case
        clamped, active = clamped + int((rows == 0).sum()), active + int((rows > 0).sum())
    assert left_out == 0, (left_out, total)
    assert clamped >= len(model.ROW_CASES) and active >= len(model.ROW_CASES)


def test_one_row_cases_are_clamped_at_one_margin_and_active_at_the_other():
    a, p, n = model.row_case(1, 1)
    for normalized in (True, False):
        lo, hi = (model.loss_rows(a, p, n, m, normalized) for m in model.margins(1))
        assert lo[0] == 0 and hi[0] > 0


def test_margin_zero_row_is_exactly_plus_zero():
    a, p, n = model.margin_zero_case()
    for normalized in (True, False):
        l = model.loss_of_sum(model.row_sum(a, p, n, normalized), 0.0, normalized)
        assert _bits(l[1:2])[0] == 0 and model.loss_rows(a, p, n, 0.0, normalized)[1] == 0
        g = model.grads(a, p, n, model.loss_rows(a, p, n, 0.0, normalized), F(1), normalized)
        assert not any(x[1].any() for x in g) and all(x[3].any() for x in g)


# ---- the model discriminates: row sums ---------------------------------------------------------------------------------------------------------------
def _sequential(t):
    s = np.zeros(t.shape[0], F)
    for j in range(t.shape[1]):
        s = s + t[:, j]
    return s


def _butterfly_up(v):
    """WRONG: xor 1, 2, 4, ..., 32."""
    lanes = np.arange(model.LANES)
    for o in (1, 2, 4, 8, 16, 32):
        v = v + v[:, lanes ^ o]
    return v[:, 0]


def _terms_factored(a, p, n):
    """WRONG: a * (n - p)."""
    return a * (n - p)


def _terms_fused(a, p, n):
    """WRONG: fma(a, n, -fl(a * p)): the first product exact (float64 holds it), one rounding at the end."""
    return (a.astype(np.float64) * n.astype(np.float64) - (a * p).astype(np.float64)).astype(F)


def _told_apart(what, pairs):
    """pairs: (case, canonical, wrong).  At least one bit of at least one case changes; prints which cases tell the variant apart."""
    hits = []
    for case, canon, wrong in pairs:
        diff = int((_bits(canon) != _bits(wrong)).sum())
        if diff:
            hits.append("%s: %d of %d" % (case, diff, canon.size))
    print("%-44s %s" % (what, "; ".join(hits) if hits else "NOT told apart"))
    assert hits, what
    return hits


def test_row_sum_orders_show_in_the_data():
    """A sequential sum, the butterfly in the order 1, 2, ..., 32 (both forms); a * (n - p) and a fused multiply (normalized form).  Each is told
    apart by at least four of the cases, not by one lucky row."""
    for normalized in (True, False):
        form = "normalized" if normalized else "distance"
        seq, up = [], []
        for name, a, p, n, _ in row_sets():
            t = model.terms(a, p, n, normalized)
            s = model.row_sum(a, p, n, normalized)
            seq.append((name, s, _sequential(t)))
            up.append((name, s, _butterfly_up(model.lane_sums(t))))
        for what, pairs in (("a sequential sum", seq), ("butterfly 1, 2, ..., 32", up)):
            hits = _told_apart("%s (%s)" % (what, form), pairs)
            assert len(hits) >= 4
    fact, fused = [], []
    for name, a, p, n, _ in row_sets():
        s = model.row_sum(a, p, n, True)
        fact.append((name, s, model.butterfly(model.lane_sums(_terms_factored(a, p, n)))))
        fused.append((name, s, model.butterfly(model.lane_sums(_terms_fused(a, p, n)))))
    assert len(_told_apart("terms a * (n - p)", fact)) >= 4
    assert len(_told_apart("terms fma(a, n, -a * p)", fused)) >= 4


def test_halving_before_the_margin_shows_only_below_the_normal_range():
    """(s + 2 m) * 0.5 against s * 0.5 + m: scaling by two commutes with rounding, so on every unit-row case the two are the SAME bits -- asserted,
    so that nobody reads the bit-exact GPU test as telling them apart there -- and differ on the denormal case, which exists for this."""
    for name, a, p, n, margin in row_sets():
        s = model.row_sum(a, p, n, False)
        assert _same_bits(model.loss_of_sum(s, margin, False), s * F(0.5) + F(margin)), name
    a, p, n, margin = model.denormal_case()
    s = model.row_sum(a, p, n, False)
    unit = np.ldexp(1.0, -149)
    assert float(s[0]) == 3 * unit and float(F(margin)) == unit
    good, bad = model.loss_of_sum(s, margin, False), s * F(0.5) + F(margin)
    assert float(good[0]) == 2 * unit and float(bad[0]) == 3 * unit
    _told_apart("(s + 2 m) / 2 formed as s / 2 + m", [("denormal 1x1", good, bad)])


def test_clamp_decision_at_zero_shows_in_the_data():
    """`>=` instead of `>`: the row with l == +0 would get its gradient."""
    pairs = []
    for normalized in (True, False):
        for name, a, p, n, margin in row_sets():
            l = model.loss_of_sum(model.row_sum(a, p, n, normalized), margin, normalized)
            rows = model.clamp(l)
            good = np.concatenate(model.grads(a, p, n, rows, F(1), normalized))
            bad = np.concatenate(model.grads(a, p, n, np.where(l >= 0, F(1), F(0)), F(1), normalized))
            pairs.append(("%s %s" % (name, "normalized" if normalized else "distance"), good, bad))
    hits = _told_apart("`>=` in the clamp mask", pairs)
    assert all(h.startswith("margin 0") for h in hits) and len(hits) == 2


def _dev_sets():
    """(name, a, p, n, rows, scale) of the backward cases: the mean over the batch."""
    for name, a, p, n, margin in row_sets():
        for normalized in (True, False):
            yield name + (" normalized" if normalized else " distance"), a, p, n, model.loss_rows(a, p, n, margin, normalized), 1.0 / a.shape[0], normalized


def test_scale_formed_once_shows_in_the_data():
    """fl(fl(x * sa) * sb) against fl(x * fl(sa * sb)): the _dev entry (1 / B times the device scalar) and the leaves (1 / k times the share)."""
    pairs = []
    for name, a, p, n, rows, scale, normalized in _dev_sets():
        good = np.concatenate(model.grads(a, p, n, rows, model.scale_dev(scale, model.SCALE_DEV), normalized))
        once = np.concatenate(model.grads(a, p, n, rows, F(scale), normalized))
        pairs.append((name, good, (once * F(model.SCALE_DEV)).astype(F)))
    assert len(_told_apart("_dev: scale applied as two multiplies", pairs)) >= 4
    pairs = []
    for L, k, D in model.LEAF_CASES:
        d = model.leaf_case(L, k, D)
        sa, sb = model.leaf_scales(L, k, True)
        good = model.leaves(d, L, k, model.MARGIN, True, sa, sb)[1]
        once = model.leaves(d, L, k, model.MARGIN, True, sa, 1.0)[1]
        pairs.append(("%dx%dx%d" % (L, k, D), good, (once * F(sb)).astype(F)))
    hits = _told_apart("leaves: scale applied as two multiplies", pairs)
    assert any(h.startswith("3x5x100") for h in hits)                                          # 1 / 5 and 1 / 3: neither a power of two


def test_leaf_loss_order_shows_in_the_data():
    pairs = []
    for L, k, D in model.LEAF_CASES:
        for normalized in (True, False):
            loss, _, rows = model.leaves(model.leaf_case(L, k, D), L, k, model.MARGIN, normalized, 1.0, 1.0)
            assert (rows == 0).any() and (rows > 0).any() or k == 1
            pairs.append(("%dx%dx%d" % (L, k, D), loss, np.array([np.sum(r) for r in rows], F)))
    _told_apart("leaf loss by np.sum", pairs)


def test_leaves_are_the_row_functions_leaf_by_leaf():
    L, k, D = 3, 5, 100
    d = model.leaf_case(L, k, D)
    loss, dd, rows = model.leaves(d, L, k, model.MARGIN, True, 0.2, 1.0 / 3)
    for l in range(L):
        a, p, n = (d[(3 * l + i) * k:(3 * l + i + 1) * k] for i in range(3))
        r = model.loss_rows(a, p, n, model.MARGIN, True)
        assert _same_bits(r, rows[l])
        g = model.grads(a, p, n, r, model.scale_leaves(0.2, 1.0 / 3), True)
        assert _same_bits(np.concatenate(g), dd[3 * l * k:3 * (l + 1) * k])
        t = F(0)
        for x in r:
            t = F(t + x)
        assert t == loss[l]


# ---- mining --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semi", [1, 0], ids=["semi_hard", "hard"])
@pytest.mark.parametrize("N", model.MINE_N)
def test_mining_model_is_the_oracle(N, semi):
    c = model.mine_case(N)
    i1, i2, _ = model.all_couples(c)
    for lab in (c.labels, c.labels_one):
        assert np.array_equal(model.mine(c.sim, N, 0, lab, i1, i2, semi), O.mine_negatives(c.sim, lab, i1, i2, semi))
    assert (model.mine(c.sim, N, 0, c.labels_one, i1, i2, semi) == -1).all()


def test_planted_mining_cases_are_what_their_names_say():
    for N in (255, 256, 257, 1000):
        c = model.mine_case(N)
        semi, hard = model.mine_expect(N, 1), model.mine_expect(N, 0)
        tie = [3, 72] + ([515] if N == 1000 else [])
        assert len({int(_bits(c.sim[0, j:j + 1])[0]) for j in tie}) == 1 and c.sim[0, 0] > c.sim[0, 3]
        assert c.sim[0, 3] == np.delete(c.sim[0], np.flatnonzero(c.labels == 0)).max()        # the tie is the top of the row
        assert all(b - a > 64 for a, b in zip(tie, tie[1:])) and len({j % 256 // 64 for j in tie[:2]}) == 2 and (N < 1000 or tie[2] % 256 == tie[0])
        assert semi["tie"][0] == 3 and hard["tie"][0] == 3
        assert _same_bits(c.sim[1, 100:101], c.sim[1, 8:9]) and c.labels[100] != c.labels[1] and semi["equals_pos"][0] != 100
        assert c.sim[2, 9] == c.sim[2].min() and semi["least_similar"][0] == -1 and hard["least_similar"][0] >= 0
        assert np.signbit(c.sim[4, 0]) and not np.signbit(c.sim[4, 1]) and semi["zeros"][0] == 0 and hard["zeros"][0] == 0
        assert hard["inf"][0] == 20 and semi["inf"][0] not in (20, 30, -1) and semi["inf"][1] >= 0 and semi["inf"][2] == -1
        i1, i2 = c.couples["general"]
        assert (np.diff(i1) < 0).any() and (np.diff(i1) > 0).any() and (c.labels[i1] == c.labels[i2]).all()
        assert (semi["general"] == -1).any() or True
    for N in model.MINE_N:
        assert not np.isnan(model.mine_case(N).sim).any()


@pytest.mark.parametrize("semi", [True, False], ids=["semi_hard", "hard"])
@pytest.mark.parametrize("N", model.MINE_N)
def test_blocked_mining_is_whole_matrix_mining_and_the_cpu_branch(N, semi):
    """Every partition of the rows into blocks of 1, 7, N - 1 and N rows: the model on the block (a copy, rows of 3.0 around it) equals the model
    on the whole matrix, and equals the CPU branch of train.siamese_descriptor._mine_block on the same block."""
    from train.siamese_descriptor import _mine_block
    c = model.mine_case(N)
    i1, i2, _ = model.all_couples(c)
    whole = model.mine(c.sim, N, 0, c.labels, i1, i2, semi)
    lab_t = torch.from_numpy(np.array(c.labels))
    for size in sorted({1, 7, max(1, N - 1), N}):
        got = np.full(len(i1), -7, np.int64)
        for r0, r1 in model.partition(N, size):
            sel = np.flatnonzero((i1 >= r0) & (i1 < r1))
            if not len(sel):
                continue
            buf, pad = model.slab(c.sim, r0, r1)
            got[sel] = model.mine(buf[pad:pad + r1 - r0], N, r0, c.labels, i1[sel], i2[sel], semi)
            cpu = _mine_block(torch.from_numpy(np.array(c.sim[r0:r1])), lab_t, torch.from_numpy(i1[sel]), torch.from_numpy(i2[sel]), semi, r0)
            assert np.array_equal(cpu.numpy(), got[sel]), (size, r0)
        assert np.array_equal(got, whole), size


def _orderable(s, fold):
    s = model.fold_zero(s) if fold else s
    u = _bits(s)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _mine_reading(buf, pad, N, row_base, lab, i1, i2, semi, ge=True, tie_last=False, i2_relative=False, row_absolute=False, fold=True):
    """The mining of one row block read out of the flat padded buffer the kernel is handed, with every decision a switch.  All switches at
    their defaults: the model.  -2: the reading leaves the buffer."""
    flat = buf.reshape(-1)
    out = np.empty(len(i1), np.int64)
    for c, (a, p) in enumerate(zip(i1.tolist(), i2.tolist())):
        off = (pad + (a if row_absolute else a - row_base)) * N
        pos = off + (p - row_base if i2_relative else p)
        if off < 0 or off + N > flat.size or pos < 0 or pos >= flat.size:
            out[c] = -2
            continue
        row, sim_pos = flat[off:off + N], flat[pos]
        excl = lab == lab[a]
        if semi:
            excl = excl | ((row >= sim_pos) if ge else (row > sim_pos))
        cand = np.flatnonzero(~excl)
        if not len(cand):
            out[c] = -1
            continue
        key = _orderable(row, fold)[cand]
        best = np.flatnonzero(key == key.max())
        out[c] = cand[best[-1] if tie_last else best[0]]
    return out


def test_mining_readings_show_in_the_data():
    """`>` in the semi-hard test, ties to the largest index, i2 taken block-relative, row a instead of a - row_base, -0 ordered below +0: each
    changes an answer on a NAMED planted case, in the blocks the GPU test hands over."""
    wrongs = {"`>` in the semi-hard test": dict(ge=False), "ties to the largest index": dict(tie_last=True), "i2 block-relative": dict(i2_relative=True),
              "row a, not a - row_base": dict(row_absolute=True), "-0 below +0": dict(fold=False)}
    told = {k: set() for k in wrongs}
    for N in (255, 256, 257, 1000):
        c = model.mine_case(N)
        i1, i2, names = model.all_couples(c)
        names = np.array(names)
        for r0, r1 in model.blocks(N):
            sel = np.flatnonzero((i1 >= r0) & (i1 < r1))
            buf, pad = model.slab(c.sim, r0, r1)
            for semi in (1, 0):
                want = model.mine(c.sim, N, 0, c.labels, i1[sel], i2[sel], semi)
                assert np.array_equal(_mine_reading(buf, pad, N, r0, c.labels, i1[sel], i2[sel], semi), want)
                for what, kw in wrongs.items():
                    bad = _mine_reading(buf, pad, N, r0, c.labels, i1[sel], i2[sel], semi, **kw)
                    told[what] |= set(names[sel][bad != want].tolist())
    for what, cases in told.items():
        print("%-30s changes %s" % (what, sorted(cases)))
    assert "equals_pos" in told["`>` in the semi-hard test"]
    assert {"tie", "zeros"} <= told["ties to the largest index"]
    assert told["i2 block-relative"] - {"general", "same"}
    assert told["row a, not a - row_base"] - {"general", "same"}
    assert "zeros" in told["-0 below +0"] and told["-0 below +0"] <= {"zeros", "general", "same"}       # only row 4 holds zeros


# ---- argument checks, no GPU -----------------------------------------------------------------------------------------------------------------------
def test_training_step_entries_check_their_arguments_without_a_gpu():
    from isx import _lib
    L = _lib.lib()
    err = L.isx_last_error
    for N, row_base, rows in ((10, 4, 7), (10, -1, 3), (10, 2, -1)):
        assert L.isx_mine_negatives_rows(None, N, row_base, rows, None, None, None, 3, 1, None, None) == -1 and b"bad shape" in err()
    assert L.isx_mine_negatives_rows(None, 10, 0, 0, None, None, None, 3, 1, None, None) == -1 and b"empty block" in err()
    assert L.isx_mine_negatives_rows(None, 10, 2, 3, None, None, None, 0, 1, None, None) == 0
    assert L.isx_mine_negatives(None, 10, None, None, None, 0, 1, None, None) == 0
    assert L.isx_triplet_leaves(None, 2, 8193, 64, 0.1, 1, 1.0, 1.0, None, None, None) == -1 and b"bad shape" in err()
    import ctypes
    x = (ctypes.c_float * 4)()
    ptr = ctypes.cast(x, ctypes.c_void_p)
    assert L.isx_triplet_loss_bwd_dev(ptr, ptr, ptr, ptr, 1, 1, 1.0, None, 1, ptr, ptr, ptr, None) == -1 and b"null pointer" in err()
    assert L.isx_triplet_loss_fwd(None, None, None, 0, 64, 0.1, 1, None, None) == 0
    assert L.isx_triplet_loss_bwd(None, None, None, None, 0, 64, 1.0, 1, None, None, None, None) == 0
