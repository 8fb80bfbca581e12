"""The references of tests/test_gpu_special_values.py, on the CPU: every case and plan the GPU file runs is non-vacuous -- judged from the oracle or
model alone, never from a kernel.  planted (without ReLU): NaN, +inf and -inf among the outputs and at most 25 % NaN; the subnormal plans: at
least 90 % of the nonzero outputs subnormal, fewer than 10 % exact zeros; overflowing: NaN, +inf, -inf and finite outputs, at least 25 % finite.

Two conditions are narrowed where arithmetic rules them out, and the narrowed form is asserted instead of dropped:
  * an overflowing reduction of ONE chunk (K <= 64) without residual cannot give NaN from finite operands (a chain that reached +inf stays there);
    those cases assert that there is none;
  * behind a ReLU (stem, pool, the mid activation) there is no -inf and a NaN has become 0: those assert +inf and the finite share."""
import numpy as np
import pytest

import _special_values as S

F = np.float32


def test_this_process_keeps_subnormals():
    """Otherwise the reference is the thing that flushes."""
    assert F(1e-40) * F(0.5) != 0
    assert S.keeps_subnormals()
    a = S.scale(np.ones(4, F), -140)
    assert (a != 0).all() and (a + a == S.scale(np.ones(4, F), -139)).all()


def test_planted_patterns_are_not_guard_patterns():
    import re, os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "_guards.py")).read()
    taken = {int(v, 16) for v in re.findall(r"= (0x[0-9A-Fa-f]{8})\b", src)}
    assert {0x7FC0DEAD, 0x7FC0BEEF} <= taken
    for v in (S.NAN_A, S.NAN_B):
        assert np.isnan(v) and int(S.bits(v)[0]) not in taken
    assert S.bits(S.NAN_A)[0] >> 31 == 0 and S.bits(S.NAN_B)[0] >> 31 == 1 and (S.bits(S.NAN_A)[0] ^ S.bits(S.NAN_B)[0]) & 0x3FFFFF


def test_compare_rule():
    a = np.array([1, np.nan, -0.0, np.inf, 1e-40], F)
    b = a.copy()
    b[1] = S.NAN_B
    S.compare(a, b)
    b[2] = 0.0
    with pytest.raises(AssertionError):
        S.compare(a, b)
    S.compare(a, b, fold_zero_sign=True)
    b[4] = 0
    with pytest.raises(AssertionError):
        S.compare(a, b, fold_zero_sign=True)
    b[4], b[0] = a[4], np.nan
    with pytest.raises(AssertionError):
        S.compare(a, b, fold_zero_sign=True)


def _check(plan, ref_of, what, can_nan=True, signed=True, ignore=None):
    """ref_of(residual, relu) -> reference output.  planted: judged on the run without ReLU, and the ReLU run has no NaN left;
    other plans: with and without the residual."""
    for res, relu in S.flags(plan):
        y = ref_of(res, relu)
        if plan == "planted":
            if relu:
                assert not np.isnan(y).any() and not (y < 0).any(), what
            else:
                S.check_plan(plan, y, what, signed=signed)
        else:
            S.check_plan(plan, y, (what, "residual", res), can_nan=can_nan, signed=signed, ignore=ignore)


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("M,Cin,Cout", S.C1_TILED + S.C1_STREAM)
def test_conv1x1(M, Cin, Cout, plan):
    _check(plan, lambda res, relu: S.c1_reference(M, Cin, Cout, plan, res, relu), (M, Cin, Cout, plan), can_nan=Cin > 64)


@pytest.mark.parametrize("plan", S.PLANS)
def test_conv1x1_tail_grid(plan):
    import _guards as G
    M, Cin, Cout = S.C1_TAIL
    split = G.tail_split_rows(M, Cout)
    assert split == 131072
    _check(plan, lambda res, relu: S.c1_reference(M, Cin, Cout, plan, res, relu, split), (S.C1_TAIL, plan), can_nan=Cin > 64)
    if plan == "planted":
        x = S.c1_operands(M, Cin, Cout, plan, True, split)[0]
        bad = np.flatnonzero(~np.isfinite(x).all(1))
        assert (bad >= split).sum() >= 4, "planted sites inside the 64x64 region"


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.DUAL)
def test_conv1x1_dual(case, plan):
    for relu in (True, False):
        y = S.dual_reference(case, plan, relu)
        if not relu:
            S.check_plan(plan, y, (case, plan))
        elif plan == "planted":
            assert not np.isnan(y).any()


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.C3_PIXEL + S.C3_POSMAJ)
def test_conv3x3(case, plan):
    _check(plan, lambda res, relu: S.c3_reference(case, plan, res, relu), (case, plan))


@pytest.mark.parametrize("case", S.C3_POSMAJ)
def test_conv3x3_divergence_is_visible(case):
    ops, plain, skipped = S.c3_divergence(case, False)
    pad00 = S.c3_padding_taps(case[1], case[2], case[5])[:, :, 0, 0]
    assert np.isnan(plain[:, pad00, 5]).all() and np.isfinite(skipped[:, pad00, 5]).all()
    assert pad00.any() and not pad00.all()
    S.compare(plain[:, ~pad00], skipped[:, ~pad00])
    assert not np.isfinite(plain[:, ~pad00, 5]).all(), "the +inf weight reaches the outputs where its tap is inside the image"


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.EXPAND)
def test_expand(case, plan):
    _check(plan, lambda res, relu: S.expand_reference(case, plan, res, relu)[1], (case, plan), can_nan=_fused_nan(case))
    mid = S.expand_reference(case, plan, True, False)[0]
    _mid_conditions(plan, mid, S.expand_operands(case, plan, True), case[4])


def _fused_nan(case):
    """Overflowing fused pairs: the mid activation overflows at a few elements, and two of them in one pixel meet as inf - inf in the expansion.
    A case of ONE pixel may or may not hold such a pair."""
    return True if case[0] * case[1] * case[2] > 1 else None


def _mid_conditions(plan, mid, ops, stride):
    if plan == "planted" and ops[0].size > ops[0].shape[-1]:
        # a NaN of conv2 met the inner ReLU: the mid activation is 0 there and the output finite
        x, w2, b2 = ops[:3]
        raw = S.O.conv3x3_nhwc(x, w2, b2, stride, None, False)
        hit = np.isnan(raw)
        assert hit.any() and (mid[hit] == 0).all()
    if plan.startswith("subnormal"):
        a = np.abs(mid[mid != 0])
        assert a.size and (a < S.TINY).all() or plan == "subnormal_products"


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.EXPAND_DUAL)
def test_expand_dual(case, plan):
    for relu in (True, False):
        mid, y = S.expand_dual_reference(case, plan, relu)
        if not relu:
            S.check_plan(plan, y, (case, plan), can_nan=_fused_nan(case))
        elif plan == "planted":
            assert not np.isnan(y).any()
    ops = S.expand_dual_operands(case, plan)
    _mid_conditions(plan, mid, ops[:3], 1)


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.EXPAND128)
def test_expand128(case, plan):
    _check(plan, lambda res, relu: S.e128_reference(case, plan, res, relu)[1], (case, plan), can_nan=_fused_nan(case))
    _mid_conditions(plan, S.e128_reference(case, plan, True, False)[0], S.e128_operands(case, plan, True), 1)


@pytest.mark.parametrize("case", S.STEM)
def test_stem_planted(case):
    """Behind the ReLU and the pool: a planted value shows as +inf or as a 0 that the base data does not have there; every launch of the GPU
    test (one site, all sites) differs from the finite base output, and only near its site."""
    base = S.O.stem7x7_pool_nhwc(*S.stem_base(*case))
    assert np.isfinite(base).all() and np.array_equal(S.bits(S.stem_model(*S.stem_base(*case))), S.bits(base))
    sites = S.stem_sites(*case)
    cols = {c for _, _, c in sites}
    assert {0, 4, case[2] - 1} <= cols and any(c % 2 for c in cols - {case[2] - 1}) and any(c % 2 == 0 and c > 4 for c in cols)
    assert any(r == 0 for _, r, _ in sites) and any(r == case[1] - 1 for _, r, _ in sites)
    assert case[2] <= 224 or {223, 224} <= cols
    for value in S.STEM_VALUES:
        for ch in range(3):
            for site in [None] + list(range(len(sites))):
                y = S.stem_reference(case, value, ch, site)
                plain = S.O.stem7x7_pool_nhwc(*S.stem_planted(case, value, ch, site))
                assert np.array_equal(S.bits(S.stem_reference(case, value, ch, site, slot=False)), S.bits(plain)), "the model without the slot is the oracle"
                # the slot term shows for channel 0 in an even column c >= 4, where it zeroes conv column (c - 4) / 2 as well, and nowhere else
                shows = ch == 0 and any(c % 2 == 0 and c >= 4 for _, _, c in (sites if site is None else [sites[site]]))
                assert np.array_equal(S.bits(y), S.bits(plain)) != shows, (case, value, ch, site)
                assert not np.isnan(y).any() and (y >= 0).all()
                diff = np.argwhere(S.bits(y) != S.bits(base))
                assert len(diff), (case, value, ch, site)
                if site is not None:
                    i, r, c = sites[site]
                    assert (diff[:, 0] == i).all() and (np.abs(diff[:, 1] - r // 4) <= 2).all() and (np.abs(diff[:, 2] - c // 4) <= 2).all()
                if value != "nan":
                    assert np.isinf(y).any(), (case, value, ch, site)


@pytest.mark.parametrize("plan", S.PLANS[1:])
@pytest.mark.parametrize("case", S.STEM)
def test_stem_scaled(case, plan):
    base = S.O.stem7x7_pool_nhwc(*S.stem_base(*case))
    S.check_plan(plan, S.stem_scaled_reference(case, plan), (case, plan), signed=False, can_nan=False, ignore=base == 0)


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.POOL)
def test_pool(case, plan):
    y = S.pool_reference(case, plan)
    assert not np.isnan(y).any()
    if plan == "planted":
        assert np.isinf(y).any()
        if case[1] >= 7:
            assert y[0, 1, 1, 0] == 0, "a NaN alone among negative values gives 0"
            assert y[0, 2, 2, 1] == F(5) + S.pool_operands(case, plan)[1][1]
    elif case[1] >= 7:
        S.check_plan(plan, y, (case, plan), signed=False, can_nan=False, ignore=S.pool_base_reference(case) == 0)


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.BIAS_ACT)
def test_bias_act(case, plan):
    for res in (True, False):
        y = S.bias_act_reference(case, plan, res, False)
        if plan == "planted":
            S.check_plan(plan, y, (case, plan, res))
            assert not np.isnan(S.bias_act_reference(case, plan, res, True)).any()
        elif plan == "overflowing":
            s = S.stats(y)
            assert s["finite"] * 4 >= s["n"] and (s["pinf"] or s["ninf"] or not res), (case, s)
        else:
            S.check_plan(plan, y, (case, plan, res))


@pytest.mark.parametrize("name", S.ALEX)
def test_alex_conv2d_planted(name):
    S.check_plan("planted", S.alex_reference(name, False), name)
    y = S.alex_reference(name, True)
    assert not np.isnan(y).any() and np.isinf(y).any()


# ---- the backward kernels: the model's own arithmetic (numpy float32 adds, oracle chains) is IEEE on these values -------------------------------
def _all(parts):
    return np.concatenate([np.asarray(p, F).reshape(-1) for p in parts])


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("name", list(S.WGRAD))
def test_wgrad(name, plan):
    """One chain per output: an overflowing chain of finite terms cannot give NaN (can_nan = False asserts there is none)."""
    dw, db = S.wgrad_reference(name, plan)
    live = dw[:, :-1] if name == "1x1_short_and_empty_split" else dw                  # the last split is empty: zeros by construction
    S.check_plan(plan, live, (name, plan), can_nan=False)
    if name == "1x1_short_and_empty_split":
        assert not dw[:, -1].any()
    if plan == "planted" and name.startswith("3x3"):
        assert np.isnan(dw[0, 0, 0, 0]).all() and np.isinf(dw[0, 0, 0, 4, 3:]).all(), "a non-finite dz under a padding tap gives NaN"


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("M,Cin,Cout", S.DGRAD1)
def test_dgrad1x1(M, Cin, Cout, plan):
    for with_add, with_mask in S.flags(plan):
        y = S.dgrad1_reference(M, Cin, Cout, plan, with_add, with_mask)
        if plan != "planted" or not with_mask:
            S.check_plan(plan, y, (M, plan, with_add), can_nan=False)
        else:
            assert (y[0, 5:7] == 0).all() and np.isnan(S.dgrad1_reference(M, Cin, Cout, plan, with_add, False)[0, 5:7]).all(), "a NaN in the mask selects 0"
        if plan == "subnormal_products" and not with_add:
            # the data holds chains that end on -0: what the + (+0) of the epilogue's absent bias turns into +0 (S.zero_fill_term)
            neg0 = lambda v: int((S.bits(v) == 0x80000000).sum())
            assert neg0(S.dgrad1_reference(M, Cin, Cout, plan, False, False, raw=True)) >= 1 and neg0(y) == 0


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("name", S.DGRAD3)
def test_dgrad3x3(name, plan):
    S.check_plan(plan, S.dgrad3_reference(name, plan, False), (name, plan), can_nan=False)
    y = S.dgrad3_reference(name, plan, True)
    if plan == "planted":
        assert y[0, 0, 0, 0] == 0 and y[0, 0, 0, 2] == 0


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.COL2IM)
def test_col2im(case, plan):
    y = S.col2im_reference(case, plan, False)
    if plan == "overflowing" and case[1] <= 2 and case[2] <= 2:
        assert np.isfinite(y).all() and y.all(), "one tap per input pixel: nothing is added, nothing can overflow"
    else:
        S.check_plan(plan, y, (case, plan), can_nan=False)


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("n", S.RELU_N)
def test_relu_grad(n, plan):
    """The kernel selects and computes nothing: nothing can overflow.  The subnormal plans must let a subnormal positive y pass dy."""
    z = S.relu_reference(n, plan)
    dy, y = S.relu_operands(n, plan)
    if plan == "planted":
        S.check_plan(plan, z, (n, plan))
        assert z[2] == 0 and z[3] == S.NINF and z[6] == 0 and z[n - 1] == S.NINF
    else:
        assert np.isfinite(z).all() and (z != 0).sum() * 4 >= n
        if plan.startswith("subnormal"):
            assert (np.abs(y[y != 0]) < S.TINY).all() and (np.abs(z[z != 0]) < S.TINY).all()


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.FOLD)
def test_fold_backward(case, plan):
    gw, gg, gb = S.fold_reference(case, plan)
    if plan == "planted":
        S.check_plan(plan, _all((gw, gg, gb)), (case, plan))
        assert np.isnan(gw[0, 0, 0, 0]) and np.isnan(gg[0, 0]) and np.isinf(gb[0, 3]) and np.isnan(gb[0, 4])
    elif plan == "overflowing":
        S.check_plan(plan, _all((gw, gg, gb)), (case, plan), can_nan=None)
    else:
        # subnormal_inputs: d = sum of the partials, gw = d * scale and gbeta are subnormal; subnormal_products: the PRODUCTS d w of the dot
        # product are, so ggamma (and gbeta) -- gw = d * scale is normal by construction
        S.check_plan(plan, _all((gw, gb) if plan == "subnormal_inputs" else (gg, gb)), (case, plan))
