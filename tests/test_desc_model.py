"""tests/_desc_model.py, the CPU model the descriptor kernels of csrc/pool.hip and csrc/region.hip are pinned to in
tests/test_gpu_desc_chains.py, checked on its own:

  * the dispatch tables (which kernel, which path) for named shapes on both sides of every boundary;
  * against float64 of the same operation, inside the bounds derived in the model's docstring: the model is the operation, not a copy of the
    kernel.  No row is left out of that comparison, and that is asserted;
  * against the oracle inside the tolerance tests/test_gpu_parity.py holds the kernels to; the locations exactly;
  * against the plausible WRONG variants, on exactly the data the GPU test runs: where the model and a wrong variant give the same bits, a
    bit-exact test says nothing about that variant.  The cases that tell each variant apart are printed (pytest -s)."""
import numpy as np
import pytest

import _desc_model as model
import oracle as O

F = np.float32
TOL = dict(rtol=2e-6, atol=2e-7)                  # tests/test_gpu_parity.py


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def row_sets():
    """(name, x, shift, aligned) of every l2norm case of the GPU test."""
    for D in model.L2_D_ALIGNED + model.L2_D_SCALAR:
        for B in model.L2_B:
            x, shift = model.row_case(B, D)
            yield "%dx%d" % (B, D), x, shift, True
    for D in model.L2_D_OFFSET:
        x, shift = model.row_case(5, D)
        yield "5x%d offset" % D, x, shift, False


# ---- dispatch tables ---------------------------------------------------------------------------------------------------------------------------------
def test_l2norm_dispatch_table():
    want = {(4, True): "wave1", (252, True): "wave1", (256, True): "wave1", (260, True): "wave2", (512, True): "wave2", (516, True): "wave4",
            (1024, True): "wave4", (1028, True): "wave8", (2044, True): "wave8", (2048, True): "wave8", (2052, True): "block_vec",
            (4100, True): "block_vec", (8196, True): "block_vec", (1, True): "block_scalar", (37, True): "block_scalar", (1023, True): "block_scalar",
            (1025, True): "block_scalar", (2049, True): "block_scalar", (256, False): "block_scalar", (2048, False): "block_scalar",
            (2052, False): "block_scalar"}
    for (D, aligned), k in want.items():
        assert model.l2norm_kernel(D, aligned) == k, (D, aligned)
    assert {model.l2norm_kernel(D, True) for D in model.L2_D_ALIGNED} == {"wave1", "wave2", "wave4", "wave8", "block_vec"}
    assert {model.l2norm_kernel(D, True) for D in model.L2_D_SCALAR} == {"block_scalar"}
    assert [b % 4 for b in model.L2_B] == [1, 1, 1] and max(model.L2_B) > 8          # one, two and three groups of four rows, the last ragged


def test_gap_dispatch_table():
    plan = model.gap_plan
    assert plan(3, 24, 49) == ("fused", 256, True)
    assert plan(2, 300, 49) == ("fused", 256, True) and -(-300 // 256) == 2          # two passes, the last ragged
    assert plan(3, 30, 15) == ("fused", 256, False)                                  # 450 floats per image: no 16-byte rows
    assert plan(2, 2048, 64) == ("fused", 128, True)                                 # even HW: stride 65, scattered staging
    assert plan(2, 2048, 196)[0] == "fallback"                                       # CP = 64 would need 32 passes
    assert plan(1, 8, 1600)[0] == "fallback"                                         # 32 channels of a 40 x 40 map exceed 52 KB
    # the same images in a launch of 511 and of 512: the 26 KB CP where it fits, the SAME path either way
    assert plan(511, 2048, 49) == ("fused", 256, True) and plan(512, 2048, 49) == ("fused", 128, True)
    assert plan(511, 512, 49) == ("fused", 256, True) and plan(512, 512, 49) == ("fused", 128, True)
    assert plan(511, 2048, 64) == plan(512, 2048, 64) == ("fused", 128, True)        # CP = 64 would not fit 16 passes: stays
    assert plan(511, 2048, 196)[0] == plan(512, 2048, 196)[0] == "fallback"
    for C in (1, 24, 300, 512, 2048, 4096, 4097):
        for HW in range(1, 260):
            assert plan(511, C, HW)[0] == plan(512, C, HW)[0] == plan(1, C, HW)[0] == plan(1 << 20, C, HW)[0], (C, HW)
    for B, C, H, W in model.GAP_NCHW:
        assert plan(B, C, H * W)[0] == ("fallback" if (C, H) in ((2048, 14), (8, 40)) else "fused")
    for C, H, W in model.GAP_BATCH:
        assert plan(3, C, H * W)[0] == plan(model.GAP_MANY, C, H * W)[0] == "fused"


def test_gap_nhwc_dispatch_table():
    want = {4: "qpt1", 2048: "qpt1", 2052: "qpt2", 4096: "qpt2", 4100: "qpt4", 8192: "qpt4", 8196: "generic", 30: "generic"}
    assert set(want) == set(model.GAP_NHWC_C)
    for C, k in want.items():
        assert model.gap_nhwc_plan(C) == k, C
    assert model.gap_nhwc_plan(2048, aligned=False) == "generic"


def test_case_data_holds_every_kind_of_row():
    x, _ = model.row_case(5, 256)
    assert model.ROW_KINDS == ("normal", "relu", "zero", "eps", "spike")
    assert (x[0] < 0).any() and (x[1] >= 0).all() and _bits(x[1, :1])[0] == 0x80000000 and not x[2].any()
    ss = (x.astype(np.float64) ** 2).sum(1)
    assert 0.5e-10 < ss[3] < 2e-10 and x[4].max() >= 1e4 and np.sort(np.abs(x[4]))[-2] < 10
    assert len(model.sqrt_sweep()) >= 65536 and np.isfinite(model.sqrt_sweep()).all()
    s = _bits(model.sqrt_sweep())
    assert set(((s >> 23) & 255).tolist()) == set(range(255)) and set((s >> 31).tolist()) == {0, 1}
    assert sorted(C * kh * kw for C, kh, kw in model.GATHER) == [36, 1020, 1024, 1028, 100352]


# ---- the model against float64 ------------------------------------------------------------------------------------------------------------------
def _inside(got, want64, bound, name):
    err = np.abs(got.astype(np.float64) - want64)
    ok = err <= bound
    assert ok.all(), (name, int((~ok).sum()), float((err / np.maximum(bound, 1e-300)).max()))
    return got.shape[0], float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def test_l2norm_lies_inside_the_row_bound():
    rows, worst = 0, 0.0
    for name, x, shift, aligned in row_sets():
        k = model.l2norm_kernel(x.shape[1], aligned)
        depth = model.ss_depth(k, x.shape[1])
        y64 = model.l2norm_rows64(x)
        n, w = _inside(model.l2norm_rows(x, aligned=aligned), y64, model.row_bound(y64, depth), name)
        ys64 = model.l2norm_rows64(x, shift=shift)
        _inside(model.l2norm_rows(x, shift=shift, aligned=aligned), ys64, model.row_bound(y64, depth, ys64), name + " shift")
        rows, worst = rows + n, max(worst, w)
    print("l2norm: %d rows, worst error / bound = %.3f" % (rows, worst))
    assert rows == (len(model.L2_D_ALIGNED) + len(model.L2_D_SCALAR)) * sum(model.L2_B) + 5 * len(model.L2_D_OFFSET) and 0 < worst <= 1       # every row compared


def test_gap_lies_inside_the_pool_and_row_bounds():
    for B, C, H, W in model.GAP_NCHW + tuple((3, C, H, W) for C, H, W in model.GAP_BATCH):
        f = model.map_case(B, C, H, W)
        name = "nchw %s" % ((B, C, H, W),)
        fused = model.gap_plan(B, C, H * W)[0] == "fused"
        p = (model.pool_in_order if fused else model.pool_lanes)(f.reshape(B, C, -1))
        _inside(p, model.pool64(f), model.pool_bound(f, fused), name + " pooled")
        y64 = model.l2norm_rows64(p)
        depth = model.ss_depth("block256" if fused else model.l2norm_kernel(C, True), C)
        _inside(model.gap_l2(f), y64, model.row_bound(y64, depth), name)
    for C in model.GAP_NHWC_C:
        for HW in model.GAP_NHWC_HW:
            f = model.map_case(2, C, HW, 1)
            m = np.ascontiguousarray(f.reshape(2, C, HW).transpose(0, 2, 1))
            p = model.pool_in_order(f.reshape(2, C, HW))
            _inside(p, model.pool64(f), model.pool_bound(f, True), "nhwc pooled")
            y64 = model.l2norm_rows64(p)
            plan = model.gap_nhwc_plan(C)
            depth = model.ss_depth(model.l2norm_kernel(C, True) if plan == "generic" else "nhwc512", C)
            _inside(model.gap_l2_nhwc(m), y64, model.row_bound(y64, depth), "nhwc %d %d" % (C, HW))


def test_best_location_and_gather_lie_inside_the_row_bound():
    for K in model.BEST_K:
        cls = model.best_case(K, 3, 2)
        d, loc = model.best_location_desc(cls)
        v = np.stack([cls[b, :, r, c] for b, (r, c) in enumerate(loc)])
        y64 = model.l2norm_rows64(v)
        _inside(d, y64, model.row_bound(y64, model.ss_depth("block256", K)), "best %d" % K)
    for C, kh, kw in model.GATHER:
        fmap, idx, Wp, shift = model.gather_case(C, kh, kw)
        for order, kernel, sh in (("chw", "block_scalar", shift), ("hwc", "gather_nhwc", model.shift_hwc(shift, C, kh, kw))):
            g, valid = model.gather_windows(fmap, kh, kw, idx, Wp, order)
            assert valid.sum() == 8 and (~valid).sum() == 4
            y64 = model.l2norm_rows64(g)
            depth = model.ss_depth(kernel, g.shape[1])
            got = model.region_gather_l2(fmap, kh, kw, idx, Wp, order=order).reshape(g.shape)
            assert not got[~valid].any() and _same_bits(got[~valid], np.zeros_like(got[~valid]))
            _inside(got[valid], y64[valid], model.row_bound(y64, depth)[valid], "gather %s %d" % (order, g.shape[1]))
            got = model.region_gather_l2(fmap, kh, kw, idx, Wp, shift=sh, order=order).reshape(g.shape)
            ys64 = y64 + sh.astype(np.float64)
            assert not got[~valid].any()
            _inside(got[valid], ys64[valid], model.row_bound(y64, depth, ys64)[valid], "gather %s %d shift" % (order, g.shape[1]))


def test_backward_lies_inside_its_bound():
    rows = 0
    for D in model.BWD_D:
        for B in model.BWD_B:
            x, dy = model.bwd_case(B, D)
            n, _ = _inside(model.l2norm_rows_bwd(x, dy), model.l2norm_rows_bwd64(x, dy), model.bwd_bound(x, dy), "bwd %dx%d" % (B, D))
            rows += n
    assert rows == sum(model.BWD_B) * len(model.BWD_D)


# ---- the model against the oracle -------------------------------------------------------------------------------------------------------------------
def test_models_agree_with_the_oracle():
    for name, x, shift, aligned in row_sets():
        np.testing.assert_allclose(model.l2norm_rows(x, aligned=aligned), O.l2norm_rows(x), err_msg=name, **TOL)
        np.testing.assert_allclose(model.l2norm_rows(x, shift=shift, aligned=aligned), O.shift_rows(O.l2norm_rows(x), shift), err_msg=name, **TOL)
    for B, C, H, W in model.GAP_NCHW + tuple((3, C, H, W) for C, H, W in model.GAP_BATCH):
        f = model.map_case(B, C, H, W)
        np.testing.assert_allclose(model.gap_l2(f), O.gap_l2(f), **TOL)
        np.testing.assert_allclose(model.gap_l2(f, B_launch=model.GAP_MANY), O.gap_l2(f), **TOL)
    for C in model.GAP_NHWC_C:
        for HW in model.GAP_NHWC_HW:
            f = model.map_case(2, C, HW, 1)
            np.testing.assert_allclose(model.gap_l2_nhwc(np.ascontiguousarray(f.reshape(2, C, HW).transpose(0, 2, 1))), O.gap_l2(f), **TOL)
    for K in model.BEST_K:
        cls = model.best_case(K, 3, 2)
        d, loc = model.best_location_desc(cls)
        for b in range(cls.shape[0]):
            od, ol = O.best_location_desc(cls[b])
            assert tuple(loc[b]) == tuple(ol), (K, b)
            np.testing.assert_allclose(d[b], od, **TOL)
        assert tuple(loc[1]) == (2, 0) and tuple(loc[2]) == (0, 1)
    for C, kh, kw in model.GATHER:
        fmap, idx, Wp, shift = model.gather_case(C, kh, kw)
        for sh in (None, shift):
            chw = model.region_gather_l2(fmap, kh, kw, idx, Wp, shift=sh)
            hwc = model.region_gather_l2(fmap, kh, kw, idx, Wp, shift=None if sh is None else model.shift_hwc(sh, C, kh, kw), order="hwc")
            for b in range(2):
                ok = np.array([0 <= i < 6 for i in idx[b]])
                want = O.region_gather_l2(fmap[b], kh, kw, idx[b][ok], Wp, sh)
                np.testing.assert_allclose(chw[b][ok], want, **TOL)
                np.testing.assert_allclose(hwc[b][ok].reshape(-1, kh, kw, C).transpose(0, 3, 1, 2).reshape(want.shape), want, **TOL)


# ---- the model discriminates ----------------------------------------------------------------------------------------------------------------------------
def _told_apart(what, pairs):
    """pairs: (case, canonical, wrong).  At least one bit of at least one case changes; prints which cases tell the variant apart."""
    hits = [case for case, a, b in pairs if not _same_bits(a, b)]
    print("%-60s told apart by %d case(s): %s" % (what, len(hits), ", ".join(hits[:6])))
    assert hits, what
    return hits


def _contiguous_partials(t, nt):
    """WRONG: thread k takes the terms [k per, (k + 1) per), per = ceil(n / nt)."""
    B, n = t.shape
    per = -(-n // nt)
    pad = np.zeros((B, per * nt), F)
    pad[:, :n] = t
    pad = pad.reshape(B, nt, per)
    v = np.zeros((B, nt), F)
    for i in range(per):
        v = v + pad[:, :, i]
    return v


def _butterfly_up(v):
    """WRONG: xor 1, 2, 4, ..., 32."""
    lanes = np.arange(model.LANES)
    for o in (1, 2, 4, 8, 16, 32):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def _block_sum_up(v):
    B, nt = v.shape
    w = _butterfly_up(v.reshape(B, nt // 64, 64))
    t = np.zeros(B, F)
    for i in range(nt // 64):
        t = t + w[:, i]
    return t


def _ss(x, kernel, contiguous=False, one_by_one=False, up=False):
    """The model's l2norm_ss with one thing read differently."""
    nt = 64 if kernel.startswith("wave") else 1024
    if kernel == "block_scalar":
        terms, one_by_one = x * x, False
    elif not one_by_one:
        terms = model.float4_terms(x)
    v = model.one_by_one_partials(x, nt) if one_by_one else (_contiguous_partials if contiguous else model.strided_partials)(terms, nt)
    if kernel.startswith("wave"):
        return (_butterfly_up if up else model.wave_butterfly)(v)
    return (_block_sum_up if up else model.block_sum)(v)


def _finish_eps_outside(x, ss, eps):
    """WRONG: sqrt(ss) + eps."""
    return x / (np.sqrt(ss) + F(eps))[:, None]


def _finish_reciprocal(x, ss, eps):
    """WRONG: x * (1 / n)."""
    return x * (F(1) / np.sqrt(ss + F(eps)))[:, None]


def _ss64(x):
    """WRONG (the oracle's way): the squares summed in float64, rounded once."""
    return (x.astype(np.float64) ** 2).sum(1).astype(F)


def test_l2norm_model_is_checked_against_itself():
    for name, x, _, aligned in row_sets():
        k = model.l2norm_kernel(x.shape[1], aligned)
        assert _same_bits(_ss(x, k), model.l2norm_ss(x, k)), name


def test_wrong_row_variants_change_bits():
    sets = list(row_sets())
    kern = [model.l2norm_kernel(x.shape[1], al) for _, x, _, al in sets]
    ss = [model.l2norm_ss(x, k) for (_, x, _, _), k in zip(sets, kern)]
    with np.errstate(all="ignore"):
        fin = [model.finish_rows(x, s, model.EPS, None, False) for (_, x, _, _), s in zip(sets, ss)]
        _told_apart("eps outside the square root", [(n, y, _finish_eps_outside(x, s, model.EPS)) for (n, x, _, _), s, y in zip(sets, ss, fin)])
        _told_apart("x * (1 / n)", [(n, y, _finish_reciprocal(x, s, model.EPS)) for (n, x, _, _), s, y in zip(sets, ss, fin)])
    _told_apart("sum of squares in float64", [(n, s, _ss64(x)) for (n, x, _, _), s in zip(sets, ss)])
    for pick, label in ((lambda k: k.startswith("wave"), "wave"), (lambda k: k == "block_vec", "block_vec"), (lambda k: k == "block_scalar", "block_scalar")):
        some = [(n, x, k, s) for (n, x, _, _), k, s in zip(sets, kern, ss) if pick(k)]
        assert some
        _told_apart("%s: contiguous split among the lanes" % label, [(n, s, _ss(x, k, contiguous=True)) for n, x, k, s in some])
        _told_apart("%s: butterfly 1 .. 32" % label, [(n, s, _ss(x, k, up=True)) for n, x, k, s in some])
        if label != "block_scalar":
            _told_apart("%s: the squares of a float4 added one by one" % label, [(n, s, _ss(x, k, one_by_one=True)) for n, x, k, s in some])
    # the three kernels are three functions: the offset rows against the aligned call, the bits of the sum and of the row
    for D in model.L2_D_OFFSET:
        x, _ = model.row_case(5, D)
        assert not _same_bits(model.l2norm_ss(x, model.l2norm_kernel(D, True)), model.l2norm_ss(x, "block_scalar")), D
        assert not _same_bits(model.l2norm_rows(x, aligned=True), model.l2norm_rows(x, aligned=False)), D
    # the signed zero: -0 in front of the post-ReLU row stays -0 in the wave kernel and becomes +0 in the scalar one
    x, shift = model.row_case(5, 256)
    assert _bits(model.l2norm_rows(x)[1, :1])[0] == 0x80000000 and _bits(model.l2norm_rows(x, aligned=False)[1, :1])[0] == 0


def test_wrong_gather_variants_change_bits():
    pairs_grouped, pairs_chw = [], []
    for C, kh, kw in model.GATHER:
        fmap, idx, Wp, _ = model.gather_case(C, kh, kw)
        g, valid = model.gather_windows(fmap, kh, kw, idx, Wp, "hwc")
        name = "F=%d" % g.shape[1]
        pairs_grouped.append((name, model.gather_nhwc_ss(g[valid]), model.block_sum(model.strided_partials(model.float4_terms(g[valid]), 1024))))
        c, _ = model.gather_windows(fmap, kh, kw, idx, Wp, "chw")
        pairs_chw.append((name, model.block_sum(model.strided_partials(c[valid] * c[valid], 1024)), model.gather_nhwc_ss(c[valid])))
    _told_apart("NHWC gather: the four squares grouped into one term", pairs_grouped)
    _told_apart("NCHW gather: float4s with one-by-one squares", pairs_chw)


def _gap_ss_by_passes(pooled, CP):
    """WRONG since the sum of squares was made independent of CP (and what the kernel did before): thread t < CP accumulates the squares of
    channels p CP + t over the passes p."""
    return model.block_sum(np.concatenate([model.strided_partials(pooled * pooled, CP), np.zeros((pooled.shape[0], 256 - CP), F)], 1))


def test_wrong_gap_variants_change_bits():
    fused = [(B, C, H, W) for B, C, H, W in model.GAP_NCHW + tuple((3, C, H, W) for C, H, W in model.GAP_BATCH)
             if model.gap_plan(B, C, H * W)[0] == "fused"]
    pooled = {s: model.pool_in_order(model.map_case(*s).reshape(s[0], s[1], -1)) for s in fused}
    for s, p in pooled.items():
        assert _same_bits(_gap_ss_by_passes(p, 256), model.gap_ss(p)), s                          # CP = 256 IS the canonical order
    _told_apart("gap_l2: CP = 128 read as CP = 256 (sum of squares)", [(str(s), model.gap_ss(p), _gap_ss_by_passes(p, 128)) for s, p in pooled.items()])
    _told_apart("gap_l2: CP = 128 read as CP = 256 (descriptor)",
                [(str(s), model.finish_rows(p, model.gap_ss(p), model.EPS, None, False), model.finish_rows(p, _gap_ss_by_passes(p, 128), model.EPS, None, False))
                 for s, p in pooled.items()])
    for C, H, W in model.GAP_BATCH:                                                               # every batch-independence shape tells it on its own
        p = pooled[(3, C, H, W)]
        assert not _same_bits(model.gap_ss(p), _gap_ss_by_passes(p, 128)), (C, H, W)
    fallback = [s for s in model.GAP_NCHW if model.gap_plan(s[0], s[1], s[2] * s[3])[0] == "fallback"]
    assert len(fallback) == 2
    _told_apart("gap_l2 fallback: butterfly pooling read as in-order pooling",
                [(str(s), model.pool_lanes(model.map_case(*s).reshape(s[0], s[1], -1)), model.pool_in_order(model.map_case(*s).reshape(s[0], s[1], -1))) for s in fallback])
    # the two layouts: equal pooled values, another sum of squares (isx.h says so)
    pairs = []
    for C in (2048, 4096, 8192):
        p = model.pool_in_order(model.map_case(2, C, 49, 1).reshape(2, C, 49))
        pairs.append(("C=%d" % C, model.gap_ss(p), model.gap_nhwc_ss(p)))
    _told_apart("gap_l2: the NHWC sum of squares read as the NCHW one", pairs)


def test_wrong_backward_variants_change_bits():
    pairs_div = []
    for D in model.BWD_D:
        for B in model.BWD_B:
            x, dy = (np.asarray(a) for a in model.bwd_case(B, D))
            got = model.l2norm_rows_bwd(x, dy)
            # c summed before n2: two independent sums, the same function
            c = model.block_sum(model.strided_partials(x * dy, 1024))
            n2 = model.block_sum(model.strided_partials(x * x, 1024)) + F(model.EPS)
            assert _same_bits(got, (n2[:, None] * dy - x * c[:, None]) * (F(1) / (n2 * np.sqrt(n2)))[:, None])
            pairs_div.append(("%dx%d" % (B, D), got, (n2[:, None] * dy - x * c[:, None]) / (n2 * np.sqrt(n2))[:, None]))
    _told_apart("backward: a division in place of the reciprocal multiply", pairs_div)


@pytest.mark.parametrize("eps", [0.0, 1e-10])
def test_sqrt_sweep_is_well_defined_on_the_host(eps):
    """What the GPU sweep compares with: numpy's float32 sqrt and division of single-element rows against float64 rounded once (both are
    correctly rounded operations; the double rounding through float64 is innocuous for one sqrt or one division of float32 operands)."""
    x = model.sqrt_sweep()
    with np.errstate(all="ignore"):
        ss = x * x + F(eps)
        n = np.sqrt(ss)
        assert _same_bits(n, np.sqrt(ss.astype(np.float64)).astype(F))
        y = x / n
        want = (x.astype(np.float64) / n.astype(np.float64)).astype(F)
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(y), ~ok) and _same_bits(y[ok], want[ok])
    assert np.isinf(y).any() == (eps == 0.0) and (y == 0).any() and (np.abs(y) == 1).any()
