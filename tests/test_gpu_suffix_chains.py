"""The trunk suffix's backward kernels (csrc/backward.hip, the non-FOLD path of csrc/wgrad_kernel.hpp, the kEpiMaskedGrad epilogue of csrc/gemm.hip,
the GRAD path of csrc/conv.hip) pinned to their documented sums, BIT FOR BIT, through the C ABI: every comparison is array_equal / torch.equal
against tests/_suffix_model.py (oracle.cosine_sim's k-ordered fmaf chains and unfused numpy float32 arithmetic).  tests/test_suffix_model.py shows
that the model is the operation (float64) and that, on the data used here, a split cut elsewhere, another order of the pixels, the partials or the
taps, a clamped border, a fused or re-associated chain rule or a mask with >= would change the bits.  Every output lies between guard rows of a
sentinel and starts as NaN.  The shapes are the smallest that reach each path and each boundary (lists in _suffix_model.py)."""
import numpy as np
import pytest
import torch

import _suffix_model as model

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
NAN = float("nan")
GUARD = 256                                       # floats: the guarded body stays 16-B aligned


def _lib():
    from isx._lib import check, lib
    return lib(), check, torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()          # a copy: the shared cases stay read-only


def _host(t):
    return t.cpu().numpy()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _guarded(*shape):
    """(buffer, body): GUARD floats of the sentinel, the body of `shape` filled with NaN, GUARD floats of the sentinel."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
    buf[GUARD:GUARD + n] = NAN
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _same(got, want, what):
    got = _host(got) if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()), float(np.nanmax(np.abs(got - want))), int(np.isnan(got).sum()))


# ---- isx_conv_wgrad_nhwc ----------------------------------------------------------------------------------------------------------------------
def _wgrad_shape(name):
    g, Cin, Cout, leaves, which = model.WGRAD_CASES[name]
    K = model.wgrad_K(name)
    S = _lib()[0].isx_conv_wgrad_splits(K, Cin, Cout, g.taps)
    assert S >= 1
    return g, Cin, Cout, leaves, which, K, S


def _wgrad(dz, x, B, leaves, g, Cin, Cout, S, with_db=True):
    L, check, st = _lib()
    wbuf, dw = _guarded(leaves, S, Cout, g.taps, Cin)
    bbuf, db = _guarded(leaves, S, Cout)
    check(L.isx_conv_wgrad_nhwc(_ptr(dz), _ptr(x), B, leaves, g.H, g.W, Cin, Cout, g.taps, g.stride, dw.data_ptr(), db.data_ptr() if with_db else None, st),
          "isx_conv_wgrad_nhwc")
    assert _guards_intact(wbuf) and _guards_intact(bbuf)
    if not with_db:
        assert bool(torch.isnan(db).all())
    return dw, db


def test_wgrad_split_rule_and_tile_dispatch_are_the_librarys():
    """For the case shapes and the real layer4 shapes: with S = isx_conv_wgrad_splits the model's kt_per = ceil(nk / S) k-tiles per split cover the
    leaf, the ranges are consecutive, and the empty splits are the trailing ones past ceil(nk / kt_per).  The two `big` cases are the smallest
    launches the dispatch of isx_conv_wgrad_nhwc sends to the 128x128 tile: (Cout / 128)(Cin / 128) taps leaves S reaches 512 with the last leaf."""
    L = _lib()[0]
    shapes = [(model.wgrad_K(n),) + model.WGRAD_CASES[n][1:3] + (model.WGRAD_CASES[n][0].taps,) for n in model.WGRAD_CASES] + list(model.LAYER4_SHAPES)
    for K, Cin, Cout, taps in shapes:
        S = L.isx_conv_wgrad_splits(K, Cin, Cout, taps)
        assert S >= 1, (K, Cin, Cout, taps)
        kt_per, ranges = model.split_ranges(K, S)
        nk = (K + 31) // 32
        assert kt_per * S >= nk > kt_per * S - S and ranges[0][0] == 0 and ranges[-1][1] == K and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
        used = (nk + kt_per - 1) // kt_per
        assert [hi > lo for lo, hi in ranges] == [s < used for s in range(S)], (K, Cin, Cout, taps, S)
    for name in model.WGRAD_BIG:
        g, Cin, Cout, leaves, _, K, S = _wgrad_shape(name)
        per_leaf = (Cout // 128) * (Cin // 128) * g.taps * S
        assert Cout % 128 == 0 and Cin % 128 == 0 and per_leaf * leaves >= 512 > per_leaf * (leaves - 1), name
    assert _wgrad_shape("1x1_short_and_empty_split")[5:] == (1300, 10) and _wgrad_shape("big_3x3")[5:] == (272, 2) and _wgrad_shape("big_1x1_stride2")[5:] == (1147, 8)


@pytest.mark.parametrize("name", model.WGRAD_CASES)
def test_wgrad_partials_are_the_split_chains(name):
    """dw[l][s] and db[l][s] of the launch against the model (the `big` cases: the first and the last leaf); every leaf of a launch of several equal
    to the launch of that leaf alone -- for the `big` cases, whose single leaves take the 64x64 tile, also the statement that the tile shape does
    not change the bits; db = NULL accepted and dw unchanged by it."""
    g, Cin, Cout, leaves, which, K, S = _wgrad_shape(name)
    dz_np, x_np = model.wgrad_inputs(name)
    want_dw, want_db = model.wgrad_case(name, S)
    dz, x = _dev(dz_np), _dev(x_np)
    dw, db = _wgrad(dz, x, g.B, leaves, g, Cin, Cout, S)
    for i, l in enumerate(range(leaves) if which is None else which):
        _same(dw[l], want_dw[i], (name, "dw", l))
        _same(db[l], want_db[i], (name, "db", l))
    if leaves > 1:
        per, rows_in = g.B // leaves, g.B // leaves * g.H * g.W
        for l in range(leaves):
            one_dw, one_db = _wgrad(dz[l * K:(l + 1) * K].clone(), x[l * rows_in:(l + 1) * rows_in].clone(), per, 1, g, Cin, Cout, S)
            assert torch.equal(one_dw[0], dw[l]) and torch.equal(one_db[0], db[l]), (name, l)
    no_db, _ = _wgrad(dz, x, g.B, leaves, g, Cin, Cout, S, with_db=False)
    assert torch.equal(no_db, dw), name


# ---- isx_bn_fold_backward ----------------------------------------------------------------------------------------------------------------------
def _fold(dwp, db, w, scale, mean, istd, taps, prior=None):
    """The three gradients of every leaf live in one flat (leaves, total) buffer of the sentinel, at offsets that leave unrelated columns in front
    of, between and behind them; leaf l at + l * total floats (leaf_stride; 0 for one leaf).  prior None: accumulate = 0 over NaN; else
    accumulate = 1 onto the priors.  Returns (gw, ggamma, gbeta) after checking that no other column was touched."""
    L, check, st = _lib()
    leaves, S, Cout, _, Cin = dwp.shape
    n = Cout * Cin * taps
    o_gw, o_gg, o_gb = 7, 7 + n + 5, 7 + n + 5 + Cout + 3
    total = o_gb + Cout + 9
    buf = torch.full((leaves + 2, total), SENTINEL, device="cuda")
    flat = buf[1:leaves + 1]
    own = torch.zeros(total, dtype=torch.bool, device="cuda")
    for i, (o, m) in enumerate(((o_gw, n), (o_gg, Cout), (o_gb, Cout))):
        own[o:o + m] = True
        flat[:, o:o + m] = NAN if prior is None else _dev(prior[i]).reshape(leaves, m)
    base = flat.data_ptr()
    check(L.isx_bn_fold_backward(dwp.data_ptr(), db.data_ptr(), leaves, S, w.data_ptr(), scale.data_ptr(), mean.data_ptr(), istd.data_ptr(), Cout, Cin, taps,
                                 0 if prior is None else 1, total if leaves > 1 else 0, base + 4 * o_gw, base + 4 * o_gg, base + 4 * o_gb, st), "isx_bn_fold_backward")
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()) and bool((flat[:, ~own] == SENTINEL).all())
    return flat[:, o_gw:o_gw + n].reshape(leaves, Cout, Cin, taps), flat[:, o_gg:o_gg + Cout], flat[:, o_gb:o_gb + Cout]


@pytest.mark.parametrize("taps,Cin,leaves,S", model.FOLD_CASES)
def test_fold_backward_is_the_documented_sum(taps, Cin, leaves, S):
    """Partials in split order, gw = d * scale, dot over the parameter layout (LDS path) or the partial layout (direct path) through the fixed block
    reduction, ggamma = (dot - mean * dbs) * istd, gbeta = dbs: written over NaN, and added onto seeded priors."""
    dwp, db, prior, plain, acc = model.fold_case(taps, Cin, leaves, S)
    dev = [_dev(a) for a in (dwp, db) + model.fold_params(taps, Cin)]
    for pri, want in ((None, plain), (prior, acc)):
        got = _fold(*dev, taps, prior=pri)
        for g_, w_, what in zip(got, want, ("gw", "ggamma", "gbeta")):
            _same(g_.contiguous(), w_, (what, "accumulate" if pri else "write"))


@pytest.mark.parametrize("name", ["1x1_short_and_empty_split", "3x3_three_leaves"])
def test_wgrad_into_fold_backward(name):
    """The chain the engine runs: the partials of isx_conv_wgrad_nhwc fed to isx_bn_fold_backward, on the GPU and in the model: equal bits for gw,
    ggamma and gbeta (ten partials, the last one zeros; three leaves of two)."""
    g, Cin, Cout, leaves, _, K, S = _wgrad_shape(name)
    dz_np, x_np = model.wgrad_inputs(name)
    params = model.fold_params(g.taps, Cin, Cout)
    want = model.fold_backward(*model.wgrad_case(name, S), *params, g.taps)
    dw, db = _wgrad(_dev(dz_np), _dev(x_np), g.B, leaves, g, Cin, Cout, S)
    got = _fold(dw.contiguous(), db.contiguous(), *[_dev(a) for a in params], g.taps)
    for g_, w_, what in zip(got, want, ("gw", "ggamma", "gbeta")):
        _same(g_.contiguous(), w_, (name, what))


# ---- isx_conv1x1_dgrad_nhwc ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", model.DGRAD1_M)
@pytest.mark.parametrize("Cin", model.DGRAD1_CIN)
@pytest.mark.parametrize("Cout", model.DGRAD1_COUT)
def test_dgrad1x1_is_one_chain_then_add_then_mask(Cout, Cin, M):
    """Each of add and mask present and absent, under every tile shape of the GEMM (isx_debug_set_gemm_cfg 0 .. 3: 128x128 with k-tiles of 16,
    64x128, 128x64, 64x64 with k-tiles of 32) and under the automatic choice: all the model's bits.  The reduction runs over Cout: 80 is no multiple of
    32 (the unaligned loads of the k-tile-32 shapes, a zero-filled last k-tile; the 128x128 shape's k-tiles of 16 divide it); Cin = 100 clips the last
    column tile."""
    L, check, st = _lib()
    dz_np, wt_np, add_np, mask_np, _ = model.dgrad1_case(Cin, Cout)
    dz, wt, add, mask = _dev(dz_np[:M]), _dev(wt_np), _dev(add_np[:M]), _dev(mask_np[:M])
    try:
        for with_add in (False, True):
            for with_mask in (False, True):
                want = model.dgrad1_want(Cin, Cout, M, with_add, with_mask)
                for cfg in (0, 1, 2, 3, -1):
                    L.isx_debug_set_gemm_cfg(cfg)
                    buf, dx = _guarded(M, Cin)
                    check(L.isx_conv1x1_dgrad_nhwc(dz.data_ptr(), M, Cout, wt.data_ptr(), Cin, add.data_ptr() if with_add else None,
                                                   mask.data_ptr() if with_mask else None, dx.data_ptr(), st), "isx_conv1x1_dgrad_nhwc")
                    assert _guards_intact(buf)
                    _same(dx, want, ("add" if with_add else "", "mask" if with_mask else "", cfg))
    finally:
        L.isx_debug_set_gemm_cfg(-1)


# ---- isx_conv3x3_dgrad_nhwc -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", model.DGRAD3_CASES)
def test_dgrad3x3_is_one_chain_over_the_neighbourhood(name):
    """One chain of 9 * Cout terms in (kh, kw, co) order over the zero-padded neighbourhood, then the mask; with and without mask (a call without
    mask used to take the inference kernel's two-level sum: the gradient instance is now chosen by the entry, not by the mask).  This entry has no
    tile hook: by pick_tile_cfg (restated in _suffix_model.py; tests/test_suffix_engine_model.py asserts what follows on the CPU) every case here
    (up to 144 pixels x 96 channels, a fraction of one round of the chip) takes the 64x64 tile -- and so do layer4's launches in the whole-step
    tests (tests/test_gpu_suffix.py: 1176 x 512 for one leaf, 9408 x 512 for eight).  The 128x128 instance of the GRAD path is chosen from
    38 913 pixels x 512 channels on (77 825 x 256, 155 649 x 128).  Two tests run it, both against dgrad3x3 of this model: the case of
    tests/test_gpu_large_tensors.py (171 199 images of 7 x 7 = 8 388 751 pixels x 256 channels, its period rows compared) and the one of
    tests/test_gpu_suffix_engine.py at the first such row count (38 913 x 512: the last tile has one live row).  The 128x64 instance is never
    chosen for 64 .. 2048 channels and up to 3 000 000 pixels: under the automatic choice no test can reach it."""
    L, check, st = _lib()
    B, H, W, Cout, Cin, _ = model.DGRAD3_CASES[name]
    dz_np, wt_np, mask_np, v = model.dgrad3_case(name)
    dz, wt, mask = _dev(dz_np), _dev(wt_np), _dev(mask_np)
    for m, want in ((mask, model.masked(v, mask_np)), (None, v)):
        buf, dx = _guarded(B, H, W, Cin)
        check(L.isx_conv3x3_dgrad_nhwc(dz.data_ptr(), B, H, W, Cout, wt.data_ptr(), Cin, _ptr(m), dx.data_ptr(), st), "isx_conv3x3_dgrad_nhwc")
        assert _guards_intact(buf)
        _same(dx, want, (name, m is not None))


# ---- isx_conv3x3_s2_col2im_nhwc -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin", model.COL2IM_CASES)
def test_col2im_adds_the_taps_in_kh_kw_order(B, H, W, Cin):
    L, check, st = _lib()
    dcol_np, mask_np, v = model.col2im_case(B, H, W, Cin)
    dcol, mask = _dev(dcol_np), _dev(mask_np)
    for m, want in ((mask, model.masked(v, mask_np)), (None, v)):
        buf, dx = _guarded(B, H, W, Cin)
        check(L.isx_conv3x3_s2_col2im_nhwc(dcol.data_ptr(), B, H, W, Cin, _ptr(m), dx.data_ptr(), st), "isx_conv3x3_s2_col2im_nhwc")
        assert _guards_intact(buf)
        _same(dx, want, m is not None)


# ---- isx_relu_grad --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", model.RELU_N)
def test_relu_grad_in_place_and_out_of_place(n):
    L, check, st = _lib()
    dy_np, y_np, want = model.relu_case(n)
    y = _dev(y_np)
    buf, dz = _guarded(n)
    check(L.isx_relu_grad(_dev(dy_np).data_ptr(), y.data_ptr(), n, dz.data_ptr(), st), "isx_relu_grad")
    assert _guards_intact(buf)
    _same(dz, want, "out of place")
    buf, dy = _guarded(n)
    dy.copy_(_dev(dy_np))
    check(L.isx_relu_grad(dy.data_ptr(), y.data_ptr(), n, dy.data_ptr(), st), "isx_relu_grad")
    assert _guards_intact(buf)
    _same(dy, want, "in place")


# ---- empty problems -------------------------------------------------------------------------------------------------------------------------------
def test_empty_problems_are_no_ops():
    """M = 0, B = 0, n = 0 return ISX_OK with null pointers; a weight-gradient launch of no images (it needs dw) writes its one partial as zeros."""
    L, check, st = _lib()
    check(L.isx_conv1x1_dgrad_nhwc(None, 0, 64, None, 64, None, None, None, st), "isx_conv1x1_dgrad_nhwc")
    check(L.isx_conv3x3_dgrad_nhwc(None, 0, 7, 7, 64, None, 64, None, None, st), "isx_conv3x3_dgrad_nhwc")
    check(L.isx_conv3x3_s2_col2im_nhwc(None, 0, 7, 7, 64, None, None, st), "isx_conv3x3_s2_col2im_nhwc")
    check(L.isx_relu_grad(None, None, 0, None, st), "isx_relu_grad")
    g = model.Geom(0, 7, 7, 9, 1)
    assert L.isx_conv_wgrad_splits(0, 64, 64, 9) == 1
    dw, db = _wgrad(None, None, 0, 1, g, 64, 64, 1)
    assert not _host(dw).any() and not _host(db).any()
