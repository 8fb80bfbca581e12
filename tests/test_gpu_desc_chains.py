"""The kernels that produce the descriptor itself (csrc/pool.hip: L2 rows with and without Shift, their backward, global average pool + L2 in
both layouts; csrc/region.hip: best-location descriptor and window gather + L2 in both layouts) pinned to their documented sums, BIT FOR BIT,
through the C ABI: every comparison of a result is on the bit patterns, so that a zero of the wrong sign shows, against tests/_desc_model.py
(unfused numpy float32 arithmetic in the kernels' order).  tests/test_desc_model.py shows that the model is the operation (float64, the oracle)
and that, on the data used here, another order of the sum, eps outside the root, a reciprocal multiply or another reading of the launcher's
rules would change the bits.  The first test sweeps the device's sqrtf and division, which everything else here relies on.  Not run here: the
non-temporal variant of the NHWC pooling kernel, which needs a map above 192 MB -- the same arithmetic with other load instructions, run by
every step of bench.py.

Every output is a body of NaN (int64: a poison value) between guards of 256 sentinels; the guards are checked after every launch.  Every
operand lies inside a larger live allocation, 1 KB from its start (or 1 KB + one float where a test is about alignment)."""
import numpy as np
import pytest
import torch

import _desc_model as model

pytestmark = pytest.mark.gpu

F = np.float32
SENTINEL = -12345.0
NAN = float("nan")
GUARD = 256
POISON = -(1 << 62)
EPS = model.EPS
TOL = dict(rtol=2e-6, atol=2e-7)                  # tests/test_gpu_parity.py


def _lib():
    from isx._lib import check, lib
    return lib(), check, torch.cuda.current_stream().cuda_stream


def _dev(a, off=0, dtype=np.float32):
    """A copy of `a` inside a larger allocation filled with the sentinel, GUARD + off elements from its start."""
    a = np.asarray(a, dtype=dtype)
    flat = torch.from_numpy(np.array(a).reshape(-1))
    buf = torch.full((a.size + 2 * GUARD + off,), SENTINEL if flat.dtype == torch.float32 else int(SENTINEL), device="cuda", dtype=flat.dtype)
    body = buf[GUARD + off:GUARD + off + a.size]
    body.copy_(flat)
    return body.view(*a.shape)


def _guarded(*shape, off=0):
    """(buffer, body): GUARD floats of the sentinel (+ off), the body of `shape` filled with NaN, GUARD floats of the sentinel."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + off,), SENTINEL, device="cuda")
    buf[GUARD + off:GUARD + off + n] = NAN
    return buf, buf[GUARD + off:GUARD + off + n].view(*shape)


def _guarded_i64(n):
    buf = torch.full((n + 2 * GUARD,), int(SENTINEL), device="cuda", dtype=torch.int64)
    buf[GUARD:GUARD + n] = POISON
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, body):
    s = int(SENTINEL) if buf.dtype == torch.int64 else SENTINEL
    lo = (body.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool((buf[:lo] == s).all()) and bool((buf[lo + body.numel():] == s).all())


def _bits(x):
    return np.ascontiguousarray(x, F).view(np.uint32)


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _assert_bits(got, want, what):
    got, want = _host(got), _host(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


def _differ(a, b):
    return bool((_bits(_host(a)) != _bits(_host(b))).any())


# ---- isx_l2norm_rows / isx_l2norm_shift_rows -------------------------------------------------------------------------------------------------------
def _l2norm(x, shift=None, eps=EPS, y_off=0, in_place=False):
    L, check, st = _lib()
    B, D = x.shape
    if in_place:
        buf, y = None, x
    else:
        buf, y = _guarded(B, D, off=y_off)
    if shift is None:
        check(L.isx_l2norm_rows(x.data_ptr(), B, D, eps, y.data_ptr(), st), "isx_l2norm_rows")
    else:
        check(L.isx_l2norm_shift_rows(x.data_ptr(), shift.data_ptr(), B, D, eps, y.data_ptr(), st), "isx_l2norm_shift_rows")
    assert buf is None or _guards_intact(buf, y)
    return y


@pytest.mark.parametrize("eps", [0.0, 1e-10])
def test_device_sqrt_and_division_are_correctly_rounded(eps):
    """65 790 single-element rows -- both signs, every exponent from the denormals to 2^127, 129 mantissas -- through isx_l2norm_rows:
    y = x / sqrtf(x * x + eps) against numpy's correctly rounded float32 operations.  NaN (0 / 0 at eps = 0) must be NaN; its payload is free."""
    x = model.sqrt_sweep()[:, None]
    want = model.l2norm_rows(x, eps)
    got = _l2norm(_dev(x), eps=eps).cpu().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and nan.sum() == (2 if eps == 0.0 else 0)
    _assert_bits(got[~nan], want[~nan], "x / sqrt(x * x + eps)")


@pytest.mark.parametrize("D", model.L2_D_ALIGNED + model.L2_D_SCALAR)
def test_l2norm_rows_are_the_documented_sums(D):
    """Out of place against the model of the kernel that (D, alignment) selects; in place (y == x) the same bits."""
    for B in model.L2_B:
        x, shift = model.row_case(B, D)
        dshift = _dev(shift)
        for sh, dsh in ((None, None), (shift, dshift)):
            got = _l2norm(_dev(x), dsh)
            _assert_bits(got, model.l2norm_rows(x, shift=sh), (B, D, sh is not None))
            buf, body = _guarded(B, D)
            body.copy_(torch.from_numpy(np.array(x)))
            _l2norm(body, dsh, in_place=True)
            assert _guards_intact(buf, body)
            _assert_bits(body, got, ("in place", B, D, sh is not None))


def test_l2norm_shift_with_no_shift_is_l2norm_rows():
    L, check, st = _lib()
    for D in (256, 2052, 37):
        x, _ = model.row_case(5, D)
        dx = _dev(x)
        buf, y = _guarded(5, D)
        check(L.isx_l2norm_shift_rows(dx.data_ptr(), None, 5, D, EPS, y.data_ptr(), st), "isx_l2norm_shift_rows")
        assert _guards_intact(buf, y)
        _assert_bits(y, _l2norm(dx), D)


@pytest.mark.parametrize("D", model.L2_D_OFFSET)
def test_l2norm_at_an_offset_of_one_float_takes_the_scalar_kernel(D):
    """x, y or the Shift one float off a 16-byte boundary: the scalar kernel's bits, which are not the aligned call's."""
    x, shift = model.row_case(5, D)
    aligned = _l2norm(_dev(x))
    _assert_bits(aligned, model.l2norm_rows(x), "aligned")
    scalar = model.l2norm_rows(x, aligned=False)
    assert _differ(aligned, scalar)
    _assert_bits(_l2norm(_dev(x, off=1)), scalar, "x off")
    _assert_bits(_l2norm(_dev(x), y_off=1), scalar, "y off")
    _assert_bits(_l2norm(_dev(x, off=1), y_off=1), scalar, "x and y off")
    buf, body = _guarded(5, D, off=1)
    body.copy_(torch.from_numpy(np.array(x)))
    _l2norm(body, in_place=True, y_off=1)
    assert _guards_intact(buf, body)
    _assert_bits(body, scalar, "in place, off")
    aligned_shift = _l2norm(_dev(x), _dev(shift))
    _assert_bits(aligned_shift, model.l2norm_rows(x, shift=shift), "aligned shift")
    scalar_shift = model.l2norm_rows(x, shift=shift, aligned=False)          # (the Shift's add can round the two onto the same bits)
    _assert_bits(_l2norm(_dev(x), _dev(shift, off=1)), scalar_shift, "shift off")


# ---- isx_l2norm_rows_bwd ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", model.BWD_D)
def test_l2norm_backward_is_the_documented_formula(D):
    L, check, st = _lib()
    for B in model.BWD_B:
        x, dy = model.bwd_case(B, D)
        dx_, ddy = _dev(x), _dev(dy)
        buf, out = _guarded(B, D)
        check(L.isx_l2norm_rows_bwd(dx_.data_ptr(), ddy.data_ptr(), B, D, EPS, out.data_ptr(), st), "isx_l2norm_rows_bwd")
        assert _guards_intact(buf, out)
        _assert_bits(out, model.l2norm_rows_bwd(x, dy), (B, D))


# ---- isx_gap_l2 ------------------------------------------------------------------------------------------------------------------------------------------
def _gap(f, nhwc=False, off=0):
    """f: a device tensor (B, C, H, W) in NCHW memory, or (B, HW, C) as it lies in memory when nhwc."""
    L, check, st = _lib()
    if nhwc:
        B, HW, C = f.shape
        H, W = HW, 1
    else:
        B, C, H, W = f.shape
    buf, y = _guarded(B, C, off=off)
    fn = L.isx_gap_l2_nhwc if nhwc else L.isx_gap_l2
    check(fn(f.data_ptr(), B, C, H, W, EPS, y.data_ptr(), st), "isx_gap_l2")
    assert _guards_intact(buf, y)
    return y


@pytest.mark.parametrize("B,C,H,W", model.GAP_NCHW)
def test_gap_l2_is_the_documented_sum(B, C, H, W):
    f = model.map_case(B, C, H, W)
    _assert_bits(_gap(_dev(f)), model.gap_l2(f), model.gap_plan(B, C, H * W))


@pytest.mark.parametrize("C,H,W", model.GAP_BATCH)
def test_gap_l2_of_an_image_does_not_depend_on_the_launch(C, H, W):
    """The same 3 images alone and as the first 3 of a launch of 512 (where the launcher stages fewer channels per pass): the same bits, the model's."""
    f = model.map_case(3, C, H, W)
    alone = _gap(_dev(f))
    _assert_bits(alone, model.gap_l2(f), "alone")
    many = torch.rand((model.GAP_MANY, C, H, W), device="cuda")
    many[:3] = torch.from_numpy(np.array(f)).cuda()
    got = _gap(many)
    assert bool(torch.isfinite(got).all())
    _assert_bits(got[:3], alone, "first 3 of %d" % model.GAP_MANY)
    _assert_bits(got[:3], model.gap_l2(f, B_launch=model.GAP_MANY), "the model at that launch size")


def _nhwc(f):
    B, C = f.shape[:2]
    return np.ascontiguousarray(f.reshape(B, C, -1).transpose(0, 2, 1))


@pytest.mark.parametrize("C", model.GAP_NHWC_C)
def test_gap_l2_nhwc_is_the_documented_sum(C):
    """Channels-last, the float4 kernels and the generic path; against the NCHW entry inside the tolerance isx.h states (equal pooled values,
    another order of the sum of squares)."""
    for HW in model.GAP_NHWC_HW:
        f = model.map_case(2, C, HW, 1)
        got = _gap(_dev(_nhwc(f)), nhwc=True)
        _assert_bits(got, model.gap_l2_nhwc(_nhwc(f)), (C, HW, model.gap_nhwc_plan(C)))
        np.testing.assert_allclose(_host(got), _host(_gap(_dev(f))), **TOL)


def test_gap_l2_nhwc_at_an_offset_takes_the_generic_path():
    """The map one float off: the generic pooling, then the row kernel that y's alignment selects -- the wave kernel on an aligned y, the scalar
    kernel on a y that is off too.  Three different bit patterns."""
    f = model.map_case(2, 2048, 49, 1)
    m = _nhwc(f)
    vec, wave, scalar = model.gap_l2_nhwc(m), model.gap_l2_nhwc(m, map_aligned=False), model.gap_l2_nhwc(m, y_aligned=False)
    assert _differ(vec, wave) and _differ(vec, scalar) and _differ(wave, scalar)
    _assert_bits(_gap(_dev(m, off=1), nhwc=True), wave, "map off")
    _assert_bits(_gap(_dev(m), nhwc=True, off=1), scalar, "y off")
    _assert_bits(_gap(_dev(m, off=1), nhwc=True, off=1), scalar, "both off")


# ---- isx_best_location_desc, both layouts ---------------------------------------------------------------------------------------------------------------
def _best(cls, nhwc):
    L, check, st = _lib()
    B, K, Hp, Wp = cls.shape
    d = _dev(np.ascontiguousarray(cls.transpose(0, 2, 3, 1)) if nhwc else cls)
    buf, desc = _guarded(B, K)
    ibuf, loc = _guarded_i64(2 * B)
    fn = L.isx_best_location_desc_nhwc if nhwc else L.isx_best_location_desc
    check(fn(d.data_ptr(), B, K, Hp, Wp, EPS, desc.data_ptr(), loc.data_ptr(), st), "isx_best_location_desc")
    assert _guards_intact(buf, desc) and _guards_intact(ibuf, loc)
    return desc, loc.view(B, 2).cpu().numpy()


@pytest.mark.parametrize("K,Hp,Wp", [(K, 3, 2) for K in model.BEST_K] + [(17, 20, 15)])
def test_best_location_desc_is_the_documented_sum_in_both_layouts(K, Hp, Wp):
    """The tie between (2, 0) and (0, 1) goes to the smaller column; -0 and +0 are one score; the two layouts give equal bits."""
    cls = model.best_case(K, Hp, Wp)
    want, want_loc = model.best_location_desc(cls)
    assert tuple(want_loc[1]) == (2, 0) and tuple(want_loc[2]) == (0, 1)
    d0, l0 = _best(cls, False)
    d1, l1 = _best(cls, True)
    assert np.array_equal(l0, want_loc) and np.array_equal(l1, want_loc)
    _assert_bits(d0, want, "NCHW")
    _assert_bits(d1, d0, "NHWC against NCHW")


# ---- isx_region_gather_l2, both layouts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,kh,kw", model.GATHER)
def test_region_gather_l2_is_the_documented_sum_in_both_layouts(C, kh, kw):
    """Six windows per image, among them index -1 and the first index past the map (zero rows); with and without Shift."""
    L, check, st = _lib()
    fmap, idx, Wp, shift = model.gather_case(C, kh, kw)
    B, _, Hf, Wf = fmap.shape
    k, Fw = idx.shape[1], C * kh * kw
    didx = _dev(idx, dtype=np.int64)
    hwc_shift = model.shift_hwc(shift, C, kh, kw)
    for order, fn, dmap in (("chw", L.isx_region_gather_l2, _dev(fmap)), ("hwc", L.isx_region_gather_l2_nhwc, _dev(np.ascontiguousarray(fmap.transpose(0, 2, 3, 1))))):
        for sh in (None, shift if order == "chw" else hwc_shift):
            dsh = None if sh is None else _dev(sh)
            buf, rows = _guarded(B, k, Fw)
            check(fn(dmap.data_ptr(), B, C, Hf, Wf, kh, kw, didx.data_ptr(), k, Wp, None if dsh is None else dsh.data_ptr(), EPS, rows.data_ptr(), st),
                  "isx_region_gather_l2")
            assert _guards_intact(buf, rows)
            want = model.region_gather_l2(fmap, kh, kw, idx, Wp, shift=sh, order=order)
            assert not want[0, 2].any() and not want[0, 3].any() and want[0, 0].any()
            _assert_bits(rows, want, (order, sh is not None))


# ---- empty problems ---------------------------------------------------------------------------------------------------------------------------------------
def test_empty_problems_launch_nothing():
    L, check, st = _lib()
    x = torch.zeros((4, 8), device="cuda")
    idx = torch.zeros((4,), device="cuda", dtype=torch.int64)
    outs = [_guarded(4, 8) for _ in range(9)]
    o = [b[1].data_ptr() for b in outs]
    ibuf, loc = _guarded_i64(8)
    check(L.isx_l2norm_rows(x.data_ptr(), 0, 8, EPS, o[0], st), "isx_l2norm_rows")
    check(L.isx_l2norm_rows(x.data_ptr(), 4, 0, EPS, o[0], st), "isx_l2norm_rows")
    check(L.isx_l2norm_shift_rows(x.data_ptr(), x.data_ptr(), 0, 8, EPS, o[1], st), "isx_l2norm_shift_rows")
    check(L.isx_l2norm_rows_bwd(x.data_ptr(), x.data_ptr(), 0, 8, EPS, o[2], st), "isx_l2norm_rows_bwd")
    check(L.isx_l2norm_rows_bwd(x.data_ptr(), x.data_ptr(), 4, 0, EPS, o[2], st), "isx_l2norm_rows_bwd")
    check(L.isx_gap_l2(x.data_ptr(), 0, 2, 2, 2, EPS, o[3], st), "isx_gap_l2")
    check(L.isx_gap_l2_nhwc(x.data_ptr(), 0, 4, 2, 1, EPS, o[4], st), "isx_gap_l2_nhwc")
    check(L.isx_best_location_desc(x.data_ptr(), 0, 2, 2, 2, EPS, o[5], loc.data_ptr(), st), "isx_best_location_desc")
    check(L.isx_best_location_desc_nhwc(x.data_ptr(), 0, 2, 2, 2, EPS, o[6], loc.data_ptr(), st), "isx_best_location_desc_nhwc")
    for B, k in ((0, 1), (1, 0)):
        check(L.isx_region_gather_l2(x.data_ptr(), B, 4, 2, 2, 1, 1, idx.data_ptr(), k, 2, None, EPS, o[7], st), "isx_region_gather_l2")
        check(L.isx_region_gather_l2_nhwc(x.data_ptr(), B, 4, 2, 2, 1, 1, idx.data_ptr(), k, 2, None, EPS, o[8], st), "isx_region_gather_l2_nhwc")
    torch.cuda.synchronize()
    assert _guards_intact(ibuf, loc) and bool((loc == POISON).all())
    for buf, body in outs:
        assert _guards_intact(buf, body) and bool(torch.isnan(body).all())
