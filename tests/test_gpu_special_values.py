"""The trunk kernels on operands that are not finite, ordinary numbers: planted NaNs and infinities, subnormal inputs, subnormal products and
overflowing chains (tests/_special_values.py), through the C ABI between the guards of tests/_guards.py as tests/test_gpu_trunk_guards.py calls
them, at that file's shapes.  These are the values at which a kernel's shortcut stops being neutral: a zero-filled k tail, a padding tap, a
dead row that repeats the last image, a padded weight slot all rest on 0 * x = 0, which holds for finite x only; a flushed subnormal or another
order of an overflowing chain gives other bits.

Every launch is checked with G.assert_clean (no planted NaN is the poison) and compared under G.assert_special: the NaN positions of kernel and
reference are the same set, everything else -- infinities and subnormals included -- equal bit for bit.  -0 folds onto +0 only for the bias and
pool kernels under ReLU.  tests/test_special_values_model.py asserts on the CPU that every reference here holds what its plan is about."""
import numpy as np
import pytest
import torch

import _alex_model as A
import _guards as G
import _special_values as S
import oracle as O
import test_gpu_trunk_guards as T

pytestmark = pytest.mark.gpu

F = np.float32
hooks, _ok, _lib = T.hooks, T._ok, T._lib


# ---- isx_conv1x1_nhwc -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("M,Cin,Cout", S.C1_TILED)
def test_conv1x1_tiled_gemm(M, Cin, Cout, plan):
    assert not G.stream_applicable(M, Cin, Cout, 0)
    for res, relu in S.flags(plan):
        ops = S.c1_operands(M, Cin, Cout, plan, res)
        want = S.c1_reference(M, Cin, Cout, plan, res, relu)
        for off in (0, 1):                                # off the boundary: the scalar branch of load_tile
            ins = T._c1_inputs(*ops, off, off)
            for cfg in (-1, 0, 1, 2, 3):
                with hooks(gemm=cfg):
                    out = T._c1_run(ins, relu, off, (plan, res, relu, "gemm cfg", cfg, "offset", off))
                G.assert_special(out, want, (plan, res, relu, "gemm cfg", cfg, "offset", off))


@pytest.mark.parametrize("plan", S.PLANS)
def test_conv1x1_tail_grid(plan):
    """128x128 tiles + the 64x64 tail grid; the planted sites lie around the split and in the 64x64 region."""
    M, Cin, Cout = S.C1_TAIL
    split = G.tail_split_rows(M, Cout, T.SLOTS)
    assert split == 131072 and not G.stream_applicable(M, Cin, Cout, 0), "the shape must take the tail split"
    rows = S.c1_windows(M, split)
    for res, relu in S.flags(plan):
        ins = T._c1_inputs(*S.c1_operands(M, Cin, Cout, plan, res, split))
        with hooks(gemm=0):
            ref = T._c1_run(ins, relu, 0, "128x128 + 64x64 tail")
        G.assert_special(T._rows(ref, rows), S.c1_reference(M, Cin, Cout, plan, res, relu, split), (plan, res, relu, "tail grid vs oracle"))
        for name, gemm, conv in (("automatic", -1, -1), ("128x128 without tail", 0, 7), ("64x64", 3, -1)):
            with hooks(gemm=gemm, conv=conv):
                out = T._c1_run(ins, relu, 0, name)
            G.assert_same_special(out, ref, (plan, res, relu, name))
            del out
        del ref, ins


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("M,Cin,Cout", S.C1_STREAM)
def test_conv1x1_stream_kernel(M, Cin, Cout, plan):
    """csrc/stream1x1.hip (weights in registers): three row windows against the oracle, the whole body against the tiled GEMM (conv cfg 9)."""
    rows = S.c1_windows(M)
    for res, relu in S.flags(plan):
        ins = T._c1_inputs(*S.c1_operands(M, Cin, Cout, plan, res))
        assert G.stream_applicable(M, Cin, Cout, ins[0].ptr), "the shape must take the streaming kernel"
        ref = T._c1_run(ins, relu, 0, "stream")
        G.assert_special(T._rows(ref, rows), S.c1_reference(M, Cin, Cout, plan, res, relu), (plan, res, relu, "stream vs oracle"))
        with hooks(conv=9):
            out = T._c1_run(ins, relu, 1, "tiled")
        G.assert_same_special(out, ref, (plan, res, relu, "stream vs conv cfg 9"))


# ---- isx_conv1x1_dual_nhwc ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.DUAL)
def test_conv1x1_dual(case, plan):
    ops = S.dual_operands(case, plan)
    for relu in (True, False):
        want = S.dual_reference(case, plan, relu)
        for cfg in (-1, 0, 2, 3):
            for off in (0, 1):
                ins = T._dual_inputs(*ops, off)
                with hooks(conv=cfg):
                    out = T._dual_run(ins, case[6], relu, off, (plan, relu, "conv cfg", cfg, "offset", off))
                G.assert_special(out, want, (plan, relu, "conv cfg", cfg, "offset", off))


# ---- isx_conv3x3_nhwc -----------------------------------------------------------------------------------------------------------------------
def _c3_all(case, plan, cfgs):
    for res, relu in S.flags(plan):
        ops = S.c3_operands(case, plan, res)
        want = S.c3_reference(case, plan, res, relu)
        for off in (0, 1):
            ins = T._c3_inputs(*ops, off)
            for cfg in cfgs:
                with hooks(conv=cfg):
                    out = T._c3_run(ins, case[5], relu, off, (plan, res, relu, "conv cfg", cfg, "offset", off))
                G.assert_special(out, want, (plan, res, relu, "conv cfg", cfg, "offset", off))


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.C3_PIXEL)
def test_conv3x3_pixel_major(case, plan):
    _c3_all(case, plan, (-1, 0, 2, 3))


def _assert_posmaj(case):
    B, H, W, Cin, Cout, stride = case
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert G.pos_major_rows(B, H, W, Cin, Ho, Wo, Cout, (Cout + 63) // 64) == (B + 127) // 128 * Ho * Wo * 128, "the shape must be eligible"
    assert B % 128 == 1


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.C3_POSMAJ)
def test_conv3x3_position_major(case, plan):
    """Forced 128x128 tiles run position-major on these shapes: longest first (cfg 0) and in raster order (cfg 11); cfg -1 / 10 are the same two
    orders under the automatic tile pick, cfg 8 the pixel-major order.  Non-finite weights sit on the centre tap, where every order agrees."""
    _assert_posmaj(case)
    _c3_all(case, plan, (-1, 10, 0, 11, 8))


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("case", S.C3_POSMAJ)
def test_conv3x3_non_finite_weight_under_a_padding_tap(case, relu):
    """The one documented divergence (csrc/conv3x3_tile.hpp): +inf on tap (0, 0).  The pixel-major order computes 0 * inf = NaN
    wherever that tap is padding, as the oracle does; the position-major order skips the tap there and equals the oracle evaluated with that
    tap's weights 0 at exactly those positions -- and the plain oracle everywhere else."""
    _assert_posmaj(case)
    ops, plain, skipped = S.c3_divergence(case, relu)
    ins = T._c3_inputs(*ops)
    for cfg, want in ((8, plain), (0, skipped), (11, skipped)):
        with hooks(conv=cfg):
            out = T._c3_run(ins, case[5], relu, 0, ("conv cfg", cfg))
        G.assert_special(out, want, ("conv cfg", cfg, "relu", relu))


# ---- fused expand kernels ---------------------------------------------------------------------------------------------------------------------
def _pair(x, w2, b2, stride, w3, b3, r, relu, what):
    """The two-kernel pair the fused kernels replace: isx_conv3x3_nhwc (+ ReLU) then isx_conv1x1_nhwc."""
    ins = T._c3_inputs(x, w2, b2, None)
    mid = T._c3_run(ins, stride, True, 0, (what, "pair: conv3x3"))
    midh = mid.host()
    out = T._c1_run(T._c1_inputs(midh.reshape(-1, midh.shape[-1]), w3, b3, None if r is None else r.reshape(-1, r.shape[-1])), relu, 0, (what, "pair: conv1x1"))
    return midh, out.host().reshape(midh.shape[:3] + (w3.shape[0],))


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.EXPAND)
def test_conv3x3_expand(case, plan):
    L, st = _lib()
    B, H, W, Cin, stride = case
    for res, relu in S.flags(plan):
        x, w2, b2, w3, b3, r = S.expand_operands(case, plan, res)
        mid, want = S.expand_reference(case, plan, res, relu)
        pmid, pair = _pair(x, w2, b2, stride, w3, b3, r, relu, (plan, res, relu))
        G.assert_special(pmid, mid, (plan, "mid of the pair"))
        G.assert_special(pair, want, (plan, res, relu, "pair"))
        for off in (0, 1):
            ins = [G.in_f32(x, 128 * Cin), G.in_f32(w2, 64 * 9 * Cin), G.in_f32(b2, 256, off), G.in_f32(np.ascontiguousarray(w3.T), 64 * 256),
                   G.in_f32(b3, 256, off), G.in_f32(r, 128 * 256, off) if res else None]
            out = G.out_f32(want.shape, 128 * 256, off)
            _ok(L.isx_conv3x3_expand_nhwc(ins[0].ptr, B, H, W, Cin, ins[1].ptr, ins[2].ptr, stride, ins[3].ptr, 256, ins[4].ptr, G.ptr(ins[5]), int(relu),
                                          out.ptr, st), (plan, "offset", off))
            G.assert_clean([out], ins, (plan, "offset", off))
            G.assert_special(out, want, (plan, res, relu, "offset", off))
            G.assert_special(out, pair, (plan, res, relu, "fused vs pair"))


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.EXPAND_DUAL)
def test_conv3x3_expand_dual(case, plan):
    L, st = _lib()
    B, H, W, Cin = case
    t, w2, b2, x2, wc, b = S.expand_dual_operands(case, plan)
    for relu in (True, False):
        mid, want = S.expand_dual_reference(case, plan, relu)
        mreg = T._c3_run(T._c3_inputs(t, w2, b2, None), 1, True, 0, (plan, "pair: conv3x3"))
        G.assert_special(mreg, mid, (plan, "mid of the pair"))
        pair = T._dual_run(T._dual_inputs(mreg.host(), x2, wc, b), 1, relu, 0, (plan, "pair: dual")).host()
        G.assert_special(pair, want, (plan, relu, "pair"))
        for off in (0, 1):
            ins = [G.in_f32(t, 128 * Cin), G.in_f32(w2, 64 * 9 * Cin), G.in_f32(b2, 256, off), G.in_f32(x2, 128 * 64),
                   G.in_f32(np.ascontiguousarray(wc.T), 64 * 256), G.in_f32(b, 256, off)]
            out = G.out_f32(want.shape, 128 * 256, off)
            _ok(L.isx_conv3x3_expand_dual_nhwc(ins[0].ptr, B, H, W, Cin, ins[1].ptr, ins[2].ptr, ins[3].ptr, ins[4].ptr, 256, ins[5].ptr, int(relu), out.ptr, st),
                (plan, "offset", off))
            G.assert_clean([out], ins, (plan, "offset", off))
            G.assert_special(out, want, (plan, relu, "offset", off))
            G.assert_special(out, pair, (plan, relu, "fused vs pair"))


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.EXPAND128)
def test_conv3x3_expand128(case, plan):
    B, H, W, Cin, Cout = case
    posmaj = B >= 128
    assert (G.pos_major_rows(B, H, W, Cin, H, W, Cout, 2) > 0) == posmaj
    for res, relu in S.flags(plan):
        ops = S.e128_operands(case, plan, res)
        mid, want = S.e128_reference(case, plan, res, relu)
        pmid, pair = _pair(ops[0], ops[1], ops[2], 1, ops[3], ops[4], ops[5], relu, (plan, res, relu))
        G.assert_special(pmid, mid, (plan, "mid of the pair"))
        G.assert_special(pair, want, (plan, res, relu, "pair"))
        for off in (0, 1):
            ins = T._e128_inputs(ops, off)
            for cfg in (-1, 8) + ((10,) if posmaj else ()):
                with hooks(conv=cfg):
                    out = T._e128_run(ins, relu, off, (plan, "conv cfg", cfg, "offset", off))
                G.assert_special(out, want, (plan, res, relu, "conv cfg", cfg, "offset", off))
                G.assert_special(out, pair, (plan, res, relu, "fused vs pair, conv cfg", cfg))


# ---- isx_stem7x7_pool_nhwc --------------------------------------------------------------------------------------------------------------------
def _stem_run(x, w, b, want, what, off=0):
    L, st = _lib()
    B, H, W, _ = x.shape
    ins = [G.in_f32(x, 8 * W * 3 + 1024), G.in_f32(w, 64 * 147, off), G.in_f32(b, 256, off)]
    out = G.out_f32(want.shape, 128 * 64 * max(1, want.shape[2] // 8), off)
    _ok(L.isx_stem7x7_pool_nhwc(ins[0].ptr, B, H, W, ins[1].ptr, ins[2].ptr, out.ptr, st), what)
    G.assert_clean([out], ins, what)
    G.assert_special(out, want, what)


@pytest.mark.parametrize("value", list(S.STEM_VALUES))
@pytest.mark.parametrize("case", S.STEM)
def test_stem7x7_pool_planted(case, value):
    """+inf, -inf or NaN in each channel in turn: at every site together and at one site per launch, so that a failure names its site.  The
    entry's input contract is finite data (include/isx.h); what it does with other data is stated there and pinned here: the oracle's sums, and
    the zero-weight k slot that pads a filter row's 21 terms to 22 as fma(x[hi][2 wo + 4][0], 0, acc) (S.stem_model) -- a non-finite value in
    channel 0 of an even column c >= 4 zeroes conv column (c - 4) / 2 too, any other planted value reaches its own window only."""
    sites = S.stem_sites(*case)
    for ch in range(3):
        for site in [None] + list(range(len(sites))):
            x, w, b = S.stem_planted(case, value, ch, site)
            _stem_run(x, w, b, S.stem_reference(case, value, ch, site), (case, value, "channel", ch, "site", "all" if site is None else sites[site]))


@pytest.mark.parametrize("plan", S.PLANS[1:])
@pytest.mark.parametrize("case", S.STEM)
def test_stem7x7_pool_scaled(case, plan):
    x, w, b = S.stem_scaled(case, plan)
    for off in (0, 1):
        _stem_run(x, w, b, S.stem_scaled_reference(case, plan), (case, plan, "offset", off), off)


# ---- isx_bias_relu_maxpool_nhwc / isx_bias_act_inplace ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.POOL)
def test_bias_relu_maxpool(case, plan):
    """A NaN alone in a window gives 0 (the oracle's fmaxf), a NaN next to larger values gives the largest."""
    L, st = _lib()
    B, H, W, C = case
    y, b = S.pool_operands(case, plan)
    want = S.pool_reference(case, plan)
    ins = [G.in_f32(y, 4 * W * C + 256), G.in_f32(b, 256)]
    out = G.out_f32(want.shape, 128 * C)
    _ok(L.isx_bias_relu_maxpool_nhwc(ins[0].ptr, ins[1].ptr, B, H, W, C, out.ptr, st), plan)
    G.assert_clean([out], ins, plan)
    G.assert_special(out, want, plan, fold_zero_sign=True)


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.BIAS_ACT)
def test_bias_act_inplace(case, plan):
    L, st = _lib()
    n, C, inner = case
    for res in (True, False):
        for relu in (True, False):
            y0, b, r = S.bias_act_operands(case, plan, res)
            want = S.bias_act_reference(case, plan, res, relu)
            for off in (0, 1):
                y = G.in_f32_io(y0, 4096, off)
                ins = [G.in_f32(b, 256, off), G.in_f32(r, 256, off) if res else None]
                _ok(L.isx_bias_act_inplace(y.ptr, ins[0].ptr, G.ptr(ins[1]), n, C, inner, int(relu), st), (plan, res, relu, "offset", off))
                assert y.guards_intact() and all(i is None or i.guards_intact() for i in ins), (plan, "offset", off)
                G.assert_special(y, want, (plan, res, relu, "offset", off), fold_zero_sign=relu)


# ---- isxa_conv2d_nhwc ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("name", S.ALEX)
def test_alex_conv2d_planted(name, relu):
    from isx import alex
    case = A.CONV_CASES[name]
    B, H, W, Cin, Cout, K, stride, pad = case
    x, w, bias = S.alex_operands(name)
    want = S.alex_reference(name, relu)
    regs = G.in_f32(x, 4096), G.in_f32(w, 4096), G.in_f32(bias, 4096), G.out_f32(want.shape, 4096)
    L = alex.lib()
    rc = L.isxa_conv2d_nhwc(regs[0].ptr, B, H, W, Cin, regs[1].ptr, Cout, K, stride, pad, regs[2].ptr, int(relu), regs[3].ptr, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (rc, L.isxa_last_error())
    G.assert_clean([regs[3]], regs[:3], name)
    G.assert_special(regs[3], want, (name, relu))


# ---- the suffix backward kernels against tests/_suffix_model.py -------------------------------------------------------------------------------------
def _lib3():
    from isx._lib import check, lib
    return lib(), check, torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("name", list(S.WGRAD))
def test_conv_wgrad(name, plan):
    """A non-finite dz at a pixel whose tap is padding gives NaN in the model (gather_rows puts a +0 row there) and must in the kernel."""
    import _suffix_model as M
    L, check, st = _lib3()
    g, Cin, Cout, leaves, which = M.WGRAD_CASES[name]
    K, Sp = M.wgrad_K(name), S.WGRAD[name]
    assert L.isx_conv_wgrad_splits(K, Cin, Cout, g.taps) == Sp
    dz, x = S.wgrad_operands(name, plan)
    want_dw, want_db = S.wgrad_reference(name, plan)
    Ho, Wo = M.out_hw(g)
    gz, gx = G.in_f32(dz, 64 * Cout), G.in_f32(x, 64 * Cin * (g.W + 2))
    dw, db = G.out_f32((leaves, Sp, Cout, g.taps, Cin), 4096), G.out_f32((leaves, Sp, Cout), 4096)
    check(L.isx_conv_wgrad_nhwc(gz.ptr, gx.ptr, g.B, leaves, g.H, g.W, Cin, Cout, g.taps, g.stride, dw.ptr, db.ptr, st), "isx_conv_wgrad_nhwc")
    G.assert_clean([dw, db], [gz, gx], (name, plan))
    G.assert_special(dw, want_dw, (name, plan, "dw"))
    G.assert_special(db, want_db, (name, plan, "db"))


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("M_,Cin,Cout", S.DGRAD1)
def test_conv1x1_dgrad(M_, Cin, Cout, plan):
    """The reduction runs over Cout = 80 (a zero-filled last k-tile under every tile shape but the 128x128 one); a NaN in the mask selects 0.  A
    chain that ends on -0 comes out as +0: the epilogue adds its absent bias as +0 (S.zero_fill_term)."""
    L, check, st = _lib3()
    dz, wt, add, mask = S.dgrad1_operands(M_, Cin, Cout, plan)
    gz, gw, ga, gm = G.in_f32(dz, 128 * Cout), G.in_f32(wt, 128 * Cout), G.in_f32(add, 128 * Cin), G.in_f32(mask, 128 * Cin)
    for with_add, with_mask in S.flags(plan):
        want = S.dgrad1_reference(M_, Cin, Cout, plan, with_add, with_mask)
        for cfg in (-1, 0, 1, 2, 3):
            with hooks(gemm=cfg):
                dx = G.out_f32((M_, Cin), 128 * Cin)
                check(L.isx_conv1x1_dgrad_nhwc(gz.ptr, M_, Cout, gw.ptr, Cin, ga.ptr if with_add else None, gm.ptr if with_mask else None, dx.ptr, st),
                      "isx_conv1x1_dgrad_nhwc")
            G.assert_clean([dx], [gz, gw, ga, gm], (plan, with_add, with_mask, cfg))
            G.assert_special(dx, want, (plan, with_add, with_mask, "gemm cfg", cfg))


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("name", S.DGRAD3)
def test_conv3x3_dgrad(name, plan):
    import _suffix_model as M
    L, check, st = _lib3()
    B, H, W, Cout, Cin, _ = M.DGRAD3_CASES[name]
    dz, wt, mask = S.dgrad3_operands(name, plan)
    gz, gw, gm = G.in_f32(dz, 128 * Cout * min(H * W, 64)), G.in_f32(wt, 128 * 9 * Cout), G.in_f32(mask, 128 * Cin)
    for with_mask in (True, False):
        dx = G.out_f32((B, H, W, Cin), 128 * Cin)
        check(L.isx_conv3x3_dgrad_nhwc(gz.ptr, B, H, W, Cout, gw.ptr, Cin, gm.ptr if with_mask else None, dx.ptr, st), "isx_conv3x3_dgrad_nhwc")
        G.assert_clean([dx], [gz, gw, gm], (name, plan, with_mask))
        G.assert_special(dx, S.dgrad3_reference(name, plan, with_mask), (name, plan, with_mask))


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.COL2IM)
def test_conv3x3_s2_col2im(case, plan):
    L, check, st = _lib3()
    B, H, W, Cin = case
    dcol, mask = S.col2im_operands(case, plan)
    gd, gm = G.in_f32(dcol, 4096), G.in_f32(mask, 4096)
    for with_mask in (True, False):
        dx = G.out_f32((B, H, W, Cin), 4096)
        check(L.isx_conv3x3_s2_col2im_nhwc(gd.ptr, B, H, W, Cin, gm.ptr if with_mask else None, dx.ptr, st), "isx_conv3x3_s2_col2im_nhwc")
        G.assert_clean([dx], [gd, gm], (case, plan, with_mask))
        G.assert_special(dx, S.col2im_reference(case, plan, with_mask), (case, plan, with_mask))


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("n", S.RELU_N)
def test_relu_grad(n, plan):
    """Out of place and in place.  The kernel selects: a subnormal y > 0 lets dy through, a NaN y gives 0."""
    L, check, st = _lib3()
    dy, y = S.relu_operands(n, plan)
    want = S.relu_reference(n, plan)
    gd, gy = G.in_f32(dy, 4096), G.in_f32(y, 4096)
    dz = G.out_f32((n,), 4096)
    check(L.isx_relu_grad(gd.ptr, gy.ptr, n, dz.ptr, st), "isx_relu_grad")
    G.assert_clean([dz], [gd, gy], (n, plan))
    G.assert_special(dz, want, (n, plan, "out of place"))
    io = G.in_f32_io(dy, 4096)
    check(L.isx_relu_grad(io.ptr, gy.ptr, n, io.ptr, st), "isx_relu_grad")
    assert io.guards_intact() and gy.guards_intact()
    G.assert_special(io, want, (n, plan, "in place"))


@pytest.mark.parametrize("plan", S.PLANS)
@pytest.mark.parametrize("case", S.FOLD)
def test_bn_fold_backward(case, plan):
    """The partials are summed in split order (+inf and -inf in two partials of one element give NaN), then the chain rule of the folded BN."""
    L, check, st = _lib3()
    taps, Cin, leaves, Sp = case
    dwp, db, w, sc, mean, istd = S.fold_operands(case, plan)
    Cout = w.shape[0]
    ins = [G.in_f32(a, 4096) for a in (dwp, db, w, sc, mean, istd)]
    outs = [G.out_f32(s, 4096) for s in ((leaves, Cout, Cin, taps), (leaves, Cout), (leaves, Cout))]
    check(L.isx_bn_fold_backward(ins[0].ptr, ins[1].ptr, leaves, Sp, ins[2].ptr, ins[3].ptr, ins[4].ptr, ins[5].ptr, Cout, Cin, taps, 0, 0,
                                 outs[0].ptr, outs[1].ptr, outs[2].ptr, st), "isx_bn_fold_backward")
    G.assert_clean(outs, ins, (case, plan))
    for got, want, what in zip(outs, S.fold_reference(case, plan), ("gw", "ggamma", "gbeta")):
        G.assert_special(got, want, (case, plan, what))
