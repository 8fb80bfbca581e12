"""The kernels of the inference trunk (1x1 / 3x3 / dual / fused-expand convolutions, the streaming 1x1 kernel, the stem and its helpers) called
through the C ABI with buffers the TEST owns (tests/_guards.py), where test_gpu_parity.py and its siblings go through isx.ops and compare a
fresh torch.empty with the oracle.  Every launch here

  * writes into a body poisoned with one NaN bit pattern: an element a tile shape, a tail grid or a row order skips is still poison afterwards
    (through ops, the caching allocator hands the second config of a loop the block that holds the first config's correct result);
  * sits between sentinel guards wide enough for every address a dead row of the last tile could map to -- 128 rows of the output for the
    pixel-major kernels, 127 images of y behind the position-major order (the dead slots of the last group of 128 images);
  * reads operands that sit between NaN guards, so that an operand read past either end reaches the output as a NaN;
  * must return 0 and equal the oracle BIT FOR BIT (uint32 views); shapes above ~2e5 outputs compare sampled rows / images / channels with the
    oracle and every forced configuration with one reference run over the whole body;
  * runs with the output (and the residual; for isx_conv1x1_nhwc every operand) on a 256-byte boundary and one float past it: the b32 buffer
    stores / loads of the epilogues and the scalar branch of load_tile (csrc/gemm_tile.hpp) take any 4-byte alignment.  The operands the
    entries refuse off a 16-byte boundary are covered on the CPU (tests/test_abi.py).

A case that means to take a path (tail grid, position-major order, streaming kernel) asserts the launcher's host arithmetic first, so a
change of thresholds fails here and does not silently test another path."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import _guards as G
import oracle as O

pytestmark = pytest.mark.gpu

F = np.float32
COMBOS = [(False, True), (True, True), (True, False), (False, False)]          # (residual, relu)
# Resident 128x128 convolution workgroups = 256 CUs x kWgPerCu128 (csrc/gemm_tile.hpp; the `slots` the launchers hand to gemm_tail_split_rows).
# KEEP IN STEP with kWgPerCu128: the path preconditions below are evaluated with it (tests/test_gpu_conv3x3_expand128.py::test_tail_tiles
# carries the same 512).
SLOTS = 256 * 2


def _lib():
    from isx._lib import lib
    return lib(), torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def hooks(gemm=-1, conv=-1):
    L = _lib()[0]
    try:
        L.isx_debug_set_gemm_cfg(gemm)
        L.isx_debug_set_conv_cfg(conv)
        yield
    finally:
        L.isx_debug_set_gemm_cfg(-1)
        L.isx_debug_set_conv_cfg(-1)


def _ok(rc, what):
    assert rc == 0, (what, rc, _lib()[0].isx_last_error())


def _same(a, b, what):
    assert torch.equal(a.raw(), b.raw()), ("bits differ from the reference run", what, int((a.raw() != b.raw()).sum()))


def _rows(out, rows):
    return out.body[torch.from_numpy(np.asarray(rows)).cuda()].cpu().numpy()


# ---- isx_conv1x1_nhwc -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _c1_case(M, Cin, Cout):
    rng = np.random.default_rng(M * 7 + Cin * 3 + Cout)
    x = np.maximum(rng.standard_normal((M, Cin), dtype=F), 0)
    w = rng.standard_normal((Cout, Cin), dtype=F) * F(Cin ** -0.5)
    return x, w, rng.standard_normal(Cout, dtype=F), rng.standard_normal((M, Cout), dtype=F)


def _c1_inputs(x, w, b, r, oin=0, ores=0):
    Cin, Cout = x.shape[1], w.shape[0]
    return (G.in_f32(x, 128 * Cin, oin), G.in_f32(w, 128 * Cin, oin), G.in_f32(b, 256, oin), None if r is None else G.in_f32(r, 128 * Cout, ores))


def _c1_run(ins, relu, oout, what):
    L, st = _lib()
    gx, gw, gb, gr = ins
    (M, Cin), Cout = gx.shape, gw.shape[0]
    out = G.out_f32((M, Cout), 128 * Cout, oout)
    _ok(L.isx_conv1x1_nhwc(gx.ptr, M, Cin, gw.ptr, Cout, gb.ptr, G.ptr(gr), int(relu), out.ptr, st), what)
    G.assert_clean([out], ins, what)
    return out


@pytest.mark.parametrize("res,relu", COMBOS)
@pytest.mark.parametrize("M,Cin,Cout", [(1, 4, 4), (65, 32, 36), (129, 100, 130), (130, 64, 256)])
def test_conv1x1_tiled_gemm(M, Cin, Cout, res, relu):
    """Every tile shape of the score / 1x1 GEMM; Cin = 32 / 64: the ALIGNED loads, Cin = 4 / 100: the clipped k-tail, and with the operands one
    float off the boundary the scalar branch of load_tile, which no other test reaches."""
    x, w, b, r = _c1_case(M, Cin, Cout)
    r = r if res else None
    assert not G.stream_applicable(M, Cin, Cout, 0)
    want = O.conv1x1_nhwc(x, w, b, r, relu)
    for oin, oout in ((0, 0), (1, 1), (0, 1), (1, 0)):
        ins = _c1_inputs(x, w, b, r, oin, oout)
        for cfg in (-1, 0, 1, 2, 3):
            with hooks(gemm=cfg):
                out = _c1_run(ins, relu, oout, ("gemm cfg", cfg, "offsets", oin, oout))
            G.assert_bits(out, want, ("gemm cfg", cfg, "offsets", oin, oout))


def _c1_windows(out, x, w, b, r, relu, rows, what):
    G.assert_bits(_rows(out, rows), O.conv1x1_nhwc(x[rows], w, b, None if r is None else r[rows], relu), what)


@pytest.mark.parametrize("Cin,Cout,res", [(32, 128, False), (64, 200, True), (40, 256, True)])
def test_conv1x1_tail_grid(Cin, Cout, res):
    """133 956 pixels = 1047 row tiles: the rows past the whole rounds run as 64x64 tiles in the same grid (conv1x1_tail_kernel).  The 128x128
    shape is FORCED, so the split alone decides the path."""
    M = 133956
    split = G.tail_split_rows(M, Cout, SLOTS)
    assert split == 131072 and not G.stream_applicable(M, Cin, Cout, 0), "the shape must take the tail split"
    x, w, b, r = _c1_case(M, Cin, Cout)
    r = r if res else None
    ins = _c1_inputs(x, w, b, r)
    with hooks(gemm=0):
        ref = _c1_run(ins, True, 0, "128x128 + 64x64 tail")
    rows = np.r_[0:100, split - 100:split + 100, M - 100:M]
    _c1_windows(ref, x, w, b, r, True, rows, "tail grid vs oracle")
    for name, gemm, conv, oout in (("automatic", -1, -1, 0), ("tail, y + 1 float", 0, -1, 1), ("128x128 without tail", 0, 7, 0), ("64x64", 3, -1, 0)):
        with hooks(gemm=gemm, conv=conv):
            out = _c1_run(ins, True, oout, name)
        _same(out, ref, name)
        del out


@pytest.mark.parametrize("tiles_m,splits", [(512 + 409, True), (512 + 410, False), (1024 + 1, True), (512, False)])
def test_conv1x1_tail_grid_boundaries(tiles_m, splits):
    """Around the decision of gemm_tail_split_rows at 512 resident workgroups: a remainder of at most 80 % of a round is split, a fuller last
    round and an exact number of rounds are not, a remainder of ONE tile is.  (test_conv1x1_tail_split_boundaries keeps the tile counts of
    the time when 1024 were resident; they no longer straddle the 80 % line.)"""
    Cin, Cout = 32, 128
    M = tiles_m * 128 - (37 if tiles_m % 2 else 0)
    split = G.tail_split_rows(M, Cout, SLOTS)
    assert (split > 0) == splits and split in (0, tiles_m // SLOTS * SLOTS * 128)
    x, w, b, _ = _c1_case(M, Cin, Cout)
    ins = _c1_inputs(x, w, b, None)
    with hooks(gemm=0):
        ref = _c1_run(ins, True, 0, "forced 128x128")
    edge = tiles_m // SLOTS * SLOTS * 128
    rows = np.unique(np.r_[0:100, max(edge - 100, 0):min(edge + 100, M), M - 100:M])
    _c1_windows(ref, x, w, b, None, True, rows, "vs oracle")
    for name, gemm, conv in (("automatic", -1, -1), ("128x128 without tail", 0, 7)):
        with hooks(gemm=gemm, conv=conv):
            out = _c1_run(ins, True, 1, name)
        _same(out, ref, name)
        del out


@pytest.mark.parametrize("res,relu", COMBOS)
@pytest.mark.parametrize("Cout", [64, 256])
def test_conv1x1_stream_kernel(Cout, res, relu):
    """csrc/stream1x1.hip: the four (residual, ReLU) instances of both widths, a ragged last pixel tile, more tiles than workgroups (Cout = 256:
    258 tiles of 64 pixels on 256 workgroups); y and the residual on and off the boundary; the same calls through the tiled GEMM (conv cfg 9)."""
    M, Cin = 16384 + 77, 64
    x, w, b, r = _c1_case(M, Cin, Cout)
    r = r if res else None
    ins = {o: _c1_inputs(x, w, b, r, 0, o) for o in (0, 1)}
    assert G.stream_applicable(M, Cin, Cout, ins[0][0].ptr), "the shape must take the streaming kernel"
    ref = _c1_run(ins[0], relu, 0, "stream")
    rows = np.r_[0:200, M // 2:M // 2 + 200, M - 200:M]
    _c1_windows(ref, x, w, b, r, relu, rows, "stream vs oracle")
    for conv, oout, ores in ((-1, 1, 1), (-1, 0, 1), (-1, 1, 0), (9, 0, 0), (9, 1, 1)):
        with hooks(conv=conv):
            out = _c1_run(ins[ores], relu, oout, ("conv cfg", conv, "y offset", oout, "residual offset", ores))
        _same(out, ref, ("conv cfg", conv, oout, ores))


@pytest.mark.parametrize("Cout", [64, 256])
def test_conv1x1_stream_shape_with_unaligned_x_takes_the_tiled_path(Cout):
    M, Cin = 16384 + 77, 64
    x, w, b, r = _c1_case(M, Cin, Cout)
    aligned, off = _c1_inputs(x, w, b, r), _c1_inputs(x, w, b, r, 1, 0)
    assert G.stream_applicable(M, Cin, Cout, aligned[0].ptr) and not G.stream_applicable(M, Cin, Cout, off[0].ptr)
    _same(_c1_run(off, True, 0, "x + 1 float"), _c1_run(aligned, True, 0, "stream"), "x + 1 float")


# ---- isx_conv3x3_nhwc -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _c3_case(B, H, W, Cin, Cout, stride):
    rng = np.random.default_rng(B * 1000 + H * 100 + W * 10 + Cin + Cout + stride)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = np.maximum(rng.standard_normal((B, H, W, Cin), dtype=F), 0)
    w = rng.standard_normal((Cout, 3, 3, Cin), dtype=F) * F((9 * Cin) ** -0.5)
    return x, w, rng.standard_normal(Cout, dtype=F), rng.standard_normal((B, Ho, Wo, Cout), dtype=F)


def _out_guard(B, Ho, Wo, Cout):
    """128 rows of y; where the position-major order is possible (B >= 128), the 127 dead image slots of the last group as well."""
    return max(128 * Cout, 127 * Ho * Wo * Cout if B >= 128 else 0)


def _c3_inputs(x, w, b, r, ores=0):
    B, H, W, Cin = x.shape
    return (G.in_f32(x, 128 * Cin * min(H * W, 64)), G.in_f32(w, 128 * 9 * Cin), G.in_f32(b, 256, ores),
            None if r is None else G.in_f32(r, _out_guard(*r.shape), ores))


def _c3_run(ins, stride, relu, oout, what):
    L, st = _lib()
    gx, gw, gb, gr = ins
    (B, H, W, Cin), Cout = gx.shape, gw.shape[0]
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = G.out_f32((B, Ho, Wo, Cout), _out_guard(B, Ho, Wo, Cout), oout)
    _ok(L.isx_conv3x3_nhwc(gx.ptr, B, H, W, Cin, gw.ptr, Cout, stride, gb.ptr, G.ptr(gr), int(relu), out.ptr, st), what)
    G.assert_clean([out], ins, what)
    return out


def _c3_all_cfgs(B, H, W, Cin, Cout, stride, res, relu, cfgs):
    x, w, b, r = _c3_case(B, H, W, Cin, Cout, stride)
    r = r if res else None
    want = O.conv3x3_nhwc(x, w, b, stride, r, relu)
    for off in (0, 1):
        ins = _c3_inputs(x, w, b, r, off)
        for cfg in cfgs:
            with hooks(conv=cfg):
                out = _c3_run(ins, stride, relu, off, ("conv cfg", cfg, "offset", off))
            G.assert_bits(out, want, ("conv cfg", cfg, "offset", off))


@pytest.mark.parametrize("res,relu", [(True, True), (False, False)])
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride", [(1, 1, 1, 32, 32, 1), (2, 3, 2, 32, 96, 2), (1, 9, 11, 64, 130, 2), (3, 5, 5, 64, 64, 1)])
def test_conv3x3_pixel_major(B, H, W, Cin, Cout, stride, res, relu):
    _c3_all_cfgs(B, H, W, Cin, Cout, stride, res, relu, (-1, 0, 2, 3))


@pytest.mark.parametrize("res,relu", [(True, True), (False, False)])
@pytest.mark.parametrize("B,H,W,Cin,Cout,stride", [(129, 3, 5, 64, 128, 1), (257, 2, 2, 128, 64, 1), (129, 6, 5, 64, 128, 2)])
def test_conv3x3_position_major(B, H, W, Cin, Cout, stride, res, relu):
    """One image in the last group of 128: 127 dead virtual rows per position, which must land nowhere.  cfg 0 forces the 128x128 tiles that
    run position-major; cfg 8 is the pixel-major order on the same shapes."""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert G.pos_major_rows(B, H, W, Cin, Ho, Wo, Cout, (Cout + 63) // 64) == (B + 127) // 128 * Ho * Wo * 128, "the shape must be eligible"
    assert B % 128 == 1
    _c3_all_cfgs(B, H, W, Cin, Cout, stride, res, relu, (-1, 0, 2, 3, 8))


def _channels(Cout):
    """Output channels the oracle evaluates on the large shapes (an output channel is an independent sum): both ends and the 128-column tile edge."""
    return np.unique(np.r_[0:8, 60:68, 124:132, Cout - 8:Cout] % Cout)


def _c3_oracle_images(out, x, w, b, r, stride, relu, images, what, all_channels=()):
    for i in images:
        ch = np.arange(w.shape[0]) if i in all_channels else _channels(w.shape[0])
        want = O.conv3x3_nhwc(x[i:i + 1], w[ch], b[ch], stride, None if r is None else np.ascontiguousarray(r[i:i + 1][..., ch]), relu)
        G.assert_bits(np.ascontiguousarray(out.body[i:i + 1].cpu().numpy()[..., ch]), want, (what, "image", i))


@pytest.mark.parametrize("Cout,stride,res", [(128, 1, False), (256, 1, True), (128, 2, True)])
def test_conv3x3_tail_grid(Cout, stride, res):
    """The shapes of test_conv3x3_tail_split (1047 row tiles): 128x128 tiles + 64x64 tail (cfg 0), 64x64 everywhere (cfg 3), the automatic pick
    with and without the tail (cfg -1, 7).  The oracle evaluates the first image and the last one, which holds the split: its rows end the
    128x128 region and fill the 64x64 one."""
    B, Ho, Cin = 9, 122, 32
    H = Ho * stride
    M = B * Ho * Ho
    split = G.tail_split_rows(M, Cout, SLOTS)
    assert (B - 1) * Ho * Ho <= split < M, "the shape must take the tail split, and the split must fall inside the last image"
    x, w, b, r = _c3_case(B, H, H, Cin, Cout, stride)
    r = r if res else None
    ins = _c3_inputs(x, w, b, r)
    with hooks(conv=0):
        ref = _c3_run(ins, stride, True, 0, "128x128 + 64x64 tail")
    _c3_oracle_images(ref, x, w, b, r, stride, True, (0, B - 1), "tail grid", all_channels=(B - 1,))     # the image that holds the split: every channel
    for cfg, oout in ((0, 1), (3, 0), (7, 0), (-1, 1)):
        with hooks(conv=cfg):
            out = _c3_run(ins, stride, True, oout, ("conv cfg", cfg))
        _same(out, ref, ("conv cfg", cfg))
        del out


def test_conv3x3_position_major_tail_grid():
    """The position-major tail of test_gpu_conv3x3_position_major.py: 14 image groups x 49 positions = 686 virtual tiles, the last 174 as 64-row
    tiles; the last group holds ONE image, so its second-half tail tiles have no live row at all."""
    H = W = 7
    Cin = Cout = 64
    groups = -(-int(1.3 * SLOTS * 128) // (49 * 128))
    B = (groups - 1) * 128 + 1
    Mv = G.pos_major_rows(B, H, W, Cin, H, W, Cout, 1)
    split = G.tail_split_rows(Mv, Cout, SLOTS)
    assert Mv == groups * 49 * 128 and 0 < split < Mv, "position-major AND the tail split"
    x, w, b, r = _c3_case(B, H, W, Cin, Cout, 1)
    ins = _c3_inputs(x, w, b, r)
    with hooks(conv=0):
        ref = _c3_run(ins, 1, True, 0, "position-major tail")
    g_tail = -(-(split // 128) // 49)                    # first group whose positions all follow the split
    assert g_tail < groups - 1
    images = sorted({0, 127, 128, g_tail * 128, g_tail * 128 + 63, g_tail * 128 + 64, g_tail * 128 + 127, B - 1})
    want = O.conv3x3_nhwc(x[images], w, b, 1, r[images], True)
    G.assert_bits(_rows(ref, images), want, "position-major tail vs oracle")
    for cfg, oout in ((0, 1), (8, 0), (-1, 1), (3, 0)):
        with hooks(conv=cfg):
            out = _c3_run(ins, 1, True, oout, ("conv cfg", cfg))
        _same(out, ref, ("conv cfg", cfg))


# ---- isx_conv1x1_dual_nhwc ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _dual_case(B, H, W, K1, K2, Cout, stride):
    rng = np.random.default_rng(B + H * 10 + W + K1 + K2 + Cout + stride)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    t = np.maximum(rng.standard_normal((B, Ho, Wo, K1), dtype=F), 0)
    x = np.maximum(rng.standard_normal((B, H, W, K2), dtype=F), 0)
    w = rng.standard_normal((Cout, K1 + K2), dtype=F) * F((K1 + K2) ** -0.5)
    return t, x, w, rng.standard_normal(Cout, dtype=F)


def _dual_inputs(t, x, w, b, obias=0):
    return G.in_f32(t, 128 * t.shape[3]), G.in_f32(x, 128 * x.shape[3]), G.in_f32(w, 128 * w.shape[1]), G.in_f32(b, 256, obias)


def _dual_run(ins, stride, relu, oout, what):
    L, st = _lib()
    gt, gx, gw, gb = ins
    (B, H, W, K2), K1, Cout = gx.shape, gt.shape[3], gw.shape[0]
    out = G.out_f32((B,) + gt.shape[1:3] + (Cout,), 128 * Cout, oout)
    _ok(L.isx_conv1x1_dual_nhwc(gt.ptr, K1, gx.ptr, B, H, W, K2, stride, gw.ptr, Cout, gb.ptr, int(relu), out.ptr, st), what)
    G.assert_clean([out], ins, what)
    return out


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("B,H,W,K1,K2,Cout,stride", [(1, 2, 2, 32, 32, 32, 1), (2, 9, 7, 32, 64, 130, 2), (2, 8, 6, 64, 64, 256, 1)])
def test_conv1x1_dual(B, H, W, K1, K2, Cout, stride, relu):
    t, x, w, b = _dual_case(B, H, W, K1, K2, Cout, stride)
    want = O.conv1x1_dual_nhwc(t, x, w, b, stride, relu)
    for cfg in (-1, 0, 2, 3):
        for oout in (0, 1):
            ins = _dual_inputs(t, x, w, b, oout)
            with hooks(conv=cfg):
                out = _dual_run(ins, stride, relu, oout, ("conv cfg", cfg, "offset", oout))
            G.assert_bits(out, want, ("conv cfg", cfg, "offset", oout))


@pytest.mark.parametrize("stride,Cout", [(1, 128), (2, 256)])
def test_conv1x1_dual_tail_grid(stride, Cout):
    B, Ho, K1, K2 = 9, 122, 32, 64
    H = Ho * stride
    split = G.tail_split_rows(B * Ho * Ho, Cout, SLOTS)
    assert (B - 1) * Ho * Ho <= split < B * Ho * Ho, "the shape must take the tail split, and the split must fall inside the last image"
    t, x, w, b = _dual_case(B, H, H, K1, K2, Cout, stride)
    ins = _dual_inputs(t, x, w, b)
    with hooks(conv=0):
        ref = _dual_run(ins, stride, True, 0, "128x128 + 64x64 tail")
    for i in (0, B - 1):
        ch = np.arange(Cout)
        want = O.conv1x1_dual_nhwc(t[i:i + 1], x[i:i + 1], w[ch], b[ch], stride, True)
        G.assert_bits(np.ascontiguousarray(ref.body[i:i + 1].cpu().numpy()[..., ch]), want, ("tail grid vs oracle, image", i))
    for cfg, oout in ((0, 1), (3, 0), (7, 0), (-1, 1)):
        with hooks(conv=cfg):
            out = _dual_run(ins, stride, True, oout, ("conv cfg", cfg))
        _same(out, ref, ("conv cfg", cfg))
        del out


# ---- isx_conv3x3_expand_nhwc / isx_conv3x3_expand_dual_nhwc (64 mid channels -> 256) ---------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cin,stride,res,relu", [(1, 1, 1, 32, 1, False, True), (1, 9, 11, 32, 2, False, False), (2, 7, 7, 64, 1, True, True)])
def test_conv3x3_expand(B, H, W, Cin, stride, res, relu):
    L, st = _lib()
    rng = np.random.default_rng(B * 100 + H + Cin)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x = np.maximum(rng.standard_normal((B, H, W, Cin), dtype=F), 0)
    w2 = rng.standard_normal((64, 3, 3, Cin), dtype=F) * F((9 * Cin) ** -0.5)
    b2 = rng.standard_normal(64, dtype=F)
    w3 = rng.standard_normal((256, 64), dtype=F) * F(0.125)
    b3 = rng.standard_normal(256, dtype=F)
    r = rng.standard_normal((B, Ho, Wo, 256), dtype=F) if res else None
    mid = O.conv3x3_nhwc(x, w2, b2, stride, None, True)
    want = O.conv1x1_nhwc(mid.reshape(-1, 64), w3, b3, r.reshape(-1, 256) if res else None, relu).reshape(B, Ho, Wo, 256)
    for off in (0, 1):
        ins = [G.in_f32(x, 128 * Cin), G.in_f32(w2, 64 * 9 * Cin), G.in_f32(b2, 256, off), G.in_f32(np.ascontiguousarray(w3.T), 64 * 256),
               G.in_f32(b3, 256, off), G.in_f32(r, 128 * 256, off) if res else None]
        out = G.out_f32((B, Ho, Wo, 256), 128 * 256, off)
        _ok(L.isx_conv3x3_expand_nhwc(ins[0].ptr, B, H, W, Cin, ins[1].ptr, ins[2].ptr, stride, ins[3].ptr, 256, ins[4].ptr, G.ptr(ins[5]), int(relu),
                                      out.ptr, st), ("offset", off))
        G.assert_clean([out], ins, ("offset", off))
        G.assert_bits(out, want, ("offset", off))


@pytest.mark.parametrize("B,H,W,Cin,relu", [(1, 1, 1, 32, True), (1, 9, 11, 32, False), (2, 7, 7, 64, True)])
def test_conv3x3_expand_dual(B, H, W, Cin, relu):
    L, st = _lib()
    rng = np.random.default_rng(B * 10 + H + Cin)
    t = np.maximum(rng.standard_normal((B, H, W, Cin), dtype=F), 0)
    x2 = np.maximum(rng.standard_normal((B, H, W, 64), dtype=F), 0)
    w2 = rng.standard_normal((64, 3, 3, Cin), dtype=F) * F((9 * Cin) ** -0.5)
    b2 = rng.standard_normal(64, dtype=F)
    wc = rng.standard_normal((256, 128), dtype=F) * F(128 ** -0.5)
    b = rng.standard_normal(256, dtype=F)
    want = O.conv1x1_dual_nhwc(O.conv3x3_nhwc(t, w2, b2, 1, None, True), x2, wc, b, 1, relu)
    for off in (0, 1):
        ins = [G.in_f32(t, 128 * Cin), G.in_f32(w2, 64 * 9 * Cin), G.in_f32(b2, 256, off), G.in_f32(x2, 128 * 64),
               G.in_f32(np.ascontiguousarray(wc.T), 64 * 256), G.in_f32(b, 256, off)]
        out = G.out_f32((B, H, W, 256), 128 * 256, off)
        _ok(L.isx_conv3x3_expand_dual_nhwc(ins[0].ptr, B, H, W, Cin, ins[1].ptr, ins[2].ptr, ins[3].ptr, ins[4].ptr, 256, ins[5].ptr, int(relu), out.ptr, st),
            ("offset", off))
        G.assert_clean([out], ins, ("offset", off))
        G.assert_bits(out, want, ("offset", off))


# ---- isx_conv3x3_expand128_nhwc (128 mid channels) ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _e128_case(B, H, W, Cin, Cout):
    rng = np.random.default_rng(B * 100 + H * 10 + W + Cin + Cout)
    x = np.maximum(rng.standard_normal((B, H, W, Cin), dtype=F), 0)
    w2 = rng.standard_normal((128, 3, 3, Cin), dtype=F) * F((9 * Cin) ** -0.5)
    b2 = rng.standard_normal(128, dtype=F)
    w3 = rng.standard_normal((Cout, 128), dtype=F) * F(128 ** -0.5)
    return x, w2, b2, w3, rng.standard_normal(Cout, dtype=F), rng.standard_normal((B, H, W, Cout), dtype=F)


def _e128_inputs(case, ores=0):
    x, w2, b2, w3, b3, r = case
    B, H, W, Cin = x.shape
    return [G.in_f32(x, 128 * Cin * min(H * W, 64)), G.in_f32(w2, 128 * 9 * Cin), G.in_f32(b2, 256, ores), G.in_f32(np.ascontiguousarray(w3.T), 128 * w3.shape[0]),
            G.in_f32(b3, 256, ores), None if r is None else G.in_f32(r, _out_guard(*r.shape), ores)]


def _e128_run(ins, relu, oout, what):
    L, st = _lib()
    (B, H, W, Cin), Cout = ins[0].shape, ins[3].shape[1]
    out = G.out_f32((B, H, W, Cout), _out_guard(B, H, W, Cout), oout)
    _ok(L.isx_conv3x3_expand128_nhwc(ins[0].ptr, B, H, W, Cin, ins[1].ptr, ins[2].ptr, ins[3].ptr, Cout, ins[4].ptr, G.ptr(ins[5]), int(relu), out.ptr, st), what)
    G.assert_clean([out], ins, what)
    return out


def _e128_oracle(case, res, relu, images):
    x, w2, b2, w3, b3, r = case
    sel = np.asarray(images)
    mid = O.conv3x3_nhwc(x[sel], w2, b2, 1, None, True)
    want = O.conv1x1_nhwc(mid.reshape(-1, 128), w3, b3, r[sel].reshape(-1, w3.shape[0]) if res else None, relu)
    return want.reshape((len(sel),) + x.shape[1:3] + (w3.shape[0],))


@pytest.mark.parametrize("B,H,W,Cin,Cout,res,relu,posmaj", [(1, 1, 1, 64, 128, True, True, False), (3, 7, 7, 64, 256, False, True, False),
                                                            (3, 7, 7, 64, 256, True, False, False), (129, 3, 5, 64, 128, True, True, True)])
def test_conv3x3_expand128(B, H, W, Cin, Cout, res, relu, posmaj):
    assert (G.pos_major_rows(B, H, W, Cin, H, W, Cout, 2) > 0) == posmaj
    case = _e128_case(B, H, W, Cin, Cout)
    case = case if res else case[:5] + (None,)
    want = _e128_oracle(case, res, relu, range(B))
    for off in (0, 1):
        ins = _e128_inputs(case, off)
        for cfg in (-1, 8):
            with hooks(conv=cfg):
                out = _e128_run(ins, relu, off, ("conv cfg", cfg, "offset", off))
            G.assert_bits(out, want, ("conv cfg", cfg, "offset", off))


def test_conv3x3_expand128_tail_grid():
    """The shape of test_gpu_conv3x3_expand128.py::test_tail_tiles: 14 image groups x 49 positions = 686 virtual tiles on 512 slots; the last
    group is ONE image.  Automatic (position-major + tail) and pixel-major (cfg 8; 81 585 rows = 638 tiles, a tail of its own)."""
    B, P, Cin, Cout = 13 * 128 + 1, 49, 64, 128
    groups = (B + 127) // 128
    Mv = G.pos_major_rows(B, 7, 7, Cin, 7, 7, Cout, 2)
    split = G.tail_split_rows(Mv, 128, SLOTS)
    assert Mv == groups * P * 128 and 0 < split < Mv, "position-major AND the tail split"
    assert G.tail_split_rows(B * P, 128, SLOTS) > 0, "the pixel-major order of this shape splits too"
    g_big, g_tail = split // 128 // P - 1, -(-(split // 128) // P)
    assert g_big >= 0 and g_tail < groups - 1
    images = [g_big * 128 + 5, g_tail * 128 + 3, g_tail * 128 + 64 + 28, B - 1]
    case = _e128_case(B, 7, 7, Cin, Cout)
    want = _e128_oracle(case, True, True, images)
    ins = _e128_inputs(case)
    ref = _e128_run(ins, True, 0, "position-major + tail")
    G.assert_bits(_rows(ref, images), want, "vs oracle")
    for cfg, oout in ((-1, 1), (8, 0), (8, 1)):
        with hooks(conv=cfg):
            out = _e128_run(ins, True, oout, ("conv cfg", cfg, "offset", oout))
        _same(out, ref, ("conv cfg", cfg, "offset", oout))


# ---- stem and its helpers ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(1, 1, 4), (1, 17, 12), (2, 50, 36), (1, 9, 228), (1, 223, 224), (1, 224, 224)])
def test_stem7x7_pool(B, H, W):
    """One step partly outside the image, narrow images (masked columns), two column bands (W = 228), ragged and whole 224 x 224 images in row bands."""
    L, st = _lib()
    rng = np.random.default_rng(H * 1000 + W + B)
    x = rng.standard_normal((B, H, W, 3), dtype=F)
    w = rng.standard_normal((64, 7, 7, 3), dtype=F) * F(147 ** -0.5)
    b = rng.standard_normal(64, dtype=F)
    want = O.stem7x7_pool_nhwc(x, w, b)
    for off in (0, 1):                                   # w and bias are per-lane scalar loads: off the boundary with the output
        ins = [G.in_f32(x, 8 * W * 3 + 1024), G.in_f32(w, 64 * 147, off), G.in_f32(b, 256, off)]
        out = G.out_f32(want.shape, 128 * 64 * max(1, want.shape[2] // 8), off)
        _ok(L.isx_stem7x7_pool_nhwc(ins[0].ptr, B, H, W, ins[1].ptr, ins[2].ptr, out.ptr, st), ("offset", off))
        G.assert_clean([out], ins, ("offset", off))
        G.assert_bits(out, want, ("offset", off))


@pytest.mark.parametrize("B,H,W,C", [(1, 1, 1, 4), (2, 7, 9, 8), (2, 12, 13, 36)])
def test_bias_relu_maxpool(B, H, W, C):
    L, st = _lib()
    rng = np.random.default_rng(H + C)
    y = rng.standard_normal((B, H, W, C), dtype=F)
    b = rng.standard_normal(C, dtype=F)
    want = O.bias_relu_maxpool_nhwc(y, b)
    ins = [G.in_f32(y, 4 * W * C + 256), G.in_f32(b, 256)]
    out = G.out_f32(want.shape, 128 * C)
    _ok(L.isx_bias_relu_maxpool_nhwc(ins[0].ptr, ins[1].ptr, B, H, W, C, out.ptr, st), "maxpool")
    G.assert_clean([out], ins)
    G.assert_bits(out, want)


@pytest.mark.parametrize("res", [True, False])
@pytest.mark.parametrize("n,C,inner,relu", [(35, 5, 1, True), (60, 5, 6, False), (64, 8, 1, True), (64, 2, 8, True)])
def test_bias_act_inplace(n, C, inner, relu, res):
    """In place: the body is the input, the guards are what the test adds.  n = 35 / 60: the scalar kernel; n = 64: the two float4 kernels when
    every pointer is on a 16-byte boundary, the scalar kernel one float off it.  Unfused fp32 adds in the kernels' order."""
    L, st = _lib()
    rng = np.random.default_rng(n + C)
    y0, b = rng.standard_normal(n, dtype=F), rng.standard_normal(C, dtype=F)
    r = rng.standard_normal(n, dtype=F) if res else None
    want = y0 + b[(np.arange(n) // inner) % C]
    want = want + r if res else want
    want = np.maximum(want, F(0)) if relu else want
    for off in (0, 1):
        y = G.in_f32_io(y0, 4096, off)
        ins = [G.in_f32(b, 256, off), G.in_f32(r, 256, off) if res else None]
        _ok(L.isx_bias_act_inplace(y.ptr, ins[0].ptr, G.ptr(ins[1]), n, C, inner, int(relu), st), ("offset", off))
        assert y.guards_intact() and all(i is None or i.guards_intact() for i in ins), ("offset", off)
        G.assert_bits(y, want.astype(F), ("offset", off))


@pytest.mark.parametrize("cl", [True, False])
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 5, 7), (1, 4, 6)])
def test_images_u8_to_f32(B, H, W, cl):
    """(1,1,1), (2,5,7): the per-pixel stores (a ragged last quad); (1,4,6): the float4 stores of both layouts (H W a multiple of 4)."""
    L, st = _lib()
    rng = np.random.default_rng(H)
    img = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    want = O.images_u8_to_f32(img, mean, std)
    want = np.ascontiguousarray(want.transpose(0, 2, 3, 1)) if cl else want
    for off in (0, 1, 2):                                # img on a dword boundary (three dword loads per four pixels) and off it (byte loads)
        gi = G.Region("u8", img.shape, 4096, off, data=img)
        out = G.out_f32(want.shape, 4096)
        _ok(L.isx_images_u8_to_f32(gi.ptr, B, H, W, *mean, *std, int(cl), out.ptr, st), ("img offset", off))
        G.assert_clean([out], [gi], ("img offset", off))
        G.assert_bits(out, want, ("img offset", off))
