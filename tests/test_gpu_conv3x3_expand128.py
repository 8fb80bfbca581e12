"""isx_conv3x3_expand128_nhwc (conv3x3_expand128_kernel, csrc/expand_kernel.hpp): conv2 (3x3 -> 128 channels, ReLU) + conv3 (1x1 -> Cout,
+ residual, ReLU) of an identity Bottleneck as ONE kernel -- the 128 x 128 accumulator tile of the 3x3 convolution goes registers -> LDS and
feeds the expansion's MFMA loop.  Bit for bit the two separate libisx kernels (isx_conv3x3_nhwc, then isx_conv1x1_nhwc) and the oracle's
composition of the two, in both row orders (position-major / pixel-major) and through the 64-row tail tiles; the CPU test at the end checks
that bad shapes are refused before any launch."""
import numpy as np
import pytest
import torch

import oracle as O


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _inputs(B, H, W, Cin, Cout, res):
    rng = np.random.default_rng(B * 100 + H * 10 + W + Cin + Cout)
    x = np.maximum(rng.standard_normal((B, H, W, Cin), dtype=np.float32), 0)
    w2 = rng.standard_normal((128, 3, 3, Cin), dtype=np.float32) * np.float32((9 * Cin) ** -0.5)
    b2 = rng.standard_normal(128, dtype=np.float32)
    w3 = rng.standard_normal((Cout, 128), dtype=np.float32) * np.float32(128 ** -0.5)
    b3 = rng.standard_normal(Cout, dtype=np.float32)
    r = rng.standard_normal((B, H, W, Cout), dtype=np.float32) if res else None
    return x, w2, b2, w3, b3, r


def _check(B, H, W, Cin, Cout, res, relu, oracle_images=None):
    """fused (automatic row order) == fused (pixel-major everywhere, debug cfg 8) == two kernels == oracle, as int32 bit patterns.
    oracle_images: the images the oracle evaluates (every image is an independent convolution); None = all of them."""
    from isx import ops
    from isx._lib import lib
    x, w2, b2, w3, b3, r = _inputs(B, H, W, Cin, Cout, res)
    xt = dev(x).permute(0, 3, 1, 2)
    rt = dev(r).permute(0, 3, 1, 2) if res else None
    w3t = dev(np.ascontiguousarray(w3.T))
    set_cfg = lib().isx_debug_set_conv_cfg
    try:
        got = host(ops.conv3x3_expand128_nhwc(xt, dev(w2), dev(b2), w3t, dev(b3), rt, relu).permute(0, 2, 3, 1))
        set_cfg(8)
        got8 = host(ops.conv3x3_expand128_nhwc(xt, dev(w2), dev(b2), w3t, dev(b3), rt, relu).permute(0, 2, 3, 1))
    finally:
        set_cfg(-1)
    mid = ops.conv3x3_nhwc(xt, dev(w2), dev(b2), 1, None, True)
    two = host(ops.conv1x1_nhwc(mid, dev(w3), dev(b3), rt, relu).permute(0, 2, 3, 1))
    np.testing.assert_array_equal(got.view(np.int32), two.view(np.int32))
    np.testing.assert_array_equal(got8.view(np.int32), two.view(np.int32))
    sel = np.arange(B) if oracle_images is None else np.asarray(oracle_images)
    want_mid = O.conv3x3_nhwc(x[sel], w2, b2, 1, None, True)
    want = O.conv1x1_nhwc(want_mid.reshape(-1, 128), w3, b3, r[sel].reshape(-1, Cout) if res else None, relu).reshape(len(sel), H, W, Cout)
    np.testing.assert_array_equal(got[sel].view(np.int32), want.view(np.int32))


# position-major (B >= 128, small maps): one position per tile; a full image group, a group of one image, two groups + one image;
# corner / edge / interior positions (1x1: every tap but the centre is padding; 3x5: an interior position with all nine taps)
@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,Cin,Cout,res,relu", [
    (128, 1, 1, 64, 128, True, True), (129, 1, 1, 128, 512, False, False), (257, 1, 1, 64, 512, True, False),
    (128, 2, 2, 128, 128, False, True), (129, 2, 2, 64, 512, True, True), (257, 2, 2, 128, 128, True, True),
    (128, 3, 3, 64, 512, False, False), (129, 3, 3, 128, 128, True, False), (257, 3, 3, 64, 128, False, True),
    (128, 3, 5, 128, 512, True, True), (129, 3, 5, 64, 128, True, True), (257, 3, 5, 64, 512, False, True)])
def test_position_major(B, H, W, Cin, Cout, res, relu):
    _check(B, H, W, Cin, Cout, res, relu)


# one launch of a little over one round of the 512 resident workgroups: 14 image groups x 49 positions = 686 tiles, of which the last 174 run
# as 348 tail tiles of 64 rows -- whole groups (both halves live), and the last group of ONE image (a half with 1 live and 63 dead rows, a
# half without a live row).  The two-kernel comparison covers every output.  The oracle evaluates whole images (all 49 positions, the border
# ones included), chosen from the split: one whose positions all lie in 128-row tiles, one of each 64-row half of a group that runs as tail
# tiles throughout, and the lone image of the last group.
@pytest.mark.gpu
def test_tail_tiles():
    B, P, slots = 13 * 128 + 1, 49, 512
    groups = (B + 127) // 128
    tiles = groups * P                                     # virtual 128-row tiles, image group outermost
    split_tile = tiles // slots * slots                    # gemm_tail_split_rows: the tiles of the whole rounds stay 128 rows tall
    assert 0 < tiles - split_tile <= slots * 4 // 5, "the shape must take the tail split"
    g_big = split_tile // P - 1                            # last group whose positions all precede the split
    g_tail = -(-split_tile // P)                           # first group whose positions all follow it
    assert g_big >= 0 and g_tail < groups - 1, "a whole group on either side of the split"
    images = [g_big * 128 + 5, g_tail * 128 + 3, g_tail * 128 + 64 + 28, B - 1]
    _check(B, 7, 7, 64, 128, True, True, oracle_images=images)


# pixel-major: B < 128 (a 128-row tile spans images; rows past the end in the last tile), 9x11 and 7x7; then the row counts at which the
# last 128-row tile of a launch without a tail has a single live row (129 = 128 + 1, 385 = 3 * 128 + 1), ONE row in all, and fewer than 64
@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,Cin,Cout,res,relu", [(3, 9, 11, 64, 512, True, True), (64, 7, 7, 64, 128, True, True), (3, 9, 11, 128, 128, False, False),
                                                     (3, 1, 43, 64, 512, True, True), (5, 7, 11, 128, 128, True, True), (1, 1, 1, 64, 128, True, True),
                                                     (1, 5, 5, 64, 512, False, True)])
def test_pixel_major(B, H, W, Cin, Cout, res, relu):
    _check(B, H, W, Cin, Cout, res, relu)


def test_bad_shapes_refused_without_gpu():
    """Shape checks come before any pointer is touched or any kernel launched; an empty batch is a no-op."""
    from isx import _lib, ops
    lib = _lib.lib()
    f = lib.isx_conv3x3_expand128_nhwc
    assert f(None, 2, 7, 7, 64, None, None, None, 192, None, None, 1, None, None) == -1 and b"multiple of 128" in lib.isx_last_error()
    assert f(None, 2, 7, 7, 96, None, None, None, 512, None, None, 1, None, None) == -1 and b"multiple of 64" in lib.isx_last_error()
    assert f(None, 2, 0, 7, 64, None, None, None, 512, None, None, 1, None, None) == -1 and b"bad shape" in lib.isx_last_error()
    assert f(None, 2, 7, 7, 64, None, None, None, 512, None, None, 1, None, None) == -1 and b"null pointer" in lib.isx_last_error()
    assert f(None, 0, 7, 7, 64, None, None, None, 512, None, None, 1, None, None) == 0
    x = torch.zeros(2, 64, 7, 7).contiguous(memory_format=torch.channels_last)
    with pytest.raises(_lib.IsxError, match=r"\(128, 3, 3, Cin\)"):         # mid weight with 64 output channels
        ops.conv3x3_expand128_nhwc(x, torch.zeros(64, 3, 3, 64), torch.zeros(64), torch.zeros(128, 512), torch.zeros(512))
    with pytest.raises(_lib.IsxError, match=r"\(128, 3, 3, Cin\)"):         # mid weight for another Cin
        ops.conv3x3_expand128_nhwc(x, torch.zeros(128, 3, 3, 32), torch.zeros(128), torch.zeros(128, 512), torch.zeros(512))
    with pytest.raises(_lib.IsxError, match="multiple of 128"):
        ops.conv3x3_expand128_nhwc(x, torch.zeros(128, 3, 3, 64), torch.zeros(128), torch.zeros(128, 192), torch.zeros(192))
    with pytest.raises(_lib.IsxError, match="multiple of 64"):
        x96 = torch.zeros(2, 96, 7, 7).contiguous(memory_format=torch.channels_last)
        ops.conv3x3_expand128_nhwc(x96, torch.zeros(128, 3, 3, 96), torch.zeros(128), torch.zeros(128, 512), torch.zeros(512))
    with pytest.raises(_lib.IsxError, match="CUDA"):                         # good shapes, CPU tensor
        ops.conv3x3_expand128_nhwc(x, torch.zeros(128, 3, 3, 64), torch.zeros(128), torch.zeros(128, 512), torch.zeros(512))
