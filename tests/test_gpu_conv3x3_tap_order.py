"""Longest tiles first in the position-major row order (pos_major_position, csrc/conv3x3_tile.hpp): within an image group the tiles of
isx_conv3x3_nhwc's 128x128 launches and of isx_conv3x3_expand128_nhwc run the nine-tap positions first, then the six-tap ones, then the
corners.  Only WHICH workgroup computes a tile changes, so every case must equal, bit for bit, the same call with the tiles in raster order
(isx_debug_set_conv_cfg(11): raster order under forced 128x128 tiles; 10 for the fused kernel, whose tiles are always 128 rows) and, for the
batches of 128 / 129 images, the CPU oracle on the images at the group boundaries.  Outputs lie between the guards and poison of
tests/_guards.py: a rank -> position mapping that is not a bijection computes one position twice and leaves another one poison.

Cases: 7x7 stride 1 (25 interior, 20 edge, 4 corner positions), 14x14 -> 7x7 stride 2 (36, 12, 1), 3x3 (1, 4, 4), 2x2 (corners only) and
1x1 (one position with one tap); B = 128 (one full group), 129 (a group of one image), 1665 = 13 * 128 + 1 (at 7x7: 686 tiles = one round of
the 512 resident workgroups + 174 tiles that run as 64-row tail tiles, the last group's with one live row or none); Cin = 64 and 128.
Reference: the torchvision ResNet trunk behind model/nn_utils.py:56-71 (extract_layers), model/siamese.py:20,107,151."""
import contextlib

import numpy as np
import pytest
import torch

import _guards as G
import oracle as O

pytestmark = pytest.mark.gpu

MAPS = [(7, 7, 1), (14, 14, 2), (3, 3, 1), (2, 2, 1), (1, 1, 1)]           # (H, W, stride)
BATCHES = [128, 129, 1665]
SLOTS = 256 * 2                                                            # resident 128-row workgroups (kWgPerCu128 = 2, csrc/gemm_tile.hpp)


def _lib():
    from isx._lib import lib
    return lib(), torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def conv_cfg(c):
    L = _lib()[0]
    try:
        L.isx_debug_set_conv_cfg(c)
        yield
    finally:
        L.isx_debug_set_conv_cfg(-1)


def _in(t, guard):
    """A device tensor as an fp32 operand between NaN guards (G.in_f32 without the trip through the host)."""
    r = G.Region("f32", tuple(t.shape), guard, data=None, guard_value=G.GUARD_IN_F32)
    r.body.copy_(t)
    return r


def _out_guard(B, Ho, Wo, Cout):
    return max(128 * Cout, 127 * Ho * Wo * Cout)                           # the 127 dead image slots of the last group


def _gen(seed, *shape, scale=1.0, relu=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randn(shape, device="cuda", generator=g) * scale
    return torch.relu_(t) if relu else t


def _images(B):
    return sorted({0, 127, 128, B - 1} & set(range(B)))


def _host(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("Cin", [64, 128])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("H,W,stride", MAPS)
def test_conv3x3_tap_order(H, W, stride, B, Cin):
    Cout, res, relu = (128 if Cin == 64 else 192), B != 128, Cin == 64     # one n-tile / a ragged second one
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert G.pos_major_rows(B, H, W, Cin, Ho, Wo, Cout, (Cout + 63) // 64) > 0, "the shape must run position-major"
    if B == 1665 and Ho * Wo == 49:
        assert G.tail_split_rows(G.pos_major_rows(B, H, W, Cin, Ho, Wo, Cout, (Cout + 63) // 64), Cout, SLOTS) > 0, "the shape must take the tail split"
    seed = 1000 * H + 10 * stride + B + Cin
    x, w, b = _gen(seed, B, H, W, Cin, relu=True), _gen(seed + 1, Cout, 3, 3, Cin, scale=(9 * Cin) ** -0.5), _gen(seed + 2, Cout)
    r = _gen(seed + 3, B, Ho, Wo, Cout) if res else None
    ins = (_in(x, 128 * Cin * min(H * W, 64)), _in(w, 128 * 9 * Cin), _in(b, 256), None if r is None else _in(r, _out_guard(B, Ho, Wo, Cout)))
    L, st = _lib()
    outs = {}
    for cfg in (0, 11):                                                    # longest first | raster order, both in 128x128 tiles (+ 64x64 tails)
        out = G.out_f32((B, Ho, Wo, Cout), _out_guard(B, Ho, Wo, Cout))
        with conv_cfg(cfg):
            rc = L.isx_conv3x3_nhwc(ins[0].ptr, B, H, W, Cin, ins[1].ptr, Cout, stride, ins[2].ptr, G.ptr(ins[3]), int(relu), out.ptr, st)
        assert rc == 0, (cfg, L.isx_last_error())
        G.assert_clean([out], ins, ("conv cfg", cfg))
        outs[cfg] = out
    assert torch.equal(outs[0].raw(), outs[11].raw()), ("longest-first order differs from the raster order", int((outs[0].raw() != outs[11].raw()).sum()))
    if B <= 129:
        for i in _images(B):
            want = O.conv3x3_nhwc(_host(x[i:i + 1]), _host(w), _host(b), stride, _host(r[i:i + 1]) if res else None, relu)
            G.assert_bits(outs[0].body[i:i + 1], want, ("oracle, image", i))


@pytest.mark.parametrize("Cin", [64, 128])
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("H,W", [(h, w) for h, w, s in MAPS if s == 1])    # the fused kernel is stride 1 only
def test_expand128_tap_order(H, W, B, Cin):
    Cout, res, relu = (128 if Cin == 64 else 256), B != 129, Cin == 128
    assert G.pos_major_rows(B, H, W, Cin, H, W, Cout, 2) > 0, "the shape must run position-major"
    if B == 1665 and H * W == 49:
        assert G.tail_split_rows(G.pos_major_rows(B, H, W, Cin, H, W, Cout, 2), 128, SLOTS) > 0, "the shape must take the tail split"
    seed = 2000 * H + B + Cin
    x, w2, b2 = _gen(seed, B, H, W, Cin, relu=True), _gen(seed + 1, 128, 3, 3, Cin, scale=(9 * Cin) ** -0.5), _gen(seed + 2, 128)
    w3, b3 = _gen(seed + 3, Cout, 128, scale=128 ** -0.5), _gen(seed + 4, Cout)
    r = _gen(seed + 5, B, H, W, Cout) if res else None
    ins = (_in(x, 128 * Cin * min(H * W, 64)), _in(w2, 128 * 9 * Cin), _in(b2, 256), _in(w3.t().contiguous(), 128 * Cout), _in(b3, 256),
           None if r is None else _in(r, _out_guard(B, H, W, Cout)))
    L, st = _lib()
    outs = {}
    for cfg in (-1, 10):                                                   # longest first | raster order
        out = G.out_f32((B, H, W, Cout), _out_guard(B, H, W, Cout))
        with conv_cfg(cfg):
            rc = L.isx_conv3x3_expand128_nhwc(ins[0].ptr, B, H, W, Cin, ins[1].ptr, ins[2].ptr, ins[3].ptr, Cout, ins[4].ptr, G.ptr(ins[5]), int(relu), out.ptr, st)
        assert rc == 0, (cfg, L.isx_last_error())
        G.assert_clean([out], ins, ("conv cfg", cfg))
        outs[cfg] = out
    assert torch.equal(outs[-1].raw(), outs[10].raw()), ("longest-first order differs from the raster order", int((outs[-1].raw() != outs[10].raw()).sum()))
    if B <= 129:
        for i in _images(B):
            mid = O.conv3x3_nhwc(_host(x[i:i + 1]), _host(w2), _host(b2), 1, None, True)
            want = O.conv1x1_nhwc(mid.reshape(-1, 128), _host(w3), _host(b3), _host(r[i]).reshape(-1, Cout) if res else None, relu).reshape(1, H, W, Cout)
            G.assert_bits(outs[-1].body[i:i + 1], want, ("oracle, image", i))
