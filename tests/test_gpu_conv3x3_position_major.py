"""The position-major row order of isx_conv3x3_nhwc (csrc/conv3x3_tile.hpp): on small maps a 128x128 tile (and a 64x64 tail tile) holds ONE
output position of up to 128 images, and the k loop visits only the filter taps that are not padding at that position.

Every case is checked bit for bit against two yardsticks: the CPU oracle's fma chains (as tests/test_gpu_layer_shapes.py does) and the same
call with the debug hook forcing the old pixel-major row order (isx_debug_set_conv_cfg(8)).  The new order runs twice: with 128x128 tiles forced
(cfg 0: the tiny shapes below would otherwise get 64x64 tiles, which keep the old order) and with the automatic pick.

Cases: the smallest maps at which the construction can go wrong -- 1x1 (only the centre tap survives), 2x2 (every position a corner), 3x3,
7x7, 14x14 -> 7x7 and an odd 5x5 -> 3x3 at stride 2, a map that is not square; batches of 128, 129 and 257 images (a group that holds one
image, a ragged last group); Cout = 192 (a ragged n-tile); with / without residual and ReLU; one launch of ~1.3 rounds of resident workgroups,
whose 64x64 tail tiles carry position-uniform rows (and, with B = 13 * 128 + 1, tail tiles without any live row); B = 64, which is not eligible.
Reference: the torchvision ResNet trunk behind model/nn_utils.py:56-71 (extract_layers), model/siamese.py:20,107,151."""
import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    from isx import ops as o
    return o


@pytest.fixture()
def conv_cfg():
    from isx._lib import lib
    conv = lib().isx_debug_set_conv_cfg
    yield conv
    conv(-1)


def _split_batch(P, cout):
    """Images such that the VIRTUAL row count (whole groups of 128 images) is ~1.3 rounds of the 512 resident 128x128 workgroups, with one
    image in the last group."""
    tn = (cout + 127) // 128
    rows_per_round = (512 // tn) * 128
    groups = -(-int(1.3 * rows_per_round) // (P * 128))
    return (groups - 1) * 128 + 1


# (H, W, stride, B, Cin, Cout, residual, relu)
CASES = [
    (1, 1, 1, 128, 64, 64, False, True),
    (2, 2, 1, 129, 64, 192, True, True),
    (2, 2, 2, 128, 128, 64, False, False),
    (3, 3, 1, 257, 128, 64, True, False),
    (7, 7, 1, 129, 128, 192, False, False),
    (14, 14, 2, 257, 64, 64, True, True),
    (5, 5, 2, 129, 64, 192, False, True),
    (3, 5, 1, 128, 64, 64, True, True),
    (7, 7, 1, _split_batch(49, 64), 64, 64, True, True),
    (7, 7, 1, 64, 64, 64, True, True),
]


@pytest.mark.parametrize("H,W,stride,B,Cin,Cout,res,relu", CASES)
def test_conv3x3_position_major(ops, conv_cfg, H, W, stride, B, Cin, Cout, res, relu):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    gen = torch.Generator(device="cuda").manual_seed(1000 * H + 100 * W + 10 * stride + B + Cin + Cout)
    x = torch.relu_(torch.randn((B, H, W, Cin), device="cuda", generator=gen))
    w = torch.randn((Cout, 3, 3, Cin), device="cuda", generator=gen) * (9 * Cin) ** -0.5
    b = torch.randn((Cout,), device="cuda", generator=gen)
    r = torch.randn((B, Ho, Wo, Cout), device="cuda", generator=gen) if res else None
    outs = {}
    for c in (8, 0, -1):                                  # old row order | 128x128 tiles forced (position-major where eligible) | automatic
        conv_cfg(c)
        y = ops.conv3x3_nhwc(x.permute(0, 3, 1, 2), w, b, stride, r.permute(0, 3, 1, 2) if res else None, relu)
        outs[c] = y.permute(0, 2, 3, 1).contiguous()
    conv_cfg(-1)
    old = outs[8].view(torch.int32)
    assert torch.equal(old, outs[0].view(torch.int32))
    assert torch.equal(old, outs[-1].view(torch.int32))
    # the oracle on the images at the group boundaries (first / last of group 0, first of group 1, last image) and, past the 128x128 / 64x64
    # split, on the two ends of the group that straddles it
    imgs = {0, 127, 128, B - 1}
    if B > 1024:
        imgs |= {1280, 1343, 1344, 1407}
    for i in sorted(j for j in imgs if 0 <= j < B):
        want = O.conv3x3_nhwc(host(x[i:i + 1]), host(w), host(b), stride, host(r[i:i + 1]) if res else None, relu)
        np.testing.assert_array_equal(host(outs[0][i:i + 1]), want)
