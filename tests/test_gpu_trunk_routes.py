"""Which kernel runs which layer of a folded trunk (model/nn_utils.fold_batch_norm): the sequence of libisx launches of one small forward,
read from ops.KERNEL_TIMER, and the convolutions left with torch, read from nn_utils.TORCH_CONV_CALLS.  Under autograd and on a tensor that
is dense in both memory formats no libisx convolution runs.  The CPU side (the routes as chosen at fold time) is tests/test_trunk_routes.py."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

S, P, T, D, E, E128 = ("isx_stem7x7_pool_nhwc", "isx_conv1x1_nhwc", "isx_conv3x3_nhwc", "isx_conv1x1_dual_nhwc", "isx_conv3x3_expand_nhwc",
                       "isx_conv3x3_expand128_nhwc")
# isx_conv3x3_expand_dual_nhwc (first block of stage 1) is recorded under E's name
RESNET50 = [S] + 3 * [P, E] + [P, T, D] + 3 * [P, E128] + [P, T, D] + 5 * [P, T, P] + [P, T, D] + 2 * [P, T, P]
RESNET18 = [S] + 16 * [T]


def _folded(name):
    from isx import backbones
    from model.nn_utils import extract_layers, fold_batch_norm
    f = fold_batch_norm(extract_layers(getattr(backbones, name)(pretrained=True).eval())[0])
    return f.cuda().to(memory_format=torch.channels_last)


def _batch():
    g = torch.Generator(device="cuda").manual_seed(7)
    return torch.randn(2, 3, 64, 64, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)


def _recorded(fn):
    """(result of fn(), names of the libisx trunk kernels it launched, convolutions it left with torch)."""
    from isx import ops
    from model import nn_utils
    nn_utils.TORCH_CONV_CALLS.clear()
    old, ops.KERNEL_TIMER = ops.KERNEL_TIMER, []
    try:
        out = fn()
        names = [rec[0] for rec in ops.KERNEL_TIMER]
    finally:
        ops.KERNEL_TIMER = old
    torch.cuda.synchronize()
    return out, names, dict(nn_utils.TORCH_CONV_CALLS)


@pytest.fixture(scope="module")
def resnet50():
    return _folded("resnet50")


def _no_grad_forward(net, x):
    with torch.no_grad():
        return net(x)


def test_resnet50_kernel_sequence(resnet50):
    assert len(RESNET50) == 43
    y, names, torch_convs = _recorded(lambda: _no_grad_forward(resnet50, _batch()))
    assert y.shape == (2, 2048, 2, 2) and torch.isfinite(y).all()
    assert names == RESNET50
    assert torch_convs == {}


def test_resnet18_kernel_sequence():
    y, names, torch_convs = _recorded(lambda: _no_grad_forward(_folded("resnet18"), _batch()))
    assert y.shape == (2, 512, 2, 2) and torch.isfinite(y).all()
    assert names == RESNET18
    # the strided 1x1 projections: no libisx kernel takes them on their own
    assert torch_convs == {((1, 1), (2, 2), 64, 128): 1, ((1, 1), (2, 2), 128, 256): 1, ((1, 1), (2, 2), 256, 512): 1}


def test_autograd_forward_records_no_kernel_and_agrees(resnet50):
    x = _batch()
    want = _no_grad_forward(resnet50, x)
    with torch.enable_grad():
        got, names, _ = _recorded(lambda: resnet50(x))
    assert names == []
    # the tolerance of folded against unfolded in test_gpu_dropin.test_bias_act_and_folded_trunk
    assert float((got - want).abs().max()) <= 2e-4 * float(want.abs().max())


def test_dense_in_both_formats_takes_the_torch_route():
    """A (B, C, 1, 1) tensor is contiguous in both memory formats: it counts as NCHW -- torch's convolution and the in-place epilogue, no libisx
    convolution."""
    from model.nn_utils import _ConvBiasAct
    torch.manual_seed(3)
    m = _ConvBiasAct(nn.Conv2d(64, 64, 1, bias=True), True).cuda()
    x = torch.randn(2, 64, 1, 1, device="cuda")
    assert x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last)
    got, names, torch_convs = _recorded(lambda: _no_grad_forward(m, x))
    assert names == [] and torch_convs == {((1, 1), (1, 1), 64, 64): 1}
    with torch.no_grad():
        want = torch.relu(m.conv(x) + m.bias.view(1, -1, 1, 1))
    assert torch.equal(got, want)
