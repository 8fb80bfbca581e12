"""The routes of a folded trunk as chosen at fold time (model/nn_utils.fold_batch_norm): every _FusedBlock's `route` and every _ConvBiasAct's
`kind` for the three ResNets, read on the CPU.  Which kernels those routes launch is tests/test_gpu_trunk_routes.py."""
import re

import pytest
import torch.nn as nn

ROUTES = {
    "resnet18": 8 * [None],
    "resnet50": ["expand_dual"] + 2 * ["expand64"] + ["dual"] + 3 * ["expand128"] + ["dual"] + 5 * [None] + ["dual"] + 2 * [None],
    "resnet152": ["expand_dual"] + 2 * ["expand64"] + ["dual"] + 7 * ["expand128"] + ["dual"] + 35 * [None] + ["dual"] + 2 * [None],
}


def _blocks(name):
    from isx import backbones
    from model.nn_utils import _FusedBlock, extract_layers, fold_batch_norm
    trunk = fold_batch_norm(extract_layers(getattr(backbones, name)(pretrained=True).eval())[0])
    return trunk, [m for m in trunk if isinstance(m, _FusedBlock)]


@pytest.fixture(scope="module")
def resnet50():
    return _blocks("resnet50")


@pytest.mark.parametrize("name", sorted(ROUTES))
def test_block_routes_and_convolution_kinds(name, request):
    _, blocks = request.getfixturevalue("resnet50") if name == "resnet50" else _blocks(name)
    assert [b.route for b in blocks] == ROUTES[name]
    projections = [b.downsample for b in blocks if b.downsample is not None]
    if name == "resnet18":
        assert all(tuple(c.kind for c in b.convs) == ("conv3x3", "conv3x3") for b in blocks)
        assert [d.kind for d in projections] == 3 * ["torch"]
    else:
        assert all(tuple(c.kind for c in b.convs) == ("conv1x1", "conv3x3", "conv1x1") for b in blocks)
        assert [d.conv.stride for d in projections] == [(1, 1), (2, 2), (2, 2), (2, 2)]
        assert [d.kind for d in projections] == ["conv1x1"] + 3 * ["torch"]
    assert all(c.in_block and not c.plain for b in blocks for c in b.convs)
    assert all(d.plain and not d.in_block and not d.relu and not d.bias.any() for d in projections)


def test_stand_alone_3x3_goes_native_up_to_128_input_channels():
    from model.nn_utils import _ConvBiasAct
    kind = lambda cin, **kw: _ConvBiasAct(nn.Conv2d(cin, 64, 3, padding=1), True, **kw).kind
    assert kind(128) == "conv3x3"
    assert kind(160) == "torch" and kind(160, in_block=True) == "conv3x3"
    assert kind(48) == "torch" and kind(48, in_block=True) == "torch"


def test_folded_state_dict_names(resnet50):
    trunk, blocks = resnet50
    names = re.compile(r"\d+\.(convs\.\d+\.conv\.weight|convs\.\d+\.bias|downsample\.conv\.weight|downsample\.bias|cba\.conv\.weight|cba\.bias)")
    keys = list(trunk.state_dict())
    assert len(keys) == 2 + 2 * (3 * 16 + 4)                       # stem, 16 blocks of three convolutions, four projections
    assert all(names.fullmatch(k) for k in keys), [k for k in keys if not names.fullmatch(k)]
