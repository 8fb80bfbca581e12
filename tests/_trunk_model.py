"""Model of the folded ResNet trunk (model/nn_utils.fold_batch_norm): what every folded module computes on an input the libisx kernels take,
written as ONE fixed composition of oracle calls on the module's own parameters.  include/isx.h states that each fused kernel has the bits of
the unfused sequence, so the composition below is the whole trunk's arithmetic; tests/test_gpu_trunk_modules.py holds the modules to it bit
for bit, tests/test_trunk_model.py holds it to a float64 evaluation of the UNFOLDED block and shows that each wiring mistake in WRONGS moves it.

numpy and the oracle only; torch only builds the blocks and hands over their parameters.  The model reads `convs[i].conv.weight`,
`convs[i].bias`, `downsample.conv.weight` and the strides -- never `w_cat()`, `w3t()`, `w_ohwi()`, `route`, `kind` or a `relu` flag: those are
what it checks.  In a residual block every convolution has a ReLU behind it, the last one behind the shortcut add.

Compositions (BHWC float32 arrays):
  Bottleneck, no projection     c1 = conv1x1(x) -> c2 = conv3x3(c1, stride) -> relu(conv1x1(c2) + bias + x)
  Bottleneck, 1x1 projection    c1, c2 -> conv1x1_dual(c2, x, [W3 | Wd], merged bias, projection stride): ONE two-level sum over c2's channels,
                                then the strided input's.  `unfused=True`: the projection as a sum of its own (conv1x1 of the strided input, zero
                                bias, no ReLU), added as the residual of conv3 -- what a block computes whose `route` is None
  BasicBlock                    conv3x3(x, stride) -> relu(conv3x3(c1) + bias + shortcut); a projection shortcut is always a sum of its own
The merged bias is the module's stored `convs[-1].bias`."""
import zlib

import numpy as np

import oracle as O

WRONGS = {
    "proj_bias_dropped": "the last convolution keeps its own bias: the projection's is lost",
    "proj_bias_twice": "the projection bias is added to the merged bias once more",
    "residual_is_input": "the block input is the residual although a projection exists (the shapes must allow it)",
    "proj_offset": "the strided projection reads (ho * stride + 1, wo * stride + 1)",
    "stride_in_conv1": "the block's stride sits in conv1 instead of conv2 (torchvision's v1 against v1.5 Bottleneck)",
    "relu_before_residual": "ReLU on the last convolution's own sum, the shortcut added behind it",
    "no_relu_after_conv2": "no ReLU behind the convolution in front of the last (conv2 of a Bottleneck, conv1 of a BasicBlock)",
    "w_cat_swapped": "[Wd | W3] against the operand [t ; x]",
    "ohwi_kh_kw_swapped": "the 3x3 weights as permute(0, 3, 2, 1): kh and kw swapped",
}
_NEED_UNMERGED = ("proj_bias_dropped", "proj_bias_twice")

P, T, D, E64, E128 = "isx_conv1x1_nhwc", "isx_conv3x3_nhwc", "isx_conv1x1_dual_nhwc", "isx_conv3x3_expand_nhwc", "isx_conv3x3_expand128_nhwc"

# id -> block (type, inplanes, planes, stride, projection), the route and kinds its fold must have, the launches of one native forward
# (isx_conv3x3_expand_dual_nhwc is recorded under E64's name), the inputs (B, H, W[, images compared]) and the WRONGS that cannot apply, by name.
# The channel counts are the smallest that select each route, the maps the smallest that keep the edge: odd, non-square, one that shrinks to
# 1 x 1, and B >= 128 where the position-major 3x3 tiles take over.  `dual_same` is not in the issue's table: a projection between equal shapes,
# the one place where "residual = block input" can be written down.
_NO_PROJ = ("proj_bias_dropped", "proj_bias_twice", "residual_is_input", "proj_offset", "w_cat_swapped")
CASES = {
    "expand_dual": dict(block=("bottleneck", 64, 64, 1, True), route="expand_dual", kinds=("conv1x1", "conv3x3", "conv1x1"), proj_kind="conv1x1",
                        launches=[P, E64], shapes=[(2, 5, 7)], exact=True,
                        # 64 -> 256 channels: the input is no residual; stride 1: no sampling phase, no stride to misplace
                        not_applicable=("residual_is_input", "proj_offset", "stride_in_conv1")),
    "expand64": dict(block=("bottleneck", 256, 64, 1, False), route="expand64", kinds=("conv1x1", "conv3x3", "conv1x1"), proj_kind=None,
                     launches=[P, E64], shapes=[(2, 5, 7)], dense_shapes=[(1, 1, 1)], exact=True, not_applicable=_NO_PROJ + ("stride_in_conv1",)),
    "expand128": dict(block=("bottleneck", 512, 128, 1, False), route="expand128", kinds=("conv1x1", "conv3x3", "conv1x1"), proj_kind=None,
                      launches=[P, E128], shapes=[(2, 5, 7), (128, 3, 3, (0, 64, 127))], exact=True,
                      not_applicable=_NO_PROJ + ("stride_in_conv1",)),
    "dual_s2": dict(block=("bottleneck", 256, 128, 2, True), route="dual", kinds=("conv1x1", "conv3x3", "conv1x1"), proj_kind="torch",
                    launches=[P, T, D], shapes=[(2, 7, 5), (2, 2, 2), (129, 6, 5, (0, 128))], exact=True,
                    not_applicable=("residual_is_input",)),                       # 256 -> 512 channels at half the size
    "dual_same": dict(block=("bottleneck", 256, 64, 1, True), route="dual", kinds=("conv1x1", "conv3x3", "conv1x1"), proj_kind="conv1x1",
                      launches=[P, T, D], shapes=[(2, 5, 7)], exact=True, not_applicable=("proj_offset", "stride_in_conv1")),
    "plain": dict(block=("bottleneck", 128, 32, 1, False), route=None, kinds=("conv1x1", "conv3x3", "conv1x1"), proj_kind=None,
                  launches=[P, T, P], shapes=[(2, 5, 7)], exact=True, not_applicable=_NO_PROJ + ("stride_in_conv1",)),
    "basic": dict(block=("basic", 64, 64, 1, False), route=None, kinds=("conv3x3", "conv3x3"), proj_kind=None,
                  launches=[T, T], shapes=[(3, 5, 5)], exact=True, not_applicable=_NO_PROJ + ("stride_in_conv1",)),
    # tolerance cases: one convolution of the block is torch's
    "basic_s2": dict(block=("basic", 64, 128, 2, True), route=None, kinds=("conv3x3", "conv3x3"), proj_kind="torch",
                     launches=[T, T], torch_convs={((1, 1), (2, 2), 64, 128): 1}, shapes=[(2, 7, 5)], exact=False,
                     # no [W3 | Wd] in a BasicBlock, whose stride IS conv1's
                     not_applicable=("residual_is_input", "w_cat_swapped", "stride_in_conv1")),
    "mixed": dict(block=("bottleneck", 192, 48, 1, False), route=None, kinds=("conv1x1", "torch", "conv1x1"), proj_kind=None,
                  launches=[P, P], torch_convs={((3, 3), (1, 1), 48, 48): 1}, shapes=[(2, 5, 7)], exact=False,
                  not_applicable=_NO_PROJ + ("stride_in_conv1",)),
}
EXACT = [c for c in CASES if CASES[c]["exact"]]


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def randomise_bn(net, seed):
    """Non-trivial statistics for every BatchNorm of `net` (on the CPU): mean N(0, 0.1), variance U(0.5, 1.5), weight U(0.5, 1.5), bias
    N(0, 0.1), and the sign of about one weight in eight flipped, so that some folded scales are negative.  Without this every folded bias of a
    default-initialised trunk is exactly 0.0 and no bias wiring shows."""
    import torch
    import torch.nn as nn
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1, generator=g)
                m.running_var.uniform_(0.5, 1.5, generator=g)
                m.weight.uniform_(0.5, 1.5, generator=g)
                m.bias.normal_(0, 0.1, generator=g)
                m.weight[torch.rand(m.weight.shape, generator=g) < 0.125] *= -1
    return net


def make_block(cid):
    """The unfolded block of a case: seeded ResNet initialisation (kaiming normal, fan out), randomised BatchNorms, eval mode, on the CPU."""
    import torch
    import torch.nn as nn
    from isx import backbones
    kind, cin, planes, stride, proj = CASES[cid]["block"]
    cls = backbones.Bottleneck if kind == "bottleneck" else backbones.BasicBlock
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(_seed(cid, "weights"))
        down = None
        if proj:
            down = nn.Sequential(nn.Conv2d(cin, planes * cls.expansion, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * cls.expansion))
        blk = cls(cin, planes, stride, down)
        for m in blk.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
    return randomise_bn(blk, _seed(cid, "bn")).eval()


def fold(block):
    """The _FusedBlock of one unfolded block."""
    import torch.nn as nn
    from model.nn_utils import fold_batch_norm
    return fold_batch_norm(nn.Sequential(block))[1]


def case_inputs(cid, dense=False):
    """[(x_bhwc, images to compare or None)] of a case: relu(N(0, 1)) as a block sees it, one array per shape of the table, and behind them the
    first shape once more with its first image negated (every pre-activation of that image moves, many change sign: a missing ReLU shows).
    `dense`: the shapes whose maps are dense in both memory formats (the torch route) instead."""
    case = CASES[cid]
    cin = case["block"][1]
    out = []
    for shape in case.get("dense_shapes", []) if dense else case["shapes"]:
        rng = np.random.default_rng(_seed(cid, shape[:3]))
        x = np.maximum(rng.standard_normal(shape[:3] + (cin,), dtype=np.float32), 0)
        out.append((x, shape[3] if len(shape) > 3 else None))
    if not dense:
        neg = out[0][0].copy()
        neg[0] = -neg[0]
        out.append((neg, None))
    return out


def _np(t):
    return t.detach().cpu().numpy().astype(np.float32)


def _ohwi(w, swapped=False):
    return np.ascontiguousarray(w.transpose(0, 3, 2, 1) if swapped else w.transpose(0, 2, 3, 1))


def _c1(x, w, bias, res=None, relu=True):
    B, H, W, C = x.shape
    co = w.shape[0]
    y = O.conv1x1_nhwc(x.reshape(-1, C), w.reshape(co, -1), bias, None if res is None else res.reshape(-1, co), relu)
    return y.reshape(B, H, W, co)


def unmerged_biases(block):
    """(b3, bd) of an unfolded block with a projection: the two folded biases before the merge, as torch's fuse_conv_bn_eval gives them."""
    import copy
    from torch.nn.utils.fusion import fuse_conv_bn_eval
    last = ("conv3", "bn3") if hasattr(block, "conv3") else ("conv2", "bn2")
    f = lambda c, n: _np(fuse_conv_bn_eval(copy.deepcopy(c).eval(), copy.deepcopy(n).eval()).bias)
    return f(getattr(block, last[0]), getattr(block, last[1])), f(block.downsample[0], block.downsample[1])


def block_reference(fb, x_bhwc, wrong=None, unfused=False, unmerged=None):
    """float32 BHWC output of the folded block `fb` on `x_bhwc` (module docstring).  `wrong`: a key of WRONGS, the same composition with that
    one mistake; the two bias mistakes need `unmerged` = unmerged_biases(unfolded block)."""
    assert wrong is None or wrong in WRONGS, wrong
    x = np.ascontiguousarray(x_bhwc, np.float32)
    ws = [_np(c.conv.weight) for c in fb.convs]
    bs = [_np(c.bias) for c in fb.convs]
    st = [c.conv.stride[0] for c in fb.convs]
    swapped = wrong == "ohwi_kh_kw_swapped"
    mid_relu = wrong != "no_relu_after_conv2"
    bias = bs[-1]
    if wrong in _NEED_UNMERGED:
        b3, bd = unmerged
        bias = b3 if wrong == "proj_bias_dropped" else (b3 + bd) + bd                 # float32 adds, as the fold's own
    if len(ws) == 3:
        if wrong == "stride_in_conv1":
            st = [st[1], st[0], st[2]]
        c1 = _c1(x[:, ::st[0], ::st[0]], ws[0], bs[0])
        t = O.conv3x3_nhwc(c1, _ohwi(ws[1], swapped), bs[1], st[1], None, mid_relu)
        last = lambda res, b=bias: _c1(t, ws[2], b, res, True)
    else:
        t = O.conv3x3_nhwc(x, _ohwi(ws[0], swapped), bs[0], st[0], None, mid_relu)
        last = lambda res, b=bias: O.conv3x3_nhwc(t, _ohwi(ws[1], swapped), b, st[1], res, True)
    if fb.downsample is None:
        if wrong == "relu_before_residual":
            return last(None) + x
        return last(x)
    if wrong == "residual_is_input":
        return last(x)
    wd, sd = _np(fb.downsample.conv.weight), fb.downsample.conv.stride[0]
    wd = wd.reshape(wd.shape[0], -1)
    xp = x
    if wrong == "proj_offset":
        H, W = x.shape[1:3]
        xp = np.ascontiguousarray(x[:, np.minimum(np.arange(H) + 1, H - 1)][:, :, np.minimum(np.arange(W) + 1, W - 1)])
    shortcut = lambda: _c1(np.ascontiguousarray(xp[:, ::sd, ::sd]), wd, np.zeros(wd.shape[0], np.float32), None, False)
    if wrong == "relu_before_residual":
        return last(None) + shortcut()
    if len(ws) == 3 and not unfused:
        w3 = ws[2].reshape(ws[2].shape[0], -1)
        w_cat = np.concatenate([wd, w3] if wrong == "w_cat_swapped" else [w3, wd], 1)
        return O.conv1x1_dual_nhwc(t, xp, w_cat, bias, sd, True)
    return last(shortcut())


def stem_reference(stem, x_bhwc):
    """float32 BHWC output of a folded _StemConvPool: conv 7x7 / 2 + bias + ReLU + max-pool 3 / 2 / 1 as the one-kernel stem sums it."""
    return O.stem7x7_pool_nhwc(x_bhwc, _ohwi(_np(stem.cba.conv.weight)), _np(stem.cba.bias))


def trunk_modules(trunk):
    """(stem, [blocks]) of a folded ResNet `features`."""
    from model.nn_utils import _ChannelsLastEntry, _FusedBlock, _StemConvPool
    mods = list(trunk)
    assert isinstance(mods[0], _ChannelsLastEntry) and isinstance(mods[1], _StemConvPool) and all(isinstance(m, _FusedBlock) for m in mods[2:])
    return mods[1], mods[2:]


def trunk_reference(trunk, x_bhwc, blocks=None):
    """The two references chained over a folded ResNet `features`; `blocks`: only that many blocks behind the stem."""
    stem, blks = trunk_modules(trunk)
    y = stem_reference(stem, x_bhwc)
    for b in blks[:blocks]:
        y = block_reference(b, y)
    return y


# ---- float64 evaluations of the FOLDED weights: the arbiter R of the tolerance cases (max|out - R| <= margin * max|reference - R|)

def _conv64(x, w_ohwi, stride, pad):
    B, H, W, _ = x.shape
    co, k = w_ohwi.shape[:2]
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    xp = np.pad(x.astype(np.float64), ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    w = w_ohwi.astype(np.float64)
    y = np.zeros((B, Ho, Wo, co))
    for kh in range(k):
        for kw in range(k):
            y += xp[:, kh:kh + stride * (Ho - 1) + 1:stride, kw:kw + stride * (Wo - 1) + 1:stride] @ w[:, kh, kw].T
    return y


def block_float64(fb, x_bhwc):
    """The folded block in float64 on its float32 weights: relu(conv_last(...) + bias + shortcut), plain sums."""
    y = np.asarray(x_bhwc, np.float64)
    for c in list(fb.convs)[:-1]:
        y = np.maximum(_conv64(y, _ohwi(_np(c.conv.weight)), c.conv.stride[0], c.conv.padding[0]) + _np(c.bias).astype(np.float64), 0)
    c = fb.convs[-1]
    y = _conv64(y, _ohwi(_np(c.conv.weight)), c.conv.stride[0], c.conv.padding[0]) + _np(c.bias).astype(np.float64)
    d = fb.downsample
    y += np.asarray(x_bhwc, np.float64) if d is None else _conv64(x_bhwc, _ohwi(_np(d.conv.weight)), d.conv.stride[0], 0)
    return np.maximum(y, 0)


def stem_float64(stem, x_bhwc):
    c = stem.cba
    y = np.maximum(_conv64(x_bhwc, _ohwi(_np(c.conv.weight)), 2, 3) + _np(c.bias).astype(np.float64), 0)
    B, H, W, C = y.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    yp = np.pad(y, ((0, 0), (1, 1), (1, 1), (0, 0)), constant_values=-np.inf)
    return np.max([yp[:, kh:kh + 2 * (Ho - 1) + 1:2, kw:kw + 2 * (Wo - 1) + 1:2] for kh in range(3) for kw in range(3)], axis=0)


def trunk_float64(trunk, x_bhwc):
    stem, blks = trunk_modules(trunk)
    y = stem_float64(stem, x_bhwc)
    for b in blks:
        y = block_float64(b, y)
    return y


def oracle_error(reference, r64):
    """E of the tolerance form: the oracle composition's own distance from the float64 evaluation of the same folded weights."""
    return float(np.abs(reference.astype(np.float64) - r64).max())


def folded_resnet(name, seed):
    """Folded `features` of an isx.backbones ResNet with randomised BatchNorms (on the CPU)."""
    from isx import backbones
    from model.nn_utils import extract_layers, fold_batch_norm
    net = randomise_bn(getattr(backbones, name)(pretrained=True).eval(), seed)
    return fold_batch_norm(extract_layers(net)[0])
