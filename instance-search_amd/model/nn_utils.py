"""Backbone surgery helpers -- same names and behaviour as the reference's
model/nn_utils.py (extract_layers :56-71, convolutionalize :26-39, get_feature_size :42-53,
set_untrained_blocks :6-23, set_net_train :160-163), written against isx.backbones instead
of torchvision.  The BN copy/replace helpers (:74-134) are training-time surgery and are
out of scope."""
import os

import torch
import torch.nn as nn

from isx import backbones as models
from isx import ops


def set_untrained_blocks(containers, n):
    """n < 0 freezes everything; otherwise the first n parameterised modules (counted across
    the containers in order) are frozen and the rest left trainable."""
    params_of = lambda m: list(m.parameters())
    for seq in containers:
        for m in seq:
            for p in params_of(m):
                p.requires_grad = n >= 0
    frozen = 0
    for seq in containers:
        for m in seq:
            if frozen >= n:
                break
            ps = params_of(m)
            if not ps:
                continue            # parameter-free modules do not count
            for p in ps:
                p.requires_grad = False
            frozen += 1


def convolutionalize(fc, in_size2d):
    """Linear(C*h*w -> out) as Conv2d(C -> out, kernel (h, w)): weight rows are viewed
    (C, h, w), i.e. channel-major then h then w."""
    kh, kw = in_size2d
    if fc.in_features % (kh * kw) != 0:
        raise ValueError('FC in_feature size {0} is not divisible by in_size2d {1}'.format(fc.in_features, in_size2d))
    cin = fc.in_features // (kh * kw)
    conv = nn.Conv2d(cin, fc.out_features, (kh, kw), bias=fc.bias is not None)
    with torch.no_grad():
        conv.weight.copy_(fc.weight.reshape(fc.out_features, cin, kh, kw))
        if fc.bias is not None:
            conv.bias.copy_(fc.bias)
    return conv.to(fc.weight.device)


def get_feature_size(seq, factor=1, default=-1):
    """Output width of the last conv-like / linear module of `seq` (conv widths times `factor`)."""
    size = default
    for m in seq:
        if isinstance(m, models.Bottleneck):
            size = m.conv3.out_channels * factor
        elif isinstance(m, models.BasicBlock):
            size = m.conv2.out_channels * factor
        elif isinstance(m, nn.Conv2d):
            size = m.out_channels * factor
        elif isinstance(m, nn.Linear):
            size = m.out_features
    return size


def extract_layers(net):
    """(features, feature_reduc, classifier) of a backbone."""
    if all(hasattr(net, a) for a in ('features', 'feature_reduc', 'classifier')):
        return net.features, net.feature_reduc, net.classifier
    if isinstance(net, models.ResNet):
        stem = [net.conv1, net.bn1, net.relu, net.maxpool]
        blocks = [b for layer in (net.layer1, net.layer2, net.layer3, net.layer4) for b in layer]
        return nn.Sequential(*(stem + blocks)), nn.Sequential(net.avgpool), nn.Sequential(net.fc)
    return net.features, nn.Sequential(), net.classifier


# ISX_ALEX: the convolutions without a BatchNorm behind them and the MaxPool2d(3, 2) of an AlexNet-style `features` (isx.backbones.alexnet,
# model.ModelDefinition.Maxnet).  "1": every one of them runs on libisxalex (isx/alex.py: general K x K convolution with the trunk's canonical sum,
# un-padded 3 / 2 max-pool) or, the 3x3 / padding 1 layers with Cin % 32 == 0, on libisx's isx_conv3x3_nhwc -- no torch convolution or pool on
# the GPU, descriptors that do not depend on the batch.  "0": the modules as they were (MIOpen, torch ReLU, torch max_pool2d), bit for bit.  "auto"
# (default): per layer kind, native where tools/alex_lab.py measured it no slower than MIOpen's route by more than that route's own spread
# (_ALEX_AUTO_KINDS; DESIGN 4, "AlexNet trunk").  Read at fold time and at every forward.  Measured at B = 256, 224 x 224 (ms per layer kind, HIP route
# against MIOpen's with its min-max spread): 11x11 / 4 0.513 : 0.573 (0.091), 5x5 1.022 : 0.978 (0.111) -- 4 % behind, inside the spread, and ahead
# again with the pool behind it --, the three 13x13 3x3 layers 1.486 : 1.670 (0.149), the three pools 0.141 : 0.235 (0.160); extraction 84.2 k : 75.6 k
# images/s.  Every kind is taken.  A kernel size outside these (conv1, conv7, ...) has not been measured and goes native under "1" only.
_ALEX_MODE = os.environ.get("ISX_ALEX", "auto")
_ALEX_AUTO_KINDS = frozenset(("conv11", "conv5", "conv3", "pool"))

# Convolutions that ran on torch's conv2d (MIOpen) on a GPU tensor in this process, as {(kernel, stride, Cin, Cout): calls}: the ResNet
# trunks leave it empty (every layer is a libisx kernel), and so does an AlexNet-style trunk under ISX_ALEX=1; the AlexNet layer kinds that
# ISX_ALEX=auto leaves with MIOpen (see _ALEX_AUTO_KINDS), a 3x3 with Cin % 32 != 0 behind a BatchNorm, grouped / dilated convolutions and
# stand-alone strided 1x1 layers land here ("what still runs on MIOpen").  Under ISX_ALEX=0 the AlexNet layers are plain torch
# modules again and are not counted.
TORCH_CONV_CALLS = {}


def _note_torch_conv(c):
    key = (tuple(c.kernel_size), tuple(c.stride), c.in_channels, c.out_channels)
    TORCH_CONV_CALLS[key] = TORCH_CONV_CALLS.get(key, 0) + 1


def _derived(owner, slot, sources, build):
    """A tensor derived from weights (`sources`), cached on `owner` under `slot` and rebuilt when a source was written in place
    (load_state_dict copies into the parameters: the version counter moves), replaced, or moved to another device.  Writes through
    `.data` bypass the version counter: call `invalidate_derived_weights(module)` after such surgery."""
    key = tuple((t.data_ptr(), t._version, str(t.device)) for t in sources)
    hit = owner.__dict__.get(slot)
    if hit is None or hit[0] != key:
        with torch.no_grad():
            hit = (key, build())
        owner.__dict__[slot] = hit
    return hit[1]


def invalidate_derived_weights(module):
    """Drop every cached re-layout of a weight (OHWI copies, concatenated / transposed projection weights) under `module`."""
    for m in module.modules():
        for slot in ('_c_w_ohwi', '_c_w_cat', '_c_w3t', '_hwc', '_c_pad64'):
            if slot in m.__dict__:
                m.__dict__[slot] = None


def _native(x):
    """The ONE per-input test of the folded ResNet trunk: what the libisx convolution kernels take -- an fp32 GPU tensor without an autograd
    graph whose memory is channels-last.  A tensor that is dense in both formats (H = W = 1, or C = 1) counts as NCHW: the torch route."""
    return x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled() and ops._is_nhwc(x)


def _as_nhwc(t):
    if t is None or t.is_contiguous(memory_format=torch.channels_last):
        return t
    return t.contiguous(memory_format=torch.channels_last)


def _is_3x3(c, strides, cin_multiple):
    return (c.kernel_size == (3, 3) and c.padding == (1, 1) and c.groups == 1 and c.dilation == (1, 1) and c.stride in strides
            and c.in_channels % cin_multiple == 0)


def _is_1x1(c, strides):
    return c.kernel_size == (1, 1) and c.padding == (0, 0) and c.groups == 1 and c.stride in strides


class _ConvBiasAct(nn.Module):
    """Bias-free convolution + fused `y = act(y + bias (+ residual))` epilogue.  `kind`, fixed here from the convolution's geometry, names
    what runs it on a `_native` input: "conv3x3" (isx_conv3x3_nhwc: implicit GEMM on the fp32 matrix cores), "conv1x1" (isx_conv1x1_nhwc: one
    fp32-MFMA GEMM over the pixels), both with the epilogue fused, or "torch" (torch's convolution, then libisx `isx_bias_act_inplace` on the
    GPU, plain torch otherwise) -- which is also what every other input gets.  `in_block`: a convolution of a BN-folded residual block
    (_FusedBlock).  The 3x3 kernel takes every one of those (1.93-1.98 ms against MIOpen's igemm + zero fill + separate epilogue pass
    2.05-2.15 ms at Cin >= 256, B = 1024; ResNet-50 extraction +2-3 % at B = 256 and at 448x448), a stand-alone layer behind a BatchNorm
    only up to Cin = 128.  (Layers without a BatchNorm, the AlexNet ones, are ISX_ALEX's, above.)
    `plain`: no epilogue of its own on the torch route and a zero bias (projection shortcut: its bias is merged into the block's last)."""

    def __init__(self, conv, relu, in_block=False, plain=False):
        super().__init__()
        bias = conv.bias.detach().clone() if conv.bias is not None else torch.zeros(conv.out_channels)
        self.conv = nn.Conv2d(conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding, conv.dilation,
                              conv.groups, bias=False)
        self.conv.weight = nn.Parameter(conv.weight.detach().clone(), requires_grad=False)
        self.bias = nn.Parameter(torch.zeros_like(bias) if plain else bias, requires_grad=False)
        self.relu = relu
        self.in_block = in_block
        self.plain = plain
        c = self.conv
        if _is_3x3(c, ((1, 1), (2, 2)), 32) and (in_block or c.in_channels <= 128):
            self.kind = "conv3x3"
        elif _is_1x1(c, ((1, 1),)) and c.dilation == (1, 1):
            self.kind = "conv1x1"
        else:
            self.kind = "torch"

    def w_ohwi(self):
        """(Cout,kh,kw,Cin) copy of the weight for the implicit-GEMM / stem kernels; follows the weight (see _derived)."""
        w = self.conv.weight
        return _derived(self, '_c_w_ohwi', (w,), lambda: w.detach().permute(0, 2, 3, 1).contiguous())

    def forward(self, x, residual=None):
        if self.kind != "torch" and _native(x):
            if self.kind == "conv3x3":
                return ops.conv3x3_nhwc(x, self.w_ohwi(), self.bias, self.conv.stride[0], _as_nhwc(residual), self.relu)
            return ops.conv1x1_nhwc(x, self.conv.weight, self.bias, _as_nhwc(residual), self.relu)
        y = self.conv(x)
        if y.is_cuda:
            _note_torch_conv(self.conv)
        if self.plain:
            return y
        if y.is_cuda and y.dtype == torch.float32 and not torch.is_grad_enabled():
            if residual is not None and residual.stride() != y.stride():
                residual = residual.contiguous(memory_format=torch.channels_last if not y.is_contiguous() else torch.contiguous_format)
            return ops.bias_act_(y, self.bias, residual, self.relu)
        if not torch.is_grad_enabled():
            # CPU inference (the parity side of the GPU tests, CPU-only users): the epilogue in place on the convolution's own output -- the same
            # fp32 adds in the same order, without three more passes' worth of fresh 100 MB tensors per layer
            y.add_(self.bias.view(1, -1, 1, 1).to(y.dtype))
            if residual is not None:
                y.add_(residual)
            return y.relu_() if self.relu else y
        y = y + self.bias.view(1, -1, 1, 1).to(y.dtype)
        if residual is not None:
            y = y + residual
        return torch.relu(y) if self.relu else y


class _StemConvPool(nn.Module):
    """conv + folded BN + ReLU + MaxPool2d(3, 2, 1) of the ResNet stem: the bias / ReLU epilogue and the pooling run
    as ONE pass over the convolution output (libisx `isx_bias_relu_maxpool_nhwc`) on channels-last GPU tensors."""

    def __init__(self, conv, pool):
        super().__init__()
        self.cba = _ConvBiasAct(conv, relu=True)
        self.pool = pool

    def forward(self, x):
        c = self.cba
        if (x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled() and c.conv.out_channels % 4 == 0):
            if ops.stem7x7_pool_applicable(x, c.conv):
                # images up to 896 wide: convolution + bias + ReLU + pooling as ONE kernel, nothing in between touches memory
                return ops.stem7x7_pool(x, c.w_ohwi(), c.bias)
            y = c.conv(x)
            _note_torch_conv(c.conv)
            if y.is_contiguous(memory_format=torch.channels_last) and not y.is_contiguous():
                return ops.bias_relu_maxpool(y, c.bias)
            return self.pool(ops.bias_act_(y, c.bias, None, c.relu))
        return self.pool(c(x))


def _is_stem_pool(m):
    return (isinstance(m, nn.MaxPool2d) and m.kernel_size in (3, (3, 3)) and m.stride in (2, (2, 2)) and m.padding in (1, (1, 1))
            and m.dilation in (1, (1, 1)) and not m.ceil_mode)


class _FusedBlock(nn.Module):
    """Inference form of a (BN-folded) BasicBlock / Bottleneck: relu(convN(...) + bias + identity) with every
    bias / residual / ReLU fused into one in-place pass per convolution.  The projection shortcut keeps no
    epilogue of its own: its bias is added to the last convolution's bias.

    `route`, fixed here from the folded convolutions, names the fused kernel that runs the block's tail on a `_native` input:
      "dual"         relu(conv_last(t) + projection(x) + bias) as ONE GEMM over [t ; x_strided] (isx_conv1x1_dual_nhwc): the shortcut tensor
                     is never materialised
      "expand_dual"  first block of the 64-channel stage: conv2 + conv3 + projection + ReLU as ONE kernel (isx_conv3x3_expand_dual_nhwc)
      "expand64"     identity Bottleneck with 64 mid channels (ResNet stage 1): conv2 + conv3 + residual + ReLU as ONE kernel
                     (isx_conv3x3_expand_nhwc): the mid activation never reaches memory
      "expand128"    identity Bottleneck with 128 mid channels (ResNet stage 2, blocks 1..): the same as ONE kernel
                     (isx_conv3x3_expand128_nhwc): the 128 x 128 accumulator tile of conv2 IS the A operand of conv3
      None           no fused tail: one call per convolution, which is also what every other input gets."""

    def __init__(self, convs, downsample):
        super().__init__()
        self.convs = nn.ModuleList([_ConvBiasAct(c, relu=True, in_block=True) for c in convs])
        self.downsample = None
        if downsample is not None:
            last = self.convs[-1]
            d_bias = downsample.bias.detach() if downsample.bias is not None else torch.zeros(downsample.out_channels)
            last.bias = nn.Parameter(last.bias + d_bias, requires_grad=False)
            self.downsample = _ConvBiasAct(downsample, relu=False, plain=True)      # projection (its bias lives in the last conv's epilogue)
        self.route = self._route()

    def _route(self):
        last, d = self.convs[-1], self.downsample
        c2 = self.convs[1].conv if len(self.convs) == 3 else None
        # conv2 of a Bottleneck as the fused expansion kernels take it: 3x3 / stride 1 with a ReLU behind it, conv3 a plain 1x1 GEMM
        mid = c2.out_channels if (c2 is not None and _is_3x3(c2, ((1, 1),), 32) and self.convs[1].relu and last.kind == "conv1x1"
                                  and last.conv.in_channels == c2.out_channels) else None
        if d is not None:
            if not (last.kind == "conv1x1" and _is_1x1(d.conv, ((1, 1), (2, 2))) and last.conv.in_channels % 32 == 0 and d.conv.in_channels % 32 == 0):
                return None
            if mid == 64 and last.conv.out_channels == 256 and d.conv.in_channels == 64 and d.conv.stride == (1, 1):
                return "expand_dual"
            return "dual"
        block_in, cout = self.convs[0].conv.in_channels, last.conv.out_channels
        if mid == 64 and cout == 256 and block_in == 256:
            return "expand64"
        if mid == 128 and c2.in_channels % 64 == 0 and cout % 128 == 0 and block_in == cout:
            return "expand128"
        return None

    def w_cat(self):
        """[W_last | W_projection] (Cout, K1 + K2) for the fused last-conv + shortcut GEMM; follows both weights (see _derived)."""
        wl, wd = self.convs[-1].conv.weight, self.downsample.conv.weight
        co = wl.shape[0]
        return _derived(self, '_c_w_cat', (wl, wd), lambda: torch.cat([wl.detach().reshape(co, -1), wd.detach().reshape(co, -1)], 1).contiguous())

    def w3t(self):
        """Transposed expansion weight of the fused conv2 + conv3 kernels: [W3 | Wd]^T with a projection shortcut, W3^T without."""
        wl = self.convs[-1].conv.weight
        if self.downsample is not None:
            wd = self.downsample.conv.weight
            return _derived(self, '_c_w3t', (wl, wd), lambda: self.w_cat().t().contiguous())
        return _derived(self, '_c_w3t', (wl,), lambda: wl.detach().reshape(wl.shape[0], -1).t().contiguous())

    def forward(self, x):
        if self.route is not None and _native(x):
            last = self.convs[-1]
            if self.route == "dual":
                t = x
                for c in self.convs[:-1]:
                    t = c(t)
                return ops.conv1x1_dual_nhwc(_as_nhwc(t), x, self.w_cat(), last.bias, self.downsample.conv.stride[0], last.relu)
            c2 = self.convs[1]
            t = _as_nhwc(self.convs[0](x))
            if self.route == "expand_dual":
                return ops.conv3x3_expand_dual_nhwc(t, c2.w_ohwi(), c2.bias, x, self.w3t(), last.bias, last.relu)
            if self.route == "expand64":
                return ops.conv3x3_expand_nhwc(t, c2.w_ohwi(), c2.bias, c2.conv.stride[0], self.w3t(), last.bias, x, last.relu)
            assert self.route == "expand128", self.route
            return ops.conv3x3_expand128_nhwc(t, c2.w_ohwi(), c2.bias, self.w3t(), last.bias, x, last.relu)
        idt = x if self.downsample is None else self.downsample(x)
        y = x
        for c in self.convs[:-1]:
            y = c(y)
        return self.convs[-1](y, idt)


def _alex_native(kind):
    return _ALEX_MODE == "1" or (_ALEX_MODE == "auto" and kind in _ALEX_AUTO_KINDS)


def _gpu_inference_nhwc(x):
    # not _native: a map that is dense in both memory formats (H = W = 1, or C = 1) counts as channels-last HERE and goes to the AlexNet
    # kernels; making the two one would change which library computes such a map
    return (x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled() and x.dim() == 4
            and x.is_contiguous(memory_format=torch.channels_last))


class _AlexConv(nn.Module):
    """A convolution with no BatchNorm behind it (+ the ReLU that follows) of an AlexNet-style trunk.  On channels-last GPU activations without
    an autograd graph, where ISX_ALEX takes its layer kind: ONE call with bias and ReLU fused -- isx.alex.conv2d_nhwc, or isx.ops.conv3x3_nhwc for a
    3x3 / padding 1 layer with Cin % 32 == 0 (the same sum: either library gives the same bits).  Everywhere else (CPU, training, ISX_ALEX kinds left
    with MIOpen) the two modules it was built from, called as the Sequential called them."""

    def __init__(self, conv, act):
        super().__init__()
        import copy
        self.conv = copy.deepcopy(conv)
        self.act = copy.deepcopy(act)                       # the nn.ReLU behind the convolution, or None
        k = conv.kernel_size[0]
        self.libisx_3x3 = (k == 3 and tuple(conv.padding) == (1, 1) and conv.stride[0] in (1, 2) and conv.in_channels % 32 == 0)
        self.kind = "conv%d" % k                             # the layer kinds of ISX_ALEX=auto: conv11, conv5, conv3 (and pool)
        if conv.bias is None:
            self.register_buffer("no_bias", torch.zeros(conv.out_channels), persistent=False)

    def w_ohwi(self):
        """(Cout,K,K,Cin) copy of the weight; follows the weight (see _derived)."""
        w = self.conv.weight
        return _derived(self, '_c_w_ohwi', (w,), lambda: w.detach().permute(0, 2, 3, 1).contiguous())

    def forward(self, x):
        c = self.conv
        if _alex_native(self.kind) and _gpu_inference_nhwc(x):
            bias = c.bias if c.bias is not None else self.no_bias
            if self.libisx_3x3:
                return ops.conv3x3_nhwc(x, self.w_ohwi(), bias, c.stride[0], None, self.act is not None)
            from isx import alex
            if x.data_ptr() % 16:
                # a view into a larger batch whose images are no multiple of 16 bytes (Cin = 3): the kernel wants its base pointer aligned
                x = x.clone(memory_format=torch.channels_last)
            return alex.conv2d_nhwc(x, self.w_ohwi(), bias, c.stride[0], c.padding[0], self.act is not None)
        y = c(x)
        if y.is_cuda:
            _note_torch_conv(c)
        return y if self.act is None else self.act(y)


class _AlexPool(nn.Module):
    """MaxPool2d(3, stride 2) without padding, dilation or ceil mode: isx.alex.maxpool3s2 (torch's bits) on channels-last GPU activations without an
    autograd graph where ISX_ALEX takes the pool, the module itself everywhere else."""
    kind = "pool"

    def __init__(self, pool):
        super().__init__()
        import copy
        self.pool = copy.deepcopy(pool)

    def forward(self, x):
        if _alex_native(self.kind) and _gpu_inference_nhwc(x):
            # "auto" picks a route per shape; under "1" a map the kernel does not take is an error (isx.alex raises), never a quiet torch pool
            if _ALEX_MODE == "1" or (x.shape[1] % 4 == 0 and x.shape[2] >= 3 and x.shape[3] >= 3):
                from isx import alex
                return alex.maxpool3s2(x)
        return self.pool(x)


def _is_alex_conv(m):
    from isx import alex
    return type(m) is nn.Conv2d and alex.conv2d_applicable(m)


def _is_alex_pool(m):
    return (type(m) is nn.MaxPool2d and m.kernel_size in (3, (3, 3)) and m.stride in (2, (2, 2)) and m.padding in (0, (0, 0))
            and m.dilation in (1, (1, 1)) and not m.ceil_mode and not m.return_indices)


def alex_route_active(features):
    """Does ISX_ALEX send a layer of this trunk to a HIP kernel?  What makes folding a trunk WITHOUT BatchNorm worth it
    (train._common.prepare_for_inference): under "0", and under "auto" while no kind is taken, such a trunk stays as it is."""
    if _ALEX_MODE == "0":
        return False
    return any((_is_alex_conv(m) and _alex_native("conv%d" % m.kernel_size[0])) or (_is_alex_pool(m) and _alex_native("pool")) for m in features)


class _ChannelsLastEntry(nn.Module):
    """First module of a folded trunk: a GPU fp32 image batch enters in channels-last memory, so that every activation
    behind it is the row-major (pixels, channels) matrix the hand-written convolution kernels (and MIOpen's NHWC kernels)
    consume.  Same values, another memory format; the 3-channel input is the only tensor ever converted."""

    def forward(self, x):
        if x.is_cuda and x.dim() == 4 and x.dtype == torch.float32 and not torch.is_grad_enabled():
            return x.contiguous(memory_format=torch.channels_last)
        return x


def fold_batch_norm(features, fuse_epilogues=True):
    """Inference-only copy of a `features` trunk with every eval-mode BatchNorm2d folded into the
    convolution in front of it (w' = w * gamma / sqrt(var + eps), b' = beta - mean * gamma / sqrt(var + eps)).
    Same function up to fp32 rounding (max relative deviation ~2e-6 on the ResNet-50 map).  With
    `fuse_epilogues` the bias-add / residual-add / ReLU after each convolution run as ONE in-place HIP kernel
    (`isx_bias_act_inplace`) instead of 4-7 separate passes over the activation.  Not part of the reference
    (its BN helpers, model/nn_utils.py:74-155, only copy / re-create / freeze BN layers)."""
    import copy
    from torch.nn.utils.fusion import fuse_conv_bn_eval

    def fold_block(b):
        convs = [fuse_conv_bn_eval(copy.deepcopy(getattr(b, c)).eval(), copy.deepcopy(getattr(b, n)).eval())
                 for c, n in (('conv1', 'bn1'), ('conv2', 'bn2'), ('conv3', 'bn3')) if hasattr(b, c)]
        down = None
        if b.downsample is not None:
            down = fuse_conv_bn_eval(copy.deepcopy(b.downsample[0]).eval(), copy.deepcopy(b.downsample[1]).eval())
        if fuse_epilogues:
            return _FusedBlock(convs, down)
        b = copy.deepcopy(b)
        for i, (c, n) in enumerate((('conv1', 'bn1'), ('conv2', 'bn2'), ('conv3', 'bn3'))):
            if hasattr(b, c):
                setattr(b, c, convs[i])
                setattr(b, n, nn.Identity())
        if down is not None:
            b.downsample = nn.Sequential(down)
        return b

    mods, out, i = list(features), [], 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.Conv2d) and i + 1 < len(mods) and isinstance(mods[i + 1], nn.BatchNorm2d):
            conv = fuse_conv_bn_eval(copy.deepcopy(m).eval(), copy.deepcopy(mods[i + 1]).eval())
            i += 2
            if fuse_epilogues and i + 1 < len(mods) and isinstance(mods[i], nn.ReLU) and _is_stem_pool(mods[i + 1]):
                out.append(_StemConvPool(conv, copy.deepcopy(mods[i + 1])))     # stem: epilogue + pooling in one pass
                i += 2
            elif fuse_epilogues and i < len(mods) and isinstance(mods[i], nn.ReLU):
                out.append(_ConvBiasAct(conv, relu=True))      # conv + BN + ReLU -> conv, one fused epilogue
                i += 1
            else:
                out.append(conv)
            continue
        if fuse_epilogues and _ALEX_MODE != "0" and _is_alex_conv(m):
            # AlexNet-style layer: convolution (+ ReLU) without a BatchNorm -> one module that ISX_ALEX routes to a HIP kernel with the epilogue fused
            act = mods[i + 1] if i + 1 < len(mods) and type(mods[i + 1]) is nn.ReLU else None
            out.append(_AlexConv(m, act))
            i += 1 if act is None else 2
            continue
        if fuse_epilogues and _ALEX_MODE != "0" and _is_alex_pool(m):
            out.append(_AlexPool(m))
            i += 1
            continue
        out.append(fold_block(m) if isinstance(m, (models.Bottleneck, models.BasicBlock)) else copy.deepcopy(m))
        i += 1
    if fuse_epilogues:
        out.insert(0, _ChannelsLastEntry())
    return nn.Sequential(*out).eval()


def set_batch_norm_train(seq, train):
    for m in seq.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.train(mode=train)


def set_net_train(net, train, bn_train=False):
    """train/eval switch; in train mode BatchNorm (only net.features has any) stays frozen
    unless bn_train."""
    net.train(mode=train)
    if train and not bn_train:
        set_batch_norm_train(net.features, False)
