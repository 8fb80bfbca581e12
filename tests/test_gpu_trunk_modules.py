"""The folded ResNet trunk (model/nn_utils.fold_batch_norm) module by module against tests/_trunk_model.py: on an input the libisx kernels
take, every _FusedBlock, the _StemConvPool and whole trunks equal ONE fixed composition of oracle calls on the module's own parameters, bit
for bit, with the launches of the case table and no convolution left to torch; every other input (NCHW, a non-dense view, autograd, a map that
is dense in both memory formats) and every block with a torch convolution agrees with a float64 evaluation of the folded weights within
MARGIN times the oracle composition's own error.  All BatchNorms are randomised (TM.randomise_bn): a default-initialised trunk folds to biases
of exactly 0.0.  The CPU side (routes, derived bound, non-vacuity of the model) is tests/test_trunk_model.py; the measured ratios of the
tolerance cases are in docs/rounds/r20.md."""
import copy
import functools

import numpy as np
import pytest
import torch

import _guards as G
import _trunk_model as TM
from test_gpu_trunk_routes import RESNET50, _recorded

pytestmark = pytest.mark.gpu

P, T, D, E64, E128 = TM.P, TM.T, TM.D, TM.E64, TM.E128
S = "isx_stem7x7_pool_nhwc"
# max|out - R| <= MARGIN * E: R the float64 evaluation of the folded weights, E = max|oracle composition - R| on the same input, computed on the
# CPU from the model alone.  Another order of a sum of the same length has an error of the same magnitude; 4 covers the spread between orders.
MARGIN = 4


def _gpu(x_bhwc):
    """BHWC numpy -> (B,C,H,W) GPU tensor in channels-last memory."""
    return torch.from_numpy(np.ascontiguousarray(x_bhwc)).cuda().permute(0, 3, 1, 2)


def _host(y):
    return y.detach().permute(0, 2, 3, 1).contiguous().cpu().numpy()


def _on_gpu(m):
    return copy.deepcopy(m).cuda().to(memory_format=torch.channels_last)


def _fwd(m, x):
    with torch.no_grad():
        return m(x)


def _pick(a, imgs):
    return a if imgs is None else np.ascontiguousarray(a[list(imgs)])


def _within(out, r64, e, what, margin=MARGIN):
    err = float(np.abs(out.astype(np.float64) - r64).max())
    print("TOLERANCE %-46s max|out - R| = %.3e  E = %.3e  ratio %.3f" % (what, err, e, err / e))
    assert out.shape == r64.shape, (what, out.shape, r64.shape)
    assert e > 0 and err <= margin * e, (what, err, e, err / e)


def _convs_of(fb):
    """{(kernel, stride, Cin, Cout): count} of every convolution of a folded block, as nn_utils.TORCH_CONV_CALLS names them."""
    out = {}
    for c in [m.conv for m in fb.convs] + ([fb.downsample.conv] if fb.downsample is not None else []):
        key = (tuple(c.kernel_size), tuple(c.stride), c.in_channels, c.out_channels)
        out[key] = out.get(key, 0) + 1
    return out


@functools.lru_cache(maxsize=None)
def _case(cid):
    fb = TM.fold(TM.make_block(cid))
    return fb, _on_gpu(fb)


@functools.lru_cache(maxsize=None)
def _inputs(cid, dense=False):
    return TM.case_inputs(cid, dense)


@functools.lru_cache(maxsize=None)
def _ref(cid, i, unfused=False):
    x, imgs = _inputs(cid)[i]
    return TM.block_reference(_case(cid)[0], _pick(x, imgs), unfused=unfused)


@functools.lru_cache(maxsize=None)
def _r64(cid, i, dense=False):
    x, imgs = _inputs(cid, dense)[i]
    return TM.block_float64(_case(cid)[0], _pick(x, imgs))


EXACT_INPUTS = [(cid, i) for cid in TM.EXACT for i in range(len(TM.CASES[cid]["shapes"]) + 1)]


@pytest.mark.parametrize("cid,i", EXACT_INPUTS, ids=["%s-%d" % ci for ci in EXACT_INPUTS])
def test_block_equals_the_model(cid, i):
    """A native input: the model's bits, the launches of the table, nothing left to torch; the same bits from the first image alone; and the
    block with `route = None`: the same bits where there is no projection, the model's `unfused` form where there is one."""
    case, (fb, blk) = TM.CASES[cid], _case(cid)
    x, imgs = _inputs(cid)[i]
    xg = _gpu(x)
    from model.nn_utils import _native
    with torch.no_grad():
        assert _native(xg)
    out, names, torch_convs = _recorded(lambda: _fwd(blk, xg))
    assert names == case["launches"] and torch_convs == {}
    G.assert_bits(_pick(_host(out), imgs), _ref(cid, i), "%s input %d" % (cid, i))
    # batch independence: the first image alone
    one, names1, _ = _recorded(lambda: _fwd(blk, xg[:1]))
    assert names1 == case["launches"]
    assert torch.equal(one, out[:1])
    # the unfused route
    plain = copy.deepcopy(blk)
    plain.route = None
    out2, names2, torch_convs2 = _recorded(lambda: _fwd(plain, xg))
    body = [T, T] if len(fb.convs) == 2 else [P, T, P]
    if fb.downsample is None:
        assert names2 == body and torch_convs2 == {}
        assert torch.equal(out2, out)
    elif fb.downsample.kind == "conv1x1":
        # the projection is a GEMM of its own, ahead of the block's convolutions, and enters conv3 as its residual: another sum than the dual
        # GEMM's, the model's `unfused` form bit for bit
        assert names2 == [P] + body and torch_convs2 == {}
        G.assert_bits(_pick(_host(out2), imgs), _ref(cid, i, True), "%s input %d, route None" % (cid, i))
    else:
        d, c3 = fb.downsample.conv, fb.convs[-1].conv
        left = {((1, 1), tuple(d.stride), d.in_channels, d.out_channels): 1}
        if tuple(out.shape[2:]) == (1, 1):
            # without a route every _ConvBiasAct asks _native of ITS input: conv2's output is one pixel, dense in both formats, and conv3 is torch's
            body = body[:-1]
            left[((1, 1), (1, 1), c3.in_channels, c3.out_channels)] = 1
        assert names2 == body and torch_convs2 == left
        r = _r64(cid, i)
        _within(_pick(_host(out2), imgs), r, TM.oracle_error(_ref(cid, i, True), r), "%s input %d route None" % (cid, i))


@pytest.mark.parametrize("cid", TM.EXACT)
def test_block_on_inputs_the_kernels_do_not_take(cid):
    """nn_utils._native is the one per-input test.  Under autograd, and on an NCHW input of a block whose weights are NCHW, every convolution is
    torch's.  A non-dense channels-last view fails _native at the block's door: the convolutions that read x (conv1, the projection) are torch's;
    each later _ConvBiasAct asks _native of ITS input, the output of torch's convolution, so what follows depends on the memory format MIOpen
    returns -- every convolution is accounted for either way, and the output agrees within the tolerance form."""
    from model.nn_utils import _native
    fb, blk = _case(cid)
    x, _ = _inputs(cid)[0]
    xg = _gpu(x)
    r, e = _r64(cid, 0), TM.oracle_error(_ref(cid, 0), _r64(cid, 0))
    every = _convs_of(fb)
    # autograd
    with torch.enable_grad():
        assert not _native(xg)
        out, names, torch_convs = _recorded(lambda: blk(xg))
    assert names == [] and torch_convs == every
    _within(_host(out), r, e, "%s autograd" % cid)
    # NCHW input, NCHW weights
    nchw = copy.deepcopy(fb).cuda()
    xn = xg.contiguous()
    assert xn.is_contiguous() and not xn.is_contiguous(memory_format=torch.channels_last)
    out, names, torch_convs = _recorded(lambda: _fwd(nchw, xn))
    assert names == [] and torch_convs == every
    assert out.shape == (x.shape[0],) + _ref(cid, 0).shape[3:] + _ref(cid, 0).shape[1:3]
    _within(_host(out), r, e, "%s NCHW" % cid)
    # the first half of the channels of a channels-last tensor twice as deep
    big = torch.zeros(xg.shape[0], 2 * xg.shape[1], xg.shape[2], xg.shape[3], device="cuda").contiguous(memory_format=torch.channels_last)
    view = big[:, :xg.shape[1]]
    view.copy_(xg)
    assert not view.is_contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        assert not _native(view)
    out, names, torch_convs = _recorded(lambda: _fwd(blk, view))
    print("ROUTE %s non-dense view: launches %s, torch %s" % (cid, names, torch_convs))
    first = [fb.convs[0].conv] + ([fb.downsample.conv] if fb.downsample is not None else [])
    assert torch_convs == {(tuple(c.kernel_size), tuple(c.stride), c.in_channels, c.out_channels): 1 for c in first}
    # MIOpen answers a channels-last-strided input with a dense channels-last output, which the next convolutions take; never a fused tail
    # (those are the native ROUTE's)
    assert names == ([T] if len(fb.convs) == 2 else [T, P])
    _within(_host(out), r, e, "%s non-dense view" % cid)


def test_block_on_a_map_dense_in_both_formats():
    """expand64 on 1 x 256 x 1 x 1: contiguous in both memory formats, which counts as NCHW -- the torch route, within the tolerance form."""
    fb, blk = _case("expand64")
    (x, _), = _inputs("expand64", True)
    xg = _gpu(x)
    assert xg.is_contiguous() and xg.is_contiguous(memory_format=torch.channels_last)
    out, names, torch_convs = _recorded(lambda: _fwd(blk, xg))
    assert names == [] and torch_convs == _convs_of(fb)
    r = _r64("expand64", 0, True)
    _within(_host(out), r, TM.oracle_error(TM.block_reference(fb, x), r), "expand64 1x1x1 (dense in both formats)")


def test_block_whose_map_shrinks_to_one_pixel_stays_native():
    """dual_s2 on 2 x 2: conv2's output `t` and the block's output are 1 x 1, dense in both formats; the block's own test was of x, so all three
    launches are libisx's (pinned bit for bit by test_block_equals_the_model[dual_s2-1]) -- but the NEXT module's _native is false."""
    from model.nn_utils import _native
    _, blk = _case("dual_s2")
    x, _ = _inputs("dual_s2")[1]
    assert x.shape[1:3] == (2, 2)
    out = _fwd(blk, _gpu(x))
    assert out.shape == (2, 512, 1, 1)
    with torch.no_grad():
        assert not _native(out)


@pytest.mark.parametrize("cid", [c for c in TM.CASES if not TM.CASES[c]["exact"]])
def test_block_with_a_torch_convolution(cid):
    """basic_s2 (strided 1x1 projection) and mixed (3x3 with Cin = 48): one convolution is torch's, the others libisx's; E comes from the model
    with that convolution computed by the oracle's chain."""
    case, (fb, blk) = TM.CASES[cid], _case(cid)
    for i, (x, _) in enumerate(_inputs(cid)):
        out, names, torch_convs = _recorded(lambda: _fwd(blk, _gpu(x)))
        print("ROUTE %s input %d: launches %s, torch %s" % (cid, i, names, torch_convs))
        # basic_s2: the projection's output is only ever a residual.  mixed: conv3 asks _native of the output of torch's 3x3, which MIOpen
        # returns channels-last for a channels-last input
        assert names == case["launches"] and torch_convs == case["torch_convs"]
        r = _r64(cid, i)
        _within(_host(out), r, TM.oracle_error(_ref(cid, i), r), "%s input %d" % (cid, i))


# ---- the stem

@functools.lru_cache(maxsize=None)
def _stem():
    import torch.nn as nn
    from isx import backbones
    from model.nn_utils import fold_batch_norm
    net = TM.randomise_bn(backbones.resnet50(pretrained=True).eval(), 11)
    stem = fold_batch_norm(nn.Sequential(net.conv1, net.bn1, net.relu, net.maxpool))[1]
    assert np.count_nonzero(TM._np(stem.cba.bias)) == 64
    return stem, _on_gpu(stem)


def _image(B, H, W, seed):
    return np.random.default_rng(seed).standard_normal((B, H, W, 3), dtype=np.float32)


@pytest.mark.parametrize("B,H,W", [(2, 17, 12), (1, 9, 228)])
def test_stem_equals_the_model(B, H, W):
    stem, gstem = _stem()
    x = _image(B, H, W, H)
    out, names, torch_convs = _recorded(lambda: _fwd(gstem, _gpu(x)))
    assert names == [S] and torch_convs == {}
    G.assert_bits(_host(out), TM.stem_reference(stem, x), "stem %dx%dx%d" % (B, H, W))


def test_stem_on_a_later_image_of_a_batch():
    """x[1:] of a 2 x 3 x 5 x 12 channels-last batch.  With W % 4 == 0 an image is a multiple of 48 bytes, so every image of a dense batch starts
    on 16 bytes: this IS an input of the one-kernel stem, bit for bit.  (A base pointer off 16 bytes needs a buffer that is itself off: below.)"""
    stem, gstem = _stem()
    x = _image(2, 5, 12, 3)
    xg = _gpu(x)[1:]
    assert xg.data_ptr() % 16 == 0 and xg.data_ptr() != _gpu(x).data_ptr()
    out, names, torch_convs = _recorded(lambda: _fwd(gstem, xg))
    assert names == [S] and torch_convs == {}
    G.assert_bits(_host(out), TM.stem_reference(stem, x[1:]), "stem x[1:]")


def _counted(monkeypatch, names):
    from isx import ops
    calls = []
    for n in names:
        def wrap(*a, _f=getattr(ops, n), _n=n, **kw):
            calls.append(_n)
            return _f(*a, **kw)
        monkeypatch.setattr(ops, n, wrap)
    return calls


@pytest.mark.parametrize("what", ["W % 4 != 0", "W > STEM_MAX_W", "base pointer off 16 bytes"])
def test_stem_fallbacks(what, monkeypatch):
    """What the one-kernel stem does not take: the convolution is torch's, then bias + ReLU + pooling as one libisx pass
    (isx_bias_relu_maxpool_nhwc) where torch's output is channels-last, isx_bias_act_inplace and torch's pool where it is not."""
    from isx import ops
    stem, gstem = _stem()
    if what == "W % 4 != 0":
        x = _image(2, 17, 10, 1)
        xg = _gpu(x)
    elif what == "W > STEM_MAX_W":
        assert ops.STEM_MAX_W == 896
        x = _image(1, 8, 900, 2)
        xg = _gpu(x)
    else:
        x = _image(1, 5, 12, 4)
        buf = torch.empty(x.size + 1, device="cuda")
        buf[1:].copy_(torch.from_numpy(x).reshape(-1))
        xg = buf[1:].view(1, 5, 12, 3).permute(0, 3, 1, 2)
        assert xg.data_ptr() % 16 == 4 and xg.is_contiguous(memory_format=torch.channels_last)
    assert not ops.stem7x7_pool_applicable(xg, gstem.cba.conv)
    with torch.no_grad():
        nhwc_out = ops._is_nhwc(gstem.cba.conv(xg))
    calls = _counted(monkeypatch, ["stem7x7_pool", "bias_relu_maxpool", "bias_act_"])
    out, names, torch_convs = _recorded(lambda: _fwd(gstem, xg))
    print("ROUTE stem %s: torch's convolution returns %s, then %s" % (what, "channels-last" if nhwc_out else "NCHW", calls))
    assert names == [] and torch_convs == {((7, 7), (2, 2), 3, 64): 1}
    assert nhwc_out, "torch's convolution of a channels-last image with channels-last weights came back NCHW"
    assert calls == ["bias_relu_maxpool"]
    r = TM.stem_float64(stem, x)
    _within(_host(out), r, TM.oracle_error(TM.stem_reference(stem, x), r), "stem %s" % what)


# ---- whole trunks

@functools.lru_cache(maxsize=None)
def _trunk(name):
    t = TM.folded_resnet(name, 50 if name == "resnet50" else 18)
    assert all(v.abs().min() > 0 for k, v in t.state_dict().items() if k.endswith("bias") and "downsample" not in k)
    return t, _on_gpu(t)


@functools.lru_cache(maxsize=None)
def _trunk_input(B, H, W):
    return _image(B, H, W, 100 + H)


@functools.lru_cache(maxsize=None)
def _trunk_ref(name, shape, blocks=None):
    return TM.trunk_reference(_trunk(name)[0], _trunk_input(*shape), blocks)


@pytest.mark.parametrize("shape", [(1, 64, 64), (1, 40, 72)])
def test_resnet50_equals_the_model(shape):
    """(1, 40, 72): maps 10 x 18 -> 5 x 9 -> 3 x 5 -> 2 x 3, odd and non-square through every strided block."""
    _, trunk = _trunk("resnet50")
    out, names, torch_convs = _recorded(lambda: _fwd(trunk, _gpu(_trunk_input(*shape))))
    assert names == RESNET50 and torch_convs == {}
    want = _trunk_ref("resnet50", shape)
    if shape == (1, 40, 72):
        assert want.shape == (1, 2, 3, 2048)
    G.assert_bits(_host(out), want, "ResNet-50 %s" % (shape,))


def test_resnet50_flips_to_torch_behind_a_one_pixel_map():
    """2 x 3 x 32 x 32: 8 x 8 behind the stem, 4 x 4, 2 x 2, and 1 x 1 INSIDE the first block of stage 4 (its conv2 has the stride).  That block
    asked _native of its 2 x 2 input and runs its three launches; its output is dense in both formats, so _native turns false at the door of
    the second block of stage 4: the last two blocks, six convolutions, are torch's."""
    cpu, trunk = _trunk("resnet50")
    shape = (2, 32, 32)
    xg = _gpu(_trunk_input(*shape))
    out, names, torch_convs = _recorded(lambda: _fwd(trunk, xg))
    assert names == [S] + 3 * [P, E64] + [P, T, D] + 3 * [P, E128] + [P, T, D] + 5 * [P, T, P] + [P, T, D]        # = RESNET50 less 2 * [P, T, P]
    assert names == RESNET50[:-6]
    assert torch_convs == {((1, 1), (1, 1), 2048, 512): 2, ((3, 3), (1, 1), 512, 512): 2, ((1, 1), (1, 1), 512, 2048): 2}
    # the last native block's output, bit for bit
    head, names_head, torch_head = _recorded(lambda: _fwd(trunk[:-2], xg))
    assert names_head == RESNET50[:-6] and torch_head == {}
    assert head.shape == (2, 2048, 1, 1)
    G.assert_bits(_host(head), _trunk_ref("resnet50", shape, 14), "ResNet-50 at 32 x 32, first block of stage 4")
    r = TM.trunk_float64(cpu, _trunk_input(*shape))
    _within(_host(out), r, TM.oracle_error(_trunk_ref("resnet50", shape), r), "ResNet-50 2x32x32 (two torch blocks)")


def test_resnet18_block_by_block():
    """The blocks without a projection are bit for bit on the GPU output of their predecessor (so MIOpen's projections do not enter); the three
    with one, and the whole output, within the tolerance form."""
    cpu, trunk = _trunk("resnet18")
    shape = (1, 64, 64)
    x = _trunk_input(*shape)
    (stem, blocks), (gstem, gblocks) = TM.trunk_modules(cpu), TM.trunk_modules(trunk)
    y = _fwd(gstem, _gpu(x))
    G.assert_bits(_host(y), TM.stem_reference(stem, x), "ResNet-18 stem")
    exact = 0
    for k, (b, gb) in enumerate(zip(blocks, gblocks)):
        yin = _host(y)
        y, names, torch_convs = _recorded(lambda: _fwd(gb, y))
        assert names == [T, T]
        if b.downsample is None:
            assert torch_convs == {}
            G.assert_bits(_host(y), TM.block_reference(b, yin), "ResNet-18 block %d" % k)
            exact += 1
        else:
            assert sum(torch_convs.values()) == 1
            r = TM.block_float64(b, yin)
            _within(_host(y), r, TM.oracle_error(TM.block_reference(b, yin), r), "ResNet-18 block %d (torch projection)" % k)
    assert exact == 5
    out = _fwd(trunk, _gpu(x))
    again = _fwd(trunk, _gpu(x))
    # printed, not asserted: two forwards of this trunk on one input were seen to differ in their last bits (docs/rounds/r20.md); the blocks
    # without a projection are pinned bit for bit above, so what moves lies behind torch's strided projections
    print("NOTE ResNet-18: whole trunk == block by block: %s; whole trunk twice: %s; max|difference| %.3e"
          % (torch.equal(out, y), torch.equal(out, again), float((out - y).abs().max())))
    r = TM.trunk_float64(cpu, x)
    _within(_host(out), r, TM.oracle_error(_trunk_ref("resnet18", shape), r), "ResNet-18 1x64x64")
