"""The net side of the training step's contract (model/siamese.TrunkHooks: TuneClassif, TuneClassifSub, DescriptorNet) and the two isx.ops
wrappers the tail engines share (colsum_leaves, head_linear_dgrad).  On the CPU every hook declines; on the GPU precompute_trunk is, per
input, bit for bit what _SplitTrunk.prefix gives for that input alone, and the wrappers are bit for bit the direct C-ABI calls on operands
the test builds itself."""
import pytest
import torch

NETS = ("TuneClassif", "TuneClassifSub", "DescriptorNet")


def _net(kind, arch="resnet18"):
    """`kind` on a seeded ResNet with layer4 trainable, in training mode with BatchNorm frozen (what train_gen sets up)."""
    from isx import backbones
    from model import siamese
    from model.nn_utils import set_net_train
    from train.params import UNTRAINED_BLOCKS
    torch.manual_seed(0)
    base, untrained = backbones.MODELS[arch](pretrained=True, seed=0), UNTRAINED_BLOCKS[arch]
    if kind == "TuneClassif":
        net = siamese.TuneClassif(base, 5, untrained=untrained)
    elif kind == "TuneClassifSub":
        net = siamese.TuneClassifSub(base, 5, (2, 2), untrained=untrained)
    else:
        net = siamese.DescriptorNet(siamese.TuneClassif(base, 5, untrained=untrained), 32, (2, 2), untrained=untrained)
    set_net_train(net, True, bn_train=False)
    return net


@pytest.mark.parametrize("kind", NETS)
def test_hooks_decline_on_the_cpu(kind):
    import copy
    from model.siamese import TrunkHooks, _SplitTrunk
    net = _net(kind)
    assert isinstance(net, TrunkHooks) and net.training and net.branches_are_scales == (kind == "TuneClassifSub")
    assert net.trunk_precomputable() is False
    assert net.suffix_engine() is None and net.head_engine() is None and net.classif_head_engine() is None
    x = torch.randn(2, 3, 64, 64)
    assert net.precompute_trunk(x) is None and net.precompute_trunk(x, cache=True) is None and net.precompute_trunk() is None
    # the split trunk: one spelling, on a fresh net, outside the state dict, copied with the net
    net._trunk.folded = None
    assert isinstance(net._trunk, _SplitTrunk) and not any("_trunk" in k for k in net.state_dict())
    twin = copy.deepcopy(net)
    assert isinstance(twin._trunk, _SplitTrunk) and twin._trunk is not net._trunk


@pytest.fixture(scope="module")
def images():
    g = torch.Generator(device="cuda").manual_seed(3)
    return {s: [torch.randn(4, 3, s, s, device="cuda", generator=g) for _ in range(3)] for s in (64, 96)}


def _recorded_prefix(net):
    """net._trunk.prefix, recording the feature tensor of every call."""
    made, prefix = [], net._trunk.prefix

    def recording(features, x):
        f, split = prefix(features, x)
        made.append(f)
        return f, split
    net._trunk.prefix = recording
    return made


def _bits_differ(a, b):
    """0.0 when a and b hold the same bits, else max |a - b| / max |b| (printed before the assertion: the figure of a failure)."""
    if a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)):
        return 0.0
    return max(float((a - b).abs().max()) / float(b.abs().max()), 1e-45)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", NETS)
@pytest.mark.parametrize("arch", ("resnet18", "resnet50"))
def test_precompute_trunk_is_the_prefix_of_each_input(arch, kind, images, monkeypatch):
    """Layer4 trainable, 4 images of 64 x 64 per input (TuneClassifSub: scales 64 and 96).  What precompute_trunk returns is, per input, bit
    for bit _SplitTrunk.prefix of that input alone.

    The comparison runs with torch.backends.cudnn.deterministic set.  ResNet-18's two strided 1x1 shortcuts (64 -> 128 and 128 -> 256,
    stride 2) run on MIOpen (model/nn_utils.TORCH_CONV_CALLS names them), and with torch's default algorithm choice five launches
    of `prefix` on the SAME 4 images gave five different results on an MI355X (max |run 1 - run 0| / max |run 0| = 3.5e-7 at 64 x 64, 4.9e-7
    at 224 x 224; the first module whose output differs between two calls on one input is the first block with such a shortcut): the
    reference would not equal itself.  With the flag set the same five launches agree in every bit, and so do the rows of a 12-image
    launch with the 4-image launches, at 64 and at 96 pixels.  resnet50 (every prefix convolution in libisx: same bits for every launch and
    batch size with or without the flag) runs the same cases."""
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    net = _net(kind, arch).cuda()
    assert net.trunk_precomputable()
    a, b, c = images[64]
    big = images[96][0]
    if kind == "TuneClassifSub":
        xs = (a, big)                                           # two scales of 4 images
        assert net.precompute_trunk(a, big[:3]) is None         # unequal batch sizes
    elif kind == "DescriptorNet":
        xs = (a, b, c)
        assert net.precompute_trunk(a, b, big) is None          # a second shape
    else:
        xs = (a,)
    alone = [net._trunk.prefix(net.features, x)[0] for x in xs]
    made = _recorded_prefix(net)
    got = net.precompute_trunk(*xs)
    assert isinstance(got, tuple) and len(got) == len(xs) and [f.shape for f in got] == [f.shape for f in alone]
    assert len(made) == (len(xs) if kind == "TuneClassifSub" else 1)     # one launch per scale / one launch on the stacked branches
    # one input: the tensor prefix produced, not a copy of it (and no torch.cat of the images in front)
    del made[:]
    (one,) = net.precompute_trunk(a)
    assert len(made) == 1 and one is made[0]
    figures = [_bits_differ(f, want) for f, want in zip(got, alone)] + [_bits_differ(one, alone[0])]
    print("%s %s: precompute_trunk vs prefix of each input alone, max |diff| / max |ref| per input (0 = same bits): %s" % (arch, kind, figures))
    assert figures == [0.0] * len(figures)


def _direct():
    from isx._lib import check, lib
    return lib(), check, torch.cuda.current_stream().cuda_stream


@pytest.mark.gpu
@pytest.mark.parametrize("N", (64, 17))
@pytest.mark.parametrize("M", (1, 64, 65))
def test_head_linear_dgrad_wrapper_is_the_direct_call(M, N):
    """K = 64; N = 64: no class padding (M = 64: the no-copy operand, M = 65: the first size with row padding); N = 17: against a weight
    padded to 64 rows, the class rows beyond 17 zero.  The reference is the tail engines' former inline code: pad, transpose, call."""
    from isx import ops
    L, check, st = _direct()
    K, Np = 64, 64
    g = torch.Generator(device="cuda").manual_seed(100 * M + N)
    dy = torch.randn(M, N, device="cuda", generator=g)
    w = torch.zeros(Np, K, device="cuda")
    w[:N] = torch.randn(N, K, device="cuda", generator=g)
    Mp = (M + 63) // 64 * 64
    dyT = dy.new_zeros((Np, Mp))
    dyT[:N, :M] = dy.t()
    want = torch.full((Mp, K), float("nan"), device="cuda")
    check(L.isx_head_linear_dgrad(dyT.data_ptr(), Mp, Np, w.data_ptr(), K, want.data_ptr(), st), "isx_head_linear_dgrad")
    got = ops.head_linear_dgrad(dy, w)
    assert got.shape == (M, K) and torch.equal(got.view(torch.int32), want[:M].view(torch.int32))
    # and it is the product: N fp32 multiply-adds per element, in any order, err at most N 2^-23 sum |dy| |w|
    err = (got.double() - dy.double() @ w[:N].double()).abs()
    assert bool((err <= N * 2.0 ** -23 * (dy.abs().double() @ w[:N].abs().double())).all())


@pytest.mark.gpu
def test_colsum_leaves_wrapper_is_the_direct_call():
    from isx import ops
    L, check, st = _direct()
    leaves, R, C = 3, 5, 70
    x = torch.randn(leaves * R, C, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    want = torch.full((leaves, C), float("nan"), device="cuda")
    check(L.isx_colsum_leaves(x.data_ptr(), leaves, R, C, want.data_ptr(), st), "isx_colsum_leaves")
    got = ops.colsum_leaves(x, leaves)
    assert got.shape == (leaves, C) and torch.equal(got.view(torch.int32), want.view(torch.int32))
    # and they are the sums: R fp32 additions per element, err at most R 2^-23 sum |x|
    err = (got.double() - x.double().view(leaves, R, C).sum(1)).abs()
    assert bool((err <= R * 2.0 ** -23 * x.abs().double().view(leaves, R, C).sum(1)).all())
