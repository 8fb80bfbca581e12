"""CPU side of the folded-trunk model (tests/_trunk_model.py): the folds have the routes of the case table, the model sits within a DERIVED
forward error bound of a float64 evaluation of the UNFOLDED block, every wiring mistake of WRONGS moves at least one bit of it on every case
it can apply to, the merged bias has the bits of fl32(b3 + bd), and torch's fold sits within its rounding count of the float64 formulas.
The GPU side, which holds the modules to the model bit for bit, is tests/test_gpu_trunk_modules.py."""
import copy
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _trunk_model as TM

U = 2.0 ** -24                                  # unit roundoff of float32


def gamma(n):
    """Higham's gamma_n: n roundings compound to a relative error of at most n u / (1 - n u)."""
    return n * U / (1 - n * U)


@functools.lru_cache(maxsize=None)
def _case(cid):
    blk = TM.make_block(cid)
    return blk, TM.fold(blk)


@functools.lru_cache(maxsize=None)
def _right(cid, i):
    x, imgs = _inputs(cid)[i]
    return TM.block_reference(_case(cid)[1], x)


@functools.lru_cache(maxsize=None)
def _inputs(cid):
    # the images that the GPU test compares: the others of a large batch never reach the oracle
    return [(x if imgs is None else np.ascontiguousarray(x[list(imgs)]), imgs) for x, imgs in TM.case_inputs(cid)]


@pytest.mark.parametrize("cid", sorted(TM.CASES))
def test_fold_has_the_route_and_kinds_of_the_table(cid):
    case, (blk, fb) = TM.CASES[cid], _case(cid)
    assert fb.route == case["route"]
    assert tuple(c.kind for c in fb.convs) == case["kinds"]
    assert (fb.downsample.kind if fb.downsample is not None else None) == case["proj_kind"]
    assert all(c.relu for c in fb.convs)
    # randomise_bn: every folded bias vector is non-zero -- the seeded default trunk folds to biases of exactly 0.0, where no bias wiring shows
    for c in fb.convs:
        assert np.count_nonzero(TM._np(c.bias)) == c.bias.numel()
    if fb.downsample is not None:
        b3, bd = TM.unmerged_biases(blk)
        assert np.count_nonzero(bd) == bd.size and np.count_nonzero(b3) == b3.size
        assert not TM._np(fb.downsample.bias).any()                          # the projection keeps none of its own
    # some folded scales are negative
    assert any((getattr(blk, n).weight < 0).any() for n in ("bn1", "bn2"))


@pytest.mark.parametrize("cid", [c for c in sorted(TM.CASES) if TM.CASES[c]["block"][4]])
def test_merged_bias_has_the_bits_of_one_float32_add(cid):
    blk, fb = _case(cid)
    b3, bd = TM.unmerged_biases(blk)
    want = (b3 + bd).astype(np.float32)
    assert b3.dtype == np.float32 and bd.dtype == np.float32
    assert np.array_equal(TM._np(fb.convs[-1].bias).view(np.int32), want.view(np.int32))
    assert not np.array_equal(want, b3) and not np.array_equal(want, bd)


@torch.no_grad()
def _exact_fold(conv, bn):
    """float64 (w * gamma / sqrt(var + eps), beta - mean * gamma / sqrt(var + eps), |mean * scale| + |beta|) of one convolution + BatchNorm."""
    scale = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    w = conv.weight.double() * scale.view(-1, 1, 1, 1)
    shift = bn.running_mean.double() * scale
    return w, bn.bias.double() - shift, shift.abs() + bn.bias.double().abs()


# Roundings of torch's fuse_conv_bn_weights, all in float32:
#   weight  conv_w * (bn_w * rsqrt(bn_rv + eps)): the add (its relative error d enters the root as d / 2), rsqrt (a correctly rounded square root
#           and a correctly rounded division: 2), bn_w * (.) (1), conv_w * (.) (1): 4.5 u, bounded by gamma_5
#   bias    (0 - bn_rm) exact, * rsqrt (2.5 from above + 1), * bn_w (1): 4.5 u on the product s = mean * scale, then s + bn_b (1) on the sum:
#           |b' - b| <= gamma_5 |s| + u (|s| (1 + gamma_5) + |bn_b|) <= gamma_6 (|s| + |bn_b|)
FOLD_W, FOLD_B = 5, 6


@pytest.mark.parametrize("cid,conv,bn", [("expand128", "conv2", "bn2"), ("expand128", "conv3", "bn3")])
def test_fold_arithmetic_against_float64(cid, conv, bn):
    from torch.nn.utils.fusion import fuse_conv_bn_eval
    blk, _ = _case(cid)
    c, n = getattr(blk, conv), getattr(blk, bn)
    fused = fuse_conv_bn_eval(copy.deepcopy(c).eval(), copy.deepcopy(n).eval())
    w, b, bmag = _exact_fold(c, n)
    fused.requires_grad_(False)
    assert fused.weight.dtype == torch.float32 and fused.weight.shape[-1] == (3 if conv == "conv2" else 1)
    assert bool(((fused.weight.double() - w).abs() <= gamma(FOLD_W) * w.abs()).all())
    assert bool(((fused.bias.double() - b).abs() <= gamma(FOLD_B) * bmag).all())
    # and the bound is no formality: the fold is not exact
    assert float((fused.weight.double() - w).abs().max()) > 0


def _layer_bound(x, ex, w, b, eb, stride, pad, res=None, er=None, extra=None):
    """One convolution of the model against exact arithmetic.  x, ex: the exact input (float64, NCHW) and the bound on the model's input error;
    w, b: the exact folded weight and bias; eb: the bound on the stored bias; res, er: the exact residual and the bound on the model's;
    extra = (x2, w2, stride2): a second operand summed in the same two-level sum (the projection of the dual GEMM; its input is exact).
    Returns (exact pre-activation, bound on the model's).

    The model's value is sum_i x^_i w^_i (1 + theta_i) + b^ (1 + theta') + r^ (1 + delta) with w^_i = w_i (1 + phi_i), |phi_i| <= gamma_5 (the
    fold).  A product term passes at most 64 fmas of its chunk (oracle: ISXO_CONV_CHUNK), one add per chunk of the reduction (padding taps
    count as terms), the bias add and the residual add: |theta_i| <= gamma_n, n = 64 + ceil(K / 64) + 2.  The bias passes two adds, the
    residual one.  With x^ = x + ex:
        |err| <= gamma_{n+5} sum |x_i| |w_i| + (1 + gamma_{n+5}) sum ex_i |w_i| + (1 + gamma_2) eb + gamma_2 |b| + (1 + u) er + u |r|
    Underflow is left out: operands of order 1e-5 .. 1e2, no product near 2^-126.  ReLU is 1-Lipschitz: the bound passes it unchanged."""
    K = w[0].numel() + (extra[1][0].numel() if extra is not None else 0)
    g = gamma(64 + math.ceil(K / 64) + 2 + FOLD_W)
    conv = lambda a, ww, s, p: F.conv2d(a, ww, None, s, p)
    a = conv(x, w, stride, pad) + b.view(1, -1, 1, 1)
    mag = conv(x.abs(), w.abs(), stride, pad)
    if extra is not None:
        x2, w2, s2 = extra
        a = a + conv(x2, w2, s2, 0)
        mag = mag + conv(x2.abs(), w2.abs(), s2, 0)
    e = g * mag + (1 + g) * conv(ex, w.abs(), stride, pad) + ((1 + gamma(2)) * eb + gamma(2) * b.abs()).view(1, -1, 1, 1)
    if res is not None:
        a = a + res
        e = e + (1 + U) * er + U * res.abs()
    return a, e


@pytest.mark.parametrize("cid", TM.EXACT)
def test_model_within_derived_bound_of_float64_unfolded_block(cid):
    """|model - float64(unfolded block)| <= the running forward bound of _layer_bound, element by element: no measured constant in it."""
    blk, fb = _case(cid)
    names = (("conv1", "bn1"), ("conv2", "bn2"), ("conv3", "bn3"))[:len(fb.convs)]
    folds = [_exact_fold(getattr(blk, c), getattr(blk, n)) for c, n in names]
    ref64 = copy.deepcopy(blk).double().eval()
    for i, (xn, _) in enumerate(_inputs(cid)):
        x = torch.from_numpy(xn).permute(0, 3, 1, 2).double()
        a, e = x, torch.zeros_like(x)
        for (w, b, bmag), (c, _) in zip(folds[:-1], names):
            conv = getattr(blk, c)
            a, e = _layer_bound(a, e, w, b, gamma(FOLD_B) * bmag, conv.stride, conv.padding)
            a = torch.relu(a)
        w, b, bmag = folds[-1]
        conv, eb = getattr(blk, names[-1][0]), gamma(FOLD_B) * bmag
        if blk.downsample is None:
            a, e = _layer_bound(a, e, w, b, eb, conv.stride, conv.padding, res=x, er=torch.zeros_like(x))
        else:
            wd, bd, bdmag = _exact_fold(blk.downsample[0], blk.downsample[1])
            # merged bias fl32(b3^ + bd^): both errors and one more rounding of the sum
            ebd = gamma(FOLD_B) * bdmag
            eb = eb + ebd + U * (b.abs() + bd.abs() + eb + ebd)
            a, e = _layer_bound(a, e, w, b + bd, eb, conv.stride, conv.padding, extra=(x, wd, blk.downsample[0].stride))
        exact = torch.relu(a)
        with torch.no_grad():
            want = ref64(x)
        # the layered float64 pass above IS the unfolded block (float64 rounding only)
        assert float((exact - want).abs().max()) <= 1e-12 * float(want.abs().max())
        got = torch.from_numpy(_right(cid, i)).permute(0, 3, 1, 2).double()
        err = (got - want).abs()
        assert bool((err <= e + 1e-12).all()), (cid, i, float((err - e).max()))
        assert float(err.max()) > 0
        if blk.downsample is not None:
            # the bound separates: a lost projection bias lies outside it
            bad = TM.block_reference(fb, xn, wrong="proj_bias_dropped", unmerged=TM.unmerged_biases(blk))
            assert not bool(((torch.from_numpy(bad).permute(0, 3, 1, 2).double() - want).abs() <= e + 1e-12).all())


@pytest.mark.parametrize("cid", sorted(TM.CASES))
def test_every_applicable_wrong_moves_a_bit(cid):
    """Non-vacuity: on every input of the case, each wiring mistake that can apply to the block gives an output that differs from the model's
    in at least one bit.  The ones that cannot apply are listed by name in the case table; nothing else is left out."""
    case, (blk, fb) = TM.CASES[cid], _case(cid)
    assert set(case["not_applicable"]) <= set(TM.WRONGS)
    applicable = sorted(set(TM.WRONGS) - set(case["not_applicable"]))
    kind, cin, planes, stride, proj = case["block"]
    cout = planes * (4 if kind == "bottleneck" else 1)
    # the structurally inapplicable ones, and no more
    structural = set()
    if not proj:
        structural |= {"proj_bias_dropped", "proj_bias_twice", "residual_is_input", "proj_offset", "w_cat_swapped"}
    if proj and (stride != 1 or cin != cout):
        structural.add("residual_is_input")
    if proj and stride == 1:
        structural.add("proj_offset")
    if kind == "basic":
        structural.add("w_cat_swapped")
    if kind == "basic" or stride == 1:
        structural.add("stride_in_conv1")
    assert set(case["not_applicable"]) == structural
    unmerged = TM.unmerged_biases(blk) if proj else None
    for i, (x, _) in enumerate(_inputs(cid)):
        right = _right(cid, i)
        for wrong in applicable:
            got = TM.block_reference(fb, x, wrong=wrong, unmerged=unmerged)
            assert got.shape == right.shape and got.dtype == np.float32, (wrong, i)
            assert not np.array_equal(got.view(np.int32), right.view(np.int32)), (cid, wrong, i)


@pytest.mark.parametrize("cid", ["expand_dual", "dual_s2", "dual_same"])
def test_unfused_projection_is_another_sum(cid):
    """A projection Bottleneck whose `route` is None adds the projection as a residual: a sum of its own, rounded on its own.  The model has
    both forms; they agree to rounding and not in bits, so the GPU test compares each route with its own form."""
    _, fb = _case(cid)
    x = _inputs(cid)[0][0]
    fused, unfused = _right(cid, 0), TM.block_reference(fb, x, unfused=True)
    assert not np.array_equal(fused, unfused)
    r = TM.block_float64(fb, x)
    assert TM.oracle_error(unfused, r) <= 4 * TM.oracle_error(fused, r) and TM.oracle_error(fused, r) <= 4 * TM.oracle_error(unfused, r)


def test_float64_arbiters_against_torch():
    """block_float64 / stem_float64 (numpy) against torch's CPU convolutions in double on the same folded weights."""
    for cid in ("dual_s2", "basic_s2", "mixed"):
        _, fb = _case(cid)
        x = _inputs(cid)[0][0]
        with torch.no_grad():
            want = copy.deepcopy(fb).double()(torch.from_numpy(x).permute(0, 3, 1, 2).double()).permute(0, 2, 3, 1).numpy()
        assert np.abs(TM.block_float64(fb, x) - want).max() <= 1e-12 * np.abs(want).max()
    stem = _stem()
    x = np.random.default_rng(5).standard_normal((2, 17, 12, 3), dtype=np.float32)
    with torch.no_grad():
        want = copy.deepcopy(stem).double()(torch.from_numpy(x).permute(0, 3, 1, 2).double()).permute(0, 2, 3, 1).numpy()
    assert np.abs(TM.stem_float64(stem, x) - want).max() <= 1e-12 * np.abs(want).max()
    # and the one-kernel stem's sum is that function to float32 rounding
    assert TM.oracle_error(TM.stem_reference(stem, x), want) <= 1e-5 * np.abs(want).max()


@functools.lru_cache(maxsize=None)
def _stem():
    from isx import backbones
    from model.nn_utils import fold_batch_norm
    import torch.nn as nn
    net = TM.randomise_bn(backbones.resnet18(pretrained=True).eval(), 11)
    return fold_batch_norm(nn.Sequential(net.conv1, net.bn1, net.relu, net.maxpool))[1]


def test_trunk_reference_chains_the_blocks():
    """trunk_reference over a folded ResNet-18 `features` is stem_reference, then block_reference block by block; every folded bias of the
    randomised trunk is non-zero (the default initialisation folds to 0.0 everywhere)."""
    trunk = TM.folded_resnet("resnet18", 3)
    stem, blocks = TM.trunk_modules(trunk)
    assert len(blocks) == 8
    assert all(v.abs().min() > 0 for k, v in trunk.state_dict().items() if k.endswith("bias") and "downsample" not in k)
    x = np.random.default_rng(9).standard_normal((1, 32, 40, 3), dtype=np.float32)
    y = TM.stem_reference(stem, x)
    assert np.array_equal(TM.trunk_reference(trunk, x, blocks=0), y)
    for b in blocks[:3]:
        y = TM.block_reference(b, y)
    assert np.array_equal(TM.trunk_reference(trunk, x, blocks=3), y)
    full = TM.trunk_reference(trunk, x)
    assert full.shape == (1, 1, 2, 512)
    r = TM.trunk_float64(trunk, x)
    assert TM.oracle_error(full, r) <= 1e-4 * np.abs(r).max()
