"""Model of the training engine of the trunk suffix (isx/suffix.py, SuffixEngine): what forward() and backward() must compute on a list of
Bottleneck blocks with eval-mode BatchNorm, written as ONE composition of functions that are already pinned -- the oracle's convolutions
(tests/test_gpu_trunk_guards.py, tests/test_gpu_trunk_modules.py) and tests/_suffix_model.py's restatements of the backward kernels
(tests/test_gpu_suffix_chains.py).  What is modelled here is the Python layer between them: which activation masks which input gradient, what
the dgrad of conv1 adds, the weight layouts, [W3' | Wd'] and b3' + bd', the rows the projection's weight gradient reads, the per-leaf rows and
accumulate = 1.  tests/test_suffix_engine_model.py holds the model to float64 autograd on the UNFOLDED blocks and shows that every mistake of
WRONGS moves a bit; tests/test_gpu_suffix_engine.py holds the engine to the model bit for bit.

numpy and the oracle only; torch only builds the blocks and hands their parameters over.  The model never reads a _Folded.

The fold of one convolution + BatchNorm: scale = fl(gamma * istd), bias = fl(beta - fl(mean * scale)), wf = fl(w * scale) -- single rounded
products and one rounded difference.  istd = 1 / sqrt(var + eps) is an INPUT: the device's rsqrt need not be correctly rounded, so the GPU test
hands in the engine's own and bounds its distance from float64 separately; the CPU test hands in the float32 rounding of the float64 value."""
import collections
import functools
import zlib

import numpy as np

import oracle as O
import _suffix_model as SM
from _trunk_model import randomise_bn

F = np.float32

WRONGS = {
    "mask_t1_for_t2": "conv3's input gradient masked with t1's pattern where the shapes allow, else not masked",
    "no_add": "the input gradient of conv1 without the shortcut's gradient",
    "add_unscattered_phase": "the projection's input gradient placed at the odd pixels of the zero map",
    "no_tap_flip": "w_dgrad of a stride-1 3x3 convolution without the flipped taps",
    "w_col_tap_major_swapped": "w_col of a stride-2 3x3 convolution with kh and kw exchanged",
    "proj_wgrad_reads_t2_rows": "the projection's weight gradient reads x without its stride: the rows of t2's grid",
    "ggamma_without_mean": "ggamma = <d, w> * istd: the mean * db term lost",
    "scale_for_istd": "scale handed to the chain rule of the fold where istd belongs",
    "db_dropped_from_gbeta": "the bias gradient never reaches gbeta",
    "accumulate_overwrites": "a second backward writes over .grad instead of adding to it",
    "leaves_share_one_sum": "the weight gradient summed over all leaves, every leaf given the total",
    "leaf_rows_swapped": "leaf l's gradients written to the row of leaf l + 1 (mod leaves)",
    "top_relu_grad_omitted": "no backward of the last block's output ReLU",
    "w_cat_swapped": "[Wd' | W3'] against the operand [t2 ; x]",
}
# moves istd by eps / (2 (var + eps)) relative: 3.3e-6 .. 1e-5 at eps = 1e-5 and variances in [0.5, 1.5] -- below the 1e-5 of the whole-step test
WRONGS_TOL = {"eps_dropped": "istd = 1 / sqrt(var): eps lost"}

# id -> blocks (inplanes, planes, stride, projection), input (B, H, W), leaves.  Planes 64 or 128: every channel count a multiple of 64.
CASES = {
    "id_id": dict(blocks=((256, 64, 1, False), (256, 64, 1, False)), shape=(2, 5, 7), leaves=1),          # add = dS; 35 pixels per image
    "p1_id": dict(blocks=((128, 64, 1, True), (256, 64, 1, False)), shape=(2, 5, 7), leaves=1),           # projection wgrad in the bottom block
    "id_p1": dict(blocks=((256, 64, 1, False), (256, 64, 1, True)), shape=(2, 5, 7), leaves=1),           # the dd path at stride 1
    "id_p2": dict(blocks=((256, 64, 1, False), (256, 128, 2, True)), shape=(2, 7, 9), leaves=1),          # col2im and scatter on an odd map
    "p2_alone": dict(blocks=((128, 64, 2, True),), shape=(3, 2, 2), leaves=1),                            # 1 x 1 output map
    "id_p2_leaves": dict(blocks=((256, 64, 1, False), (256, 128, 2, True)), shape=(6, 7, 9), leaves=3),
    "id_id_leaves": dict(blocks=((256, 64, 1, False), (256, 64, 1, False)), shape=(4, 5, 7), leaves=2),   # 70 pixels per leaf: a k-tile over the boundary
}

# one convolution + BatchNorm as numpy: w (Cout, Cin, kh, kw) and the four vectors
Conv = collections.namedtuple("Conv", "w gamma beta mean var eps stride taps")
Folded = collections.namedtuple("Folded", "istd scale bias wf w_fwd w_dgrad w_col")


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def make_blocks(cid):
    """The unfolded blocks of a case: seeded kaiming-normal weights, randomised BatchNorm statistics (the default ones have mean 0 and hide every
    mean term), eval mode, on the CPU."""
    import torch
    import torch.nn as nn
    from isx import backbones
    blocks = []
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(_seed(cid, "weights"))
        for cin, planes, stride, proj in CASES[cid]["blocks"]:
            down = None
            if proj:
                down = nn.Sequential(nn.Conv2d(cin, planes * 4, 1, stride=stride, bias=False), nn.BatchNorm2d(planes * 4))
            blocks.append(backbones.Bottleneck(cin, planes, stride, down))
        seq = nn.Sequential(*blocks)
        for m in seq.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
    return list(randomise_bn(seq, _seed(cid, "bn")).eval())


def case_inputs(cid):
    """(x, r): the input relu(N(0, 1)) and the weights r of the loss sum(y * r), both BHWC float32."""
    case = CASES[cid]
    B, H, W = case["shape"]
    rng = np.random.default_rng(_seed(cid, "x"))
    x = np.maximum(rng.standard_normal((B, H, W, case["blocks"][0][0]), dtype=F), 0)
    for _, planes, stride, _ in case["blocks"]:
        H, W, C = (H - 1) // stride + 1, (W - 1) // stride + 1, 4 * planes
    return x, rng.standard_normal((B, H, W, C), dtype=F)


def _np(t, dtype=F):
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(dtype))


def block_params(blocks):
    """Per block (conv1, conv2, conv3, projection or None) as Conv tuples."""
    def one(conv, bn):
        return Conv(_np(conv.weight), _np(bn.weight), _np(bn.bias), _np(bn.running_mean), _np(bn.running_var), float(bn.eps), conv.stride[0],
                    conv.kernel_size[0] * conv.kernel_size[1])
    return [(one(b.conv1, b.bn1), one(b.conv2, b.bn2), one(b.conv3, b.bn3), one(b.downsample[0], b.downsample[1]) if b.downsample is not None else None)
            for b in blocks]


def istd64(conv, eps_dropped=False):
    return 1.0 / np.sqrt(conv.var.astype(np.float64) + (0.0 if eps_dropped else conv.eps))


def istd32(params, eps_dropped=False):
    """Per block, per convolution: fl32 of the float64 1 / sqrt(var + eps)."""
    return [tuple(None if c is None else istd64(c, eps_dropped).astype(F) for c in blk) for blk in params]


# ---- the fold and its layouts ---------------------------------------------------------------------------------------------------------------
def fold(c, istd, wrong=None):
    scale = c.gamma * istd
    bias = c.beta - c.mean * scale
    wf = c.w * scale[:, None, None, None]                                            # (Cout, Cin, kh, kw)
    w_fwd = np.ascontiguousarray(wf.transpose(0, 2, 3, 1))                           # OHWI
    w_dgrad = w_col = None
    if c.taps == 1:
        w_dgrad = np.ascontiguousarray(wf.reshape(wf.shape[0], wf.shape[1]).T)       # (Cin, Cout)
    elif c.stride == 2:
        t = wf.transpose(0, 3, 2, 1) if wrong == "w_col_tap_major_swapped" else wf.transpose(0, 2, 3, 1)
        w_col = np.ascontiguousarray(t.reshape(wf.shape[0], -1).T)                   # (9 Cin, Cout), rows (kh, kw, ci)
    else:
        t = wf if wrong == "no_tap_flip" else wf[:, :, ::-1, ::-1]
        w_dgrad = np.ascontiguousarray(t.transpose(1, 2, 3, 0))                      # (Cin, kh, kw, Cout), taps flipped
    assert scale.dtype == F and bias.dtype == F and wf.dtype == F
    return Folded(istd, scale, bias, wf, w_fwd, w_dgrad, w_col)


def fold_cat(f3, fd, wrong=None):
    """([W3' | Wd'], fl(b3' + bd')) of the fused last convolution + projection."""
    w3, wd = f3.wf.reshape(f3.wf.shape[0], -1), fd.wf.reshape(fd.wf.shape[0], -1)
    return np.ascontiguousarray(np.concatenate([wd, w3] if wrong == "w_cat_swapped" else [w3, wd], 1)), f3.bias + fd.bias


def fold_all(params, istds, wrong=None):
    return [tuple(None if c is None else fold(c, i, wrong) for c, i in zip(blk, ist)) for blk, ist in zip(params, istds)]


# ---- isx_conv_wgrad_splits ------------------------------------------------------------------------------------------------------------------
def wgrad_splits(K, Cin, Cout, taps):
    """wgrad_splits of csrc/backward.hip as host arithmetic: the number of pixel splits for K pixels of ONE leaf."""
    nk = (K + 31) // 32
    if Cout % 128 == 0 and Cin % 128 == 0 and nk >= 8:
        n128 = (Cout // 128) * (Cin // 128) * taps
        best, best_t = 1, 1e300
        s = 1
        while s <= 8 and nk // s >= 4:
            rounds = (n128 * 8 * s + 767) // 768
            t = float(rounds) * (float(nk) / s + 6.0)
            if t < best_t:
                best_t, best = t, s
            s += 1
        return best
    big = Cout % 128 == 0 and Cin % 128 == 0 and (Cout // 128) * (Cin // 128) * taps >= 512
    tiles = ((Cout // 128) * (Cin // 128) if big else (Cout // 64) * (Cin // 64)) * taps
    s = min((512 + tiles - 1) // tiles, nk // 4, 16)
    return max(s, 1)


def conv_shapes(cid):
    """(pixels of one leaf, Cin, Cout, taps) of every weight-gradient launch of a case."""
    case = CASES[cid]
    B, H, W = case["shape"]
    per = B // case["leaves"]
    out = []
    for cin, planes, stride, proj in case["blocks"]:
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        out += [(per * H * W, cin, planes, 1), (per * Ho * Wo, planes, planes, 9), (per * Ho * Wo, planes, 4 * planes, 1)]
        if proj:
            out.append((per * Ho * Wo, cin, 4 * planes, 1))
        H, W = Ho, Wo
    return out


# ---- forward --------------------------------------------------------------------------------------------------------------------------------
def forward(params, folds, x, wrong=None):
    """[(x, t1, t2, y)] per block, BHWC float32: what SuffixEngine.forward keeps in `saved`; the output is the last y."""
    x = np.ascontiguousarray(x, F)
    saved = []
    for (c1, c2, c3, cd), (f1, f2, f3, fd) in zip(params, folds):
        B, H, W, C = x.shape
        t1 = O.conv1x1_nhwc(x.reshape(-1, C), f1.w_fwd.reshape(f1.w_fwd.shape[0], -1), f1.bias, None, True).reshape(B, H, W, -1)
        t2 = O.conv3x3_nhwc(t1, f2.w_fwd, f2.bias, c2.stride, None, True)
        if cd is None:
            y = O.conv1x1_nhwc(t2.reshape(-1, t2.shape[3]), f3.w_fwd.reshape(f3.w_fwd.shape[0], -1), f3.bias, x.reshape(-1, C), True)
            y = y.reshape(t2.shape[:3] + (-1,))
        else:
            w_cat, bias_cat = fold_cat(f3, fd, wrong)
            y = O.conv1x1_dual_nhwc(t2, x, w_cat, bias_cat, cd.stride, True)
        saved.append((x, t1, t2, y))
        x = y
    return saved


# ---- backward -------------------------------------------------------------------------------------------------------------------------------
def _flat(a):
    return np.ascontiguousarray(a.reshape(-1, a.shape[-1]))


def _param_grads(dz, x, geom, c, f, leaves, prior, wrong, src_stride=None):
    """wgrad_partials -> fold_backward of one convolution: (gw (leaves, Cout, Cin, kh, kw), ggamma, gbeta (leaves, Cout))."""
    Ho, Wo = SM.out_hw(geom)
    Cout, Cin = c.w.shape[:2]
    if wrong == "leaves_share_one_sum":
        dwp, db = SM.wgrad_partials(dz, x, geom, 1, wgrad_splits(geom.B * Ho * Wo, Cin, Cout, c.taps))
        dwp, db = np.repeat(dwp, leaves, 0), np.repeat(db, leaves, 0)
    else:
        S = wgrad_splits(geom.B // leaves * Ho * Wo, Cin, Cout, c.taps)
        if src_stride is None:
            dwp, db = SM.wgrad_partials(dz, x, geom, leaves, S)
        else:                                          # the rows of x the launch reads, for another stride than the projection's own
            K = geom.B // leaves * Ho * Wo
            ranges = SM.split_ranges(K, S)[1]
            dwp, db = SM.wgrad_from(dz, x, [np.arange(geom.B * Ho * Wo, dtype=np.int64)], range(leaves), S,
                                    lambda l, s: np.arange(l * K + ranges[s][0], l * K + ranges[s][1]))
    w = np.ascontiguousarray(c.w.reshape(Cout, Cin, c.taps))
    mean = np.zeros_like(c.mean) if wrong == "ggamma_without_mean" else c.mean
    istd = f.scale if wrong == "scale_for_istd" else f.istd
    if wrong == "db_dropped_from_gbeta":
        gw, gg, _ = SM.fold_backward(dwp, db, w, f.scale, mean, istd, c.taps, None)
        gb = np.zeros_like(gg)
        if prior is not None:
            gw, gg, gb = prior[0].reshape(gw.shape) + gw, prior[1] + gg, prior[2] + gb
    else:
        if prior is not None and wrong != "accumulate_overwrites":
            prior = (prior[0].reshape((leaves, Cout, Cin, c.taps)), prior[1], prior[2])
        else:
            prior = None
        gw, gg, gb = SM.fold_backward(dwp, db, w, f.scale, mean, istd, c.taps, prior)
    if wrong == "leaf_rows_swapped":
        gw, gg, gb = (np.roll(g, 1, 0) for g in (gw, gg, gb))
    return [gw.reshape((leaves,) + c.w.shape), gg, gb]


def backward(params, folds, saved, dy, leaves=1, prior=None, wrong=None):
    """SuffixEngine.backward, line for line.  dy: BHWC.  Returns the flat list of the engine's parameter order -- per block conv1, conv2, conv3,
    projection, each (weight, bn.weight, bn.bias) -- every array with a leading axis of `leaves`.  prior: such a list (leaves = 1) that the
    gradients are added to: accumulate = 1 onto an existing .grad."""
    assert prior is None or leaves == 1
    dy = np.ascontiguousarray(dy, F)
    at = [0]
    for blk in params:
        at.append(at[-1] + 3 * sum(c is not None for c in blk))

    def pri(bi, k):
        return None if prior is None else prior[at[bi] + 3 * k:at[bi] + 3 * k + 3]

    grads = [None] * len(params)
    dS = None
    for bi in range(len(params) - 1, -1, -1):
        (c1, c2, c3, cd), (f1, f2, f3, fd) = params[bi], folds[bi]
        x, t1, t2, y = saved[bi]
        B, H, W, _ = x.shape
        Ho, Wo = t2.shape[1:3]
        if dS is None:
            dS = dy if wrong == "top_relu_grad_omitted" else SM.relu_grad(dy, y)
        dS2 = _flat(dS)
        g3 = _param_grads(dS2, _flat(t2), SM.Geom(B, Ho, Wo, 1, 1), c3, f3, leaves, pri(bi, 2), wrong)
        gd = []
        if cd is not None:
            unstrided = wrong == "proj_wgrad_reads_t2_rows" and cd.stride != 1
            gd = _param_grads(dS2, _flat(x), SM.Geom(B, H, W, 1, cd.stride), cd, fd, leaves, pri(bi, 3), wrong, src_stride=1 if unstrided else None)
        mask = t2
        if wrong == "mask_t1_for_t2":
            mask = t1 if t1.shape == t2.shape else None
        dT2 = SM.dgrad1x1(dS2, f3.w_dgrad, None, None if mask is None else _flat(mask))
        g2 = _param_grads(dT2, _flat(t1), SM.Geom(B, H, W, 9, c2.stride), c2, f2, leaves, pri(bi, 1), wrong)
        if c2.stride == 2:
            dcol = SM.dgrad1x1(dT2, f2.w_col)
            dT1 = SM.col2im_s2(dcol.reshape(-1, 9, c2.w.shape[1]), B, H, W, c2.w.shape[1], t1)
        else:
            dT1 = SM.dgrad3x3(dT2.reshape(B, H, W, -1), f2.w_dgrad, t1)
        g1 = _param_grads(_flat(dT1), _flat(x), SM.Geom(B, H, W, 1, 1), c1, f1, leaves, pri(bi, 0), wrong)
        grads[bi] = g1 + g2 + g3 + gd
        if bi == 0:
            break
        if cd is None:
            add = dS2
        else:
            dd = SM.dgrad1x1(dS2, fd.w_dgrad).reshape(B, Ho, Wo, -1)
            add = np.zeros(x.shape, F)
            s = cd.stride
            if wrong == "add_unscattered_phase" and s != 1:
                nh, nw = len(range(1, H, s)), len(range(1, W, s))
                add[:, 1::s, 1::s] = dd[:, :nh, :nw]
            else:
                add[:, ::s, ::s] = dd
            add = _flat(add)
        if wrong == "no_add":
            add = None
        dS = SM.dgrad1x1(_flat(dT1), f1.w_dgrad, add, _flat(x)).reshape(x.shape)
    return [g for blk in grads for g in blk]


# ---- whole cases, computed once and shared read-only ----------------------------------------------------------------------------------------
def _frozen(arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False
    return arrays


def run(params, istds, x, r, leaves=1, prior=None, wrong=None):
    """(saved, grads) of the loss sum(y * r) on the given istd."""
    folds = fold_all(params, istds, wrong)
    saved = forward(params, folds, x, wrong)
    return saved, backward(params, folds, saved, r, leaves, prior, wrong)


@functools.lru_cache(maxsize=None)
def case_params(cid):
    return block_params(make_blocks(cid))


@functools.lru_cache(maxsize=None)
def case_cpu(cid, wrong=None):
    """(saved, grads) of a case on the CPU test's istd (fl32 of float64)."""
    params = case_params(cid)
    x, r = case_inputs(cid)
    saved, grads = run(params, istd32(params), x, r, CASES[cid]["leaves"], None, wrong)
    for s in saved:
        _frozen(s)
    return saved, _frozen(grads)
