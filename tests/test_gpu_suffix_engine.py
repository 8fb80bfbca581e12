"""The training engine of the trunk suffix (isx/suffix.py, SuffixEngine) held, BIT FOR BIT, to tests/_suffix_engine_model.py: the fold and its
layouts, every tensor the forward keeps, every parameter gradient -- through eng.backward, through autograd, with other memory layouts, onto an
existing .grad, leaf by leaf into flat rows -- and the caches behind the parameters' version counters.  The kernels themselves are pinned at the
C ABI (tests/test_gpu_suffix_chains.py, tests/test_gpu_trunk_guards.py); what is pinned here is the Python layer that decides what they are fed.
tests/test_suffix_engine_model.py shows on the CPU that the model is the operation and that each mistake of its WRONGS moves a bit of a gradient.
Every comparison is the project's _same (tests/test_gpu_suffix_chains.py: numpy's array_equal on the float32 values, so 'bit for bit' holds up
to the sign of a zero; the CPU file compares int32 views) unless it says otherwise.  The one number that is not the model's is
istd = rsqrt(var + eps): the model takes the engine's own, and the engine's is held to float64 under ISTD_BOUND.

The last test runs isx_conv3x3_dgrad_nhwc where its automatic choice takes the 128x128 tile (tests/test_suffix_engine_model.py:
test_dgrad3x3_tile_choice_restated)."""
import numpy as np
import pytest
import torch

import _suffix_engine_model as EM
import _suffix_model as SM
from test_gpu_suffix_chains import SENTINEL, _dev, _guarded, _guards_intact, _lib, _same

pytestmark = pytest.mark.gpu

# |f.istd - istd64| / istd64, istd64 = 1 / sqrt(double(var) + eps).  Measured on an MI355X over every convolution of every case: 6.526e-08 at
# most (docs/rounds/r21.md) -- one rounding of var + eps (it enters the root at half weight), the device's rsqrt and the rounding of the result.
# The bound in force is twice that figure; it must stay under 8 * 2^-24 = 4.8e-07, a factor 7 below what a dropped eps moves (3.3e-06).
ISTD_MEASURED = 6.526e-08
ISTD_BOUND = 2 * ISTD_MEASURED
assert ISTD_BOUND <= 8 * 2.0 ** -24

ONE_LEAF = [c for c in sorted(EM.CASES) if EM.CASES[c]["leaves"] == 1]
LEAVES = [c for c in sorted(EM.CASES) if EM.CASES[c]["leaves"] > 1]


def _nchw(a):
    """BHWC numpy -> (B, C, H, W) channels-last CUDA tensor."""
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda().permute(0, 3, 1, 2)


def _bhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().cpu().numpy()


def _engine(cid):
    from isx.suffix import SuffixEngine
    blocks = [b.cuda() for b in EM.make_blocks(cid)]
    assert SuffixEngine.applicable(blocks)
    return blocks, SuffixEngine(blocks)


def _folded(eng):
    return [list(convs) + [down] for convs, down in eng.layers]


def _istds(eng):
    return [tuple(None if f is None else f.istd.cpu().numpy() for f in blk) for blk in _folded(eng)]


_MODEL = {}


def _model(cid, eng):
    """(params, folds, saved, grads) of the case on the ENGINE's istd (after a forward), computed once per case."""
    istds = _istds(eng)
    if cid not in _MODEL:
        params = EM.case_params(cid)
        x, r = EM.case_inputs(cid)
        folds = EM.fold_all(params, istds)
        saved = EM.forward(params, folds, x)
        _MODEL[cid] = (istds, params, folds, saved, EM.backward(params, folds, saved, r, EM.CASES[cid]["leaves"]))
    assert all(a is b is None or np.array_equal(a, b) for s, t in zip(_MODEL[cid][0], istds) for a, b in zip(s, t))     # one rsqrt, one result
    return _MODEL[cid][1:]


def _setup(cid):
    blocks, eng = _engine(cid)
    x, r = EM.case_inputs(cid)
    xd, rd = _nchw(x), _nchw(r)
    y, saved = eng.forward(xd)
    return blocks, eng, xd, rd, y, saved


def _grads_equal(got, want, what, leaf=0):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g is not None, (what, i)
        _same(g.detach().contiguous(), w[leaf], (what, i))


@pytest.mark.parametrize("cid", sorted(EM.CASES))
def test_fold_and_forward(cid):
    """istd under its bound against float64 (printed); given it, scale, bias and w_fwd are single rounded products and one rounded difference,
    w_dgrad, w_col, [W3' | Wd'] and b3' + bd' the model's permutations and sum; the model's split rule is the library's for every convolution;
    every tensor of `saved` and the output are the model's."""
    blocks, eng, xd, rd, y, saved = _setup(cid)
    params, folds, want_saved, _ = _model(cid, eng)
    worst = 0.0
    for fb, pb, mb in zip(_folded(eng), params, folds):
        for f, c, m in zip(fb, pb, mb):
            assert (f is None) == (c is None)
            if f is None:
                continue
            i64 = EM.istd64(c)
            worst = max(worst, float(np.max(np.abs(f.istd.cpu().numpy().astype(np.float64) - i64) / i64)))
            for name in ("scale", "bias", "w_fwd", "w_dgrad", "w_col"):
                want = getattr(m, name)
                if want is None:
                    assert name in ("w_dgrad", "w_col") and getattr(f, name, None) is None
                else:
                    _same(getattr(f, name), want, (cid, name))
            assert f.mean.data_ptr() == f.bn.running_mean.data_ptr()
        if fb[3] is not None:
            w_cat, bias_cat = EM.fold_cat(mb[2], mb[3])
            _same(fb[3].w_cat, w_cat, (cid, "w_cat"))
            _same(fb[3].bias_cat, bias_cat, (cid, "bias_cat"))
    print("suffix engine %s: max |istd - istd64| / istd64 = %.3e (bound %.3e)" % (cid, worst, ISTD_BOUND))
    assert worst <= ISTD_BOUND
    L = _lib()[0]
    for K, Cin, Cout, taps in EM.conv_shapes(cid):
        assert L.isx_conv_wgrad_splits(K, Cin, Cout, taps) == EM.wgrad_splits(K, Cin, Cout, taps), (K, Cin, Cout, taps)
    assert len(saved) == len(want_saved)
    for bi, (got, want) in enumerate(zip(saved, want_saved)):
        for t, w, name in zip(got, want, ("x", "t1", "t2", "y")):
            assert t.is_contiguous()
            _same(t, w, (cid, bi, name))
    _same(_bhwc(y), want_saved[-1][3], (cid, "output"))
    assert y.is_contiguous(memory_format=torch.channels_last) or y.shape[2] * y.shape[3] == 1


@pytest.mark.parametrize("cid", ONE_LEAF)
def test_backward_three_ways(cid):
    """eng.backward with every .grad None; (eng(x) * r).sum().backward(); the same with x NCHW-contiguous and dy a non-contiguous view: the
    model's gradients each time."""
    blocks, eng, xd, rd, y, saved = _setup(cid)
    want = _model(cid, eng)[3]
    assert all(p.grad is None for p in eng.params)
    _grads_equal(eng.backward(saved, rd), want, (cid, "direct"))
    assert all(p.grad is None for p in eng.params)
    (eng(xd) * rd).sum().backward()
    _grads_equal([p.grad for p in eng.params], want, (cid, "autograd"))
    for p in eng.params:
        p.grad = None
    x_nchw = xd.contiguous()
    assert x_nchw.is_contiguous() and (x_nchw.shape[1] == 1 or not x_nchw.is_contiguous(memory_format=torch.channels_last))
    wide = torch.full(tuple(rd.shape[:3]) + (2 * rd.shape[3],), float("nan"), device="cuda")
    dy = wide[..., ::2]
    dy.copy_(rd)
    assert not dy.is_contiguous() and not dy.is_contiguous(memory_format=torch.channels_last)
    eng(x_nchw).backward(dy)
    _grads_equal([p.grad for p in eng.params], want, (cid, "nchw input, strided dy"))


@pytest.mark.filterwarnings("ignore:grad and param do not obey the gradient layout contract")
@pytest.mark.parametrize("cid", ONE_LEAF)
def test_accumulation_onto_an_existing_grad(cid):
    """A second backward -- with OTHER loss weights r2, so that prior + g is a rounded add and not 2 g -- adds into the first's .grad tensors
    (same storage) and gives the bits of fold_backward(..., prior = first).  A parameter whose .grad is then replaced by a non-contiguous
    tensor is handed a FRESH contiguous tensor by the engine (the kernel adds onto its zeros: exact), and the add onto the old .grad is
    autograd's AccumulateGrad: torch's add, not the kernel's -- one rounding of prior + g, so the result lies within 2^-24 of the float64 sum.
    The in-place parameters of that third backward have the bits of the kernel's add, fl(second + g), as fold_backward forms it on a prior."""
    blocks, eng, xd, rd, y, saved = _setup(cid)
    params, folds, want_saved, plain = _model(cid, eng)
    (eng(xd) * rd).sum().backward()
    _grads_equal([p.grad for p in eng.params], plain, (cid, "first"))
    ptrs = [p.grad.data_ptr() for p in eng.params]
    r2 = np.random.default_rng(EM._seed(cid, "r2")).standard_normal(EM.case_inputs(cid)[1].shape, dtype=np.float32)
    (eng(xd) * _nchw(r2)).sum().backward()
    assert [p.grad.data_ptr() for p in eng.params] == ptrs
    second = EM.backward(params, folds, want_saved, r2, 1, prior=plain)
    assert not any(np.array_equal(s2[0], 2 * g[0]) for s2, g in zip(second, plain))
    _grads_equal([p.grad for p in eng.params], second, (cid, "second"))
    # the top block's conv3 weight gets a non-contiguous .grad of the same values
    i = len(eng.params) - (6 if eng.layers[-1][1] is not None else 3)
    p = eng.params[i]
    assert p is eng.layers[-1][0][2].conv.weight
    held = torch.empty(tuple(p.shape) + (2,), device="cuda")[..., 0]
    held.copy_(p.grad)
    p.grad = held
    assert not p.grad.is_contiguous()
    (eng(xd) * rd).sum().backward()
    for j, q in enumerate(eng.params):
        if j != i:
            assert q.grad.data_ptr() == ptrs[j]
            _same(q.grad, second[j][0] + plain[j][0], (cid, "third, in place", j))
            continue
        exact = second[j][0].astype(np.float64) + plain[j][0].astype(np.float64)
        got = q.grad.detach().contiguous().cpu().numpy()
        assert got.shape == exact.shape and np.all(np.abs(got - exact) <= 2.0 ** -24 * np.abs(exact)), (cid, j)
    # and what the engine returns for it: a fresh contiguous tensor of the gradient alone for that parameter, None for all in-place ones
    again = torch.empty(tuple(p.shape) + (2,), device="cuda")[..., 0]
    again.copy_(p.grad)
    p.grad = again
    out = eng.backward(saved, rd)
    assert [g is None for g in out] == [j != i for j in range(len(out))]
    # (not the .grad in force; the first .grad's storage was released above, the allocator may hand its address out again)
    assert out[i].is_contiguous() and out[i].data_ptr() != p.grad.data_ptr()
    _same(out[i], plain[i][0], (cid, "fresh"))


@pytest.mark.parametrize("cid", LEAVES)
def test_leaf_rows(cid):
    """leaves > 1: every leaf's gradients are WRITTEN to row l of a flat buffer at the parameters' slices -- unrelated columns in front of,
    between and behind them, a sentinel row above and below -- and equal the model of that leaf ALONE; nothing else is touched, every returned
    gradient is None, no .grad appears; without leaf_grads the call raises."""
    from isx._lib import IsxError
    blocks, eng, xd, rd, y, saved = _setup(cid)
    leaves = EM.CASES[cid]["leaves"]
    params, folds, want_saved, want = _model(cid, eng)
    slices, at = {}, 7
    for k, p in enumerate(eng.params):
        slices[p] = (at, at + p.numel())
        at += p.numel() + (5, 3, 9)[k % 3]
    total = at
    buf = torch.full((leaves + 2, total), SENTINEL, device="cuda")
    flat_all = buf[1:leaves + 1]
    with pytest.raises(IsxError):
        eng.backward(saved, rd, leaves)
    out = eng.backward(saved, rd, leaves, (flat_all, slices))
    assert len(out) == len(eng.params) and all(g is None for g in out) and all(p.grad is None for p in eng.params)
    own = torch.zeros(total, dtype=torch.bool, device="cuda")
    x, r = EM.case_inputs(cid)
    per = x.shape[0] // leaves
    for l in range(leaves):
        sl = slice(l * per, (l + 1) * per)
        alone_saved = EM.forward(params, folds, x[sl])
        alone = EM.backward(params, folds, alone_saved, r[sl])
        for k, p in enumerate(eng.params):
            lo, hi = slices[p]
            own[lo:hi] = True
            _same(flat_all[l, lo:hi].reshape(p.shape), alone[k][0], (cid, l, k))
            assert np.array_equal(alone[k][0], want[k][l])
    assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()) and bool((flat_all[:, ~own] == SENTINEL).all())


def test_caches_follow_the_parameters():
    """With nothing changed the _Folded tensors keep their storage.  After an in-place change of ONE tensor -- bn3.running_mean, the projection's
    BatchNorm weight, conv3.weight -- the next forward equals the model on the new parameters, and [W3' | Wd'] and b3' + bd' follow."""
    cid = "id_p2"
    blocks, eng, xd, rd, y, saved = _setup(cid)
    names = ("istd", "scale", "bias", "w_fwd", "w_dgrad", "w_col", "w_cat", "bias_cat")

    def ptrs():
        return [getattr(f, n).data_ptr() for fb in _folded(eng) for f in fb if f is not None for n in names if getattr(f, n, None) is not None]

    before = ptrs()
    eng.forward(xd)
    assert ptrs() == before and len(before) == 2 * 3 * 5 + 5 + 2
    top = blocks[-1]
    x = EM.case_inputs(cid)[0]
    last_cat = [_folded(eng)[-1][3].w_cat.clone(), _folded(eng)[-1][3].bias_cat.clone()]
    changes = (lambda: top.bn3.running_mean.add_(0.25), lambda: top.downsample[1].weight.mul_(1.5), lambda: top.conv3.weight.mul_(0.75))
    for k, change in enumerate(changes):
        with torch.no_grad():
            change()
        y, saved = eng.forward(xd)
        params = EM.block_params(blocks)
        folds = EM.fold_all(params, _istds(eng))
        want = EM.forward(params, folds, x)
        for bi, (got, w) in enumerate(zip(saved, want)):
            for t, a in zip(got, w):
                _same(t, a, (k, bi))
        fd = _folded(eng)[-1][3]
        w_cat, bias_cat = EM.fold_cat(folds[-1][2], folds[-1][3])
        _same(fd.w_cat, w_cat, (k, "w_cat"))
        _same(fd.bias_cat, bias_cat, (k, "bias_cat"))
        # each change moves what it must: the mean the merged bias alone, the two weights [W3' | Wd'] (the projection's BatchNorm weight the bias too)
        assert torch.equal(fd.w_cat, last_cat[0]) == (k == 0) and torch.equal(fd.bias_cat, last_cat[1]) == (k == 2)
        last_cat = [fd.w_cat.clone(), fd.bias_cat.clone()]


# ---- isx_conv3x3_dgrad_nhwc under the 128x128 tile --------------------------------------------------------------------------------------------
BIG = (109, 21, 17, 32, 512)                     # B, H, W, Cout, Cin: 38 913 pixels = 304 full 128-row tiles and one with a single live row


def test_dgrad3x3_where_the_automatic_choice_is_the_128x128_tile():
    """109 images of 21 x 17, Cout = 32, Cin = 512: the smallest M at which pick_tile_cfg (restated in _suffix_model.py) takes 128x128 for 512
    columns.  With and without mask, between guards, over NaN: images 0, 54 and 108 whole against the model (an output depends on its own image
    only), every image against a second launch of the same images in reversed batch order (other tiles, other rows of them)."""
    L, check, st = _lib()
    B, H, W, Cout, Cin = BIG
    assert int(SM.pick_tile_cfg(B * H * W, Cin)) == 0 and B * H * W % 128 == 1
    dz_np = SM.inputs(B * H * W, Cout, 2101, special_rows=False).reshape(B, H, W, Cout)
    wt_np = SM.inputs(Cin, 9 * Cout, 2102, special_rows=False).reshape(Cin, 3, 3, Cout)
    mask_np = SM.mask_data((B, H, W, Cin), 2103)
    dz, wt, mask = _dev(dz_np), _dev(wt_np), _dev(mask_np)
    dz_rev, mask_rev = dz.flip(0).contiguous(), mask.flip(0).contiguous()
    picked = (0, 54, 108)
    want = SM.dgrad3x3(np.ascontiguousarray(dz_np[list(picked)]), wt_np)
    for with_mask in (True, False):
        outs = []
        for d, m in ((dz, mask), (dz_rev, mask_rev)):
            buf, dx = _guarded(B, H, W, Cin)
            check(L.isx_conv3x3_dgrad_nhwc(d.data_ptr(), B, H, W, Cout, wt.data_ptr(), Cin, m.data_ptr() if with_mask else None, dx.data_ptr(), st),
                  "isx_conv3x3_dgrad_nhwc")
            assert _guards_intact(buf)
            outs.append(dx)
        assert not bool(torch.isnan(outs[0]).any())
        assert torch.equal(outs[0], outs[1].flip(0)), with_mask
        w = SM.masked(want, mask_np[list(picked)]) if with_mask else want
        _same(outs[0][list(picked)], w, ("128x128", with_mask))
