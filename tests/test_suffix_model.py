"""tests/_suffix_model.py, the CPU model the trunk suffix's backward kernels are pinned to in tests/test_gpu_suffix_chains.py, checked on its own:

  * against float64 (torch-CPU convolution_backward, autograd through the BatchNorm fold, numpy), at the bounds tests/test_gpu_suffix.py holds
    the kernels to for the same quantity: the model is the operation, not a copy of the kernel;
  * against the plausible WRONG sums, on the data of every case the GPU test runs: where the canonical result and a wrong one give the same
    bits, a bit-exact test says nothing about it.  The share of differing elements is printed (pytest -s) and has to reach 1 %, except for the
    mask variants, where only the planted zeros can differ and all of them have to.

A wrong variant is only asked to show where it is another expression; the cases where it is the same one are left out, each with its reason.
NOT among the variants: the column sum as a fused chain fma(dz, 1, s) -- dz * 1 is exact, so it is s + dz rounded once, the same bits."""
import numpy as np
import pytest
import torch

import _suffix_model as model
from _head_model import chains

F = np.float32


def _rel(a, b):
    b = np.asarray(b, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - b).max()) / (float(np.abs(b).max()) + 1e-30)


def _share(name, case, canon, wrong, least=0.01):
    diff = float(np.mean(canon != wrong))
    print("%-36s %-36s %6.2f %% of %d elements differ" % (name, case, 100 * diff, canon.size))
    assert diff > 0 and diff >= least, (name, case, diff)
    return diff


def _splits(name):
    from isx._lib import lib
    g, Cin, Cout, _, _ = model.WGRAD_CASES[name]
    S = lib().isx_conv_wgrad_splits(model.wgrad_K(name), Cin, Cout, g.taps)
    assert S >= 1
    return S


def _t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


# ---- the model against float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", model.WGRAD_CASES)
def test_wgrad_against_float64(name):
    """The partials of a leaf add up to the weight gradient of its images (2e-5 of the largest entry) and to the column sums of its dz (1e-5)."""
    g, Cin, Cout, leaves, which = model.WGRAD_CASES[name]
    dz, x = model.wgrad_inputs(name)
    dw, db = model.wgrad_case(name, _splits(name))
    Ho, Wo = model.out_hw(g)
    per, k = g.B // leaves, 3 if g.taps == 9 else 1
    X = _t64(x).view(g.B, g.H, g.W, Cin).permute(0, 3, 1, 2)
    DZ = _t64(dz).view(g.B, Ho, Wo, Cout).permute(0, 3, 1, 2)
    for i, l in enumerate(range(leaves) if which is None else which):
        sl = slice(l * per, (l + 1) * per)
        _, gw, _ = torch.ops.aten.convolution_backward(DZ[sl].contiguous(), X[sl].contiguous(), torch.zeros(Cout, Cin, k, k, dtype=torch.float64), None, [g.stride] * 2,
                                                       [k // 2] * 2, [1, 1], False, [0, 0], 1, [False, True, False])
        got = dw[i].astype(np.float64).sum(0).reshape(Cout, k, k, Cin).transpose(0, 3, 1, 2)
        assert _rel(got, gw.numpy()) <= 2e-5, (name, l)
        assert _rel(db[i].astype(np.float64).sum(0), DZ[sl].sum((0, 2, 3)).numpy()) <= 1e-5, (name, l)


def test_wgrad_short_and_empty_split_is_what_the_case_says():
    name = "1x1_short_and_empty_split"
    S = _splits(name)
    kt_per, ranges = model.split_ranges(model.wgrad_K(name), S)
    assert (S, kt_per) == (10, 5) and ranges[8] == (1280, 1300) and ranges[9] == (1300, 1300)
    dw, db = model.wgrad_case(name, S)
    assert not dw[0, 9].any() and not db[0, 9].any() and dw[0, 8].any()


@pytest.mark.parametrize("taps,Cin,leaves,S", model.FOLD_CASES)
def test_fold_backward_against_float64_autograd(taps, Cin, leaves, S):
    """Autograd in float64 through the fold w' = w * s, b' = beta - mean * s, s = gamma * istd: gw within 1e-5, ggamma 1e-4, gbeta 1e-6 of the
    largest entry; the accumulating call adds exactly that onto the priors."""
    dwp, db, prior, plain, acc = model.fold_case(taps, Cin, leaves, S)
    w, scale, mean, istd = model.fold_params(taps, Cin)
    for l in range(leaves):
        w64 = _t64(w).requires_grad_()
        gam, bet = (_t64(scale) / _t64(istd)).requires_grad_(), torch.zeros(model.FOLD_COUT, dtype=torch.float64).requires_grad_()
        s = gam * _t64(istd)
        wf, bf = w64 * s.view(-1, 1, 1), bet - _t64(mean) * s
        ((wf.permute(0, 2, 1) * _t64(dwp[l]).sum(0)).sum() + (bf * _t64(db[l]).sum(0)).sum()).backward()
        assert _rel(plain[0][l], w64.grad.numpy()) <= 1e-5 and _rel(plain[1][l], gam.grad.numpy()) <= 1e-4 and _rel(plain[2][l], bet.grad.numpy()) <= 1e-6
    for a, p, q in zip(acc, prior, plain):
        assert np.array_equal(a, p + q)


@pytest.mark.parametrize("Cin", model.DGRAD1_CIN)
@pytest.mark.parametrize("Cout", model.DGRAD1_COUT)
def test_dgrad1x1_against_float64(Cin, Cout):
    dz, wt, add, mask, v = model.dgrad1_case(Cin, Cout)
    assert np.array_equal(model.dgrad1x1(dz, wt), v) and np.array_equal(model.dgrad1x1(dz[:65], wt, add[:65], mask[:65]), model.dgrad1_want(Cin, Cout, 65, True, True))
    ref = dz.astype(np.float64) @ wt.astype(np.float64).T
    np.testing.assert_allclose(v, ref.astype(F), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(model.dgrad1x1(dz, wt, add, mask), ((ref + add) * (mask > 0)).astype(F), rtol=1e-4, atol=1e-3)


def _w_oihw(wt):
    """wt[ci][kh][kw][co] = w'[co][2-kh][2-kw][ci], undone."""
    return _t64(wt[:, ::-1, ::-1].copy()).permute(3, 0, 1, 2).contiguous()


@pytest.mark.parametrize("name", model.DGRAD3_CASES)
def test_dgrad3x3_against_float64(name):
    B, H, W, Cout, Cin, up = model.DGRAD3_CASES[name]
    dz, wt, mask, v = model.dgrad3_case(name)
    DZ = _t64(dz).permute(0, 3, 1, 2).contiguous()
    gx, _, _ = torch.ops.aten.convolution_backward(DZ, torch.zeros(B, Cin, H, W, dtype=torch.float64), _w_oihw(wt), None, [1, 1], [1, 1], [1, 1], False, [0, 0], 1,
                                                   [True, False, False])
    want = gx.permute(0, 2, 3, 1).numpy()
    assert _rel(v, want) <= 2e-5
    assert _rel(model.dgrad3x3(dz, wt, mask), want * (mask > 0)) <= 2e-5
    if up:                                        # and it is the input gradient of the stride-2 convolution whose gradient lies on the even pixels
        g2, _, _ = torch.ops.aten.convolution_backward(DZ[:, :, ::2, ::2].contiguous(), torch.zeros(B, Cin, H, W, dtype=torch.float64), _w_oihw(wt), None, [2, 2],
                                                       [1, 1], [1, 1], False, [0, 0], 1, [True, False, False])
        assert _rel(v, g2.permute(0, 2, 3, 1).numpy()) <= 2e-5


@pytest.mark.parametrize("B,H,W,Cin", model.COL2IM_CASES)
def test_col2im_against_float64_scatter(B, H, W, Cin):
    """The gather of the model against the scatter of the definition: tap (kh, kw) of output pixel (ho, wo) goes to (2 ho + kh - 1, 2 wo + kw - 1)."""
    dcol, mask, v = model.col2im_case(B, H, W, Cin)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    d = dcol.astype(np.float64).reshape(B, Ho, Wo, 9, Cin)
    want = np.zeros((B, H, W, Cin))
    for ho in range(Ho):
        for wo in range(Wo):
            for kh in range(3):
                for kw in range(3):
                    h, w = 2 * ho + kh - 1, 2 * wo + kw - 1
                    if 0 <= h < H and 0 <= w < W:
                        want[:, h, w] += d[:, ho, wo, kh * 3 + kw]
    assert _rel(v, want) <= 2e-5
    assert _rel(model.col2im_s2(dcol, B, H, W, Cin, mask), want * (mask > 0)) <= 2e-5


@pytest.mark.parametrize("n", model.RELU_N)
def test_relu_grad_is_exact(n):
    dy, y, dz = model.relu_case(n)
    assert np.array_equal(dz, dy * (y > 0))
    assert not dz[y == 0].any() and np.signbit(y[y == 0]).any() and not np.signbit(y[y == 0]).all()


# ---- the model discriminates: weight gradient ---------------------------------------------------------------------------------------------------
def _src_clamped(g, dh, dw):
    """WRONG: a source outside the map reads the edge pixel."""
    b, h, w = model.src_bhw(g, dh, dw)
    return (b * g.H + np.clip(h, 0, g.H - 1)) * g.W + np.clip(w, 0, g.W - 1)


@pytest.mark.parametrize("name", model.WGRAD_CASES)
def test_wgrad_orders_show_in_the_data(name):
    g, Cin, Cout, leaves, which = model.WGRAD_CASES[name]
    dz, x = model.wgrad_inputs(name)
    S, K = _splits(name), model.wgrad_K(name)
    dw, db = model.wgrad_case(name, S)
    ls = range(leaves) if which is None else which
    nk = (K + 31) // 32
    ranges = model.split_ranges(K, S)[1]
    offs = model.tap_offsets(g.taps)
    srcs = [model.src_rows(g, dh, dw_) for dh, dw_ in offs]

    def run(srcs=srcs, ranges=ranges, order=lambda p: p, carry=False):
        def pixels(l, s):
            own = order(np.arange(l * K + ranges[s][0], l * K + ranges[s][1]))
            return np.concatenate([order(np.arange((l - 1) * K + ranges[s][0], (l - 1) * K + ranges[s][1])), own]) if carry and l > 0 else own
        return model.wgrad_from(dz, x, srcs, ls, S, pixels)

    assert all(np.array_equal(a, b) for a, b in zip(run(), (dw, db)))          # the harness of the variants is the model
    both, only_dw = {}, {}
    floor = [(32 * s * (nk // S), K if s == S - 1 else 32 * (s + 1) * (nk // S)) for s in range(S)]
    if floor != ranges:                           # S divides nk (S = 1 among them): floor and ceil are one rule
        both["splits cut at floor"] = run(ranges=floor)
    per64 = ((K + 63) // 64 + S - 1) // S
    tiles64 = [(min(K, 64 * s * per64), min(K, 64 * (s + 1) * per64)) for s in range(S)]
    if tiles64 != ranges:                         # one split, or kt_per even: the cuts of 64-pixel tiles fall on the same pixels
        both["k-tiles of 64 pixels"] = run(ranges=tiles64)
    both["pixels in reverse order"] = run(order=lambda p: p[::-1])              # (every case has a split of >= 3 pixels: another sum for db too)
    if leaves > 1:                                # (leaf 0 has no predecessor: at most (leaves - 1) / leaves of the elements can differ)
        both["sum continues from the previous leaf"] = run(carry=True)
    if g.taps == 9:                               # taps == 1: one tap, and a strided 1x1 source never leaves the map
        only_dw["taps transposed (dw, dh)"] = run(srcs=[model.src_rows(g, dw_, dh) for dh, dw_ in offs])
        only_dw["border source clamped to the edge"] = run(srcs=[_src_clamped(g, dh, dw_) for dh, dw_ in offs])
    if name in ("1x1_short_and_empty_split", "3x3_three_leaves") + model.WGRAD_BIG:       # the cases with an odd kt_per that does not divide nk
        assert "splits cut at floor" in both and "k-tiles of 64 pixels" in both
    for what, (bad_dw, bad_db) in both.items():
        _share(what, "wgrad dw " + name, dw, bad_dw)
        _share(what, "wgrad db " + name, db, bad_db)
    for what, (bad_dw, bad_db) in only_dw.items():
        _share(what, "wgrad dw " + name, dw, bad_dw)
        assert np.array_equal(bad_db, db)


# ---- the model discriminates: chain rule of the fold ---------------------------------------------------------------------------------------------
def _block_dot_fused(d, w):
    """WRONG: the per-thread sums as fma(d_i, w_i, acc) (float64 holds the product of two floats exactly)."""
    K = d.shape[-1]
    n = (K + 255) // 256
    d64, w64 = np.zeros(d.shape[:-1] + (n * 256,)), np.zeros(d.shape[:-1] + (n * 256,))
    d64[..., :K], w64[..., :K] = d, w
    v = np.zeros(d.shape[:-1] + (256,), F)
    for j in range(n):
        v = (d64[..., j * 256:(j + 1) * 256] * w64[..., j * 256:(j + 1) * 256] + v).astype(F)
    return model.block_dot(v)                     # 256 sums: one per thread, then the same reduction


@pytest.mark.parametrize("taps,Cin,leaves,S", model.FOLD_CASES)
def test_fold_orders_show_in_the_data(taps, Cin, leaves, S):
    dwp, db, _, (gw, gg, gb), _ = model.fold_case(taps, Cin, leaves, S)
    w, scale, mean, istd = model.fold_params(taps, Cin)
    case = "fold taps=%d Cin=%d leaves=%d S=%d" % (taps, Cin, leaves, S)
    lds = model.fold_lds_path(taps, Cin)
    assert lds == ((taps, Cin) in ((9, 64), (9, 512)))
    d, dbs = model.fold_sum(np.moveaxis(dwp, 1, 0)), model.fold_sum(np.moveaxis(db, 1, 0))
    assert np.array_equal(model.fold_ggamma(model.fold_dot(d, w, lds), mean, dbs, istd), gg) and np.array_equal(dbs, gb)
    if S >= 3:                                    # one partial: nothing to add; two commute
        bad = model.fold_backward(dwp[:, ::-1], db[:, ::-1], w, scale, mean, istd, taps)
        _share("partials added in reverse order", case + " gw", gw, bad[0])
        _share("partials added in reverse order", case + " gbeta", gb, bad[2])
    if taps > 1:                                  # taps == 1: (ci, tap) and (tap, ci) are one layout
        _share("dot over the other layout", case + " ggamma", gg, model.fold_ggamma(model.fold_dot(d, w, not lds), mean, dbs, istd))
    if taps * Cin > 256:                          # up to 256 products a thread has one: fma(d, w, 0) is the rounded product
        a, b = (np.swapaxes(d, -1, -2), w) if lds else (d, np.swapaxes(w, -1, -2))
        fused = _block_dot_fused(*(np.ascontiguousarray(np.broadcast_to(t, a.shape)).reshape(a.shape[:-2] + (-1,)) for t in (a, b)))
        _share("dot with fused multiply-add", case + " ggamma", gg, model.fold_ggamma(fused, mean, dbs, istd))
    dot = model.fold_dot(d, w, lds)
    _share("ggamma as dot*istd - mean*dbs*istd", case + " ggamma", gg, dot * istd - mean * dbs * istd)


# ---- the model discriminates: input gradients --------------------------------------------------------------------------------------------------
def _mask_variant(case, v, mask, canon):
    """mask >= 0 instead of > 0: exactly the planted zeros (both signs) change, all of them."""
    wrong = np.where(mask >= 0, v, F(0))
    planted = mask == 0
    assert planted.any() and np.signbit(mask[planted]).any() and not np.signbit(mask[planted]).all()
    print("%-36s %-36s %d planted zeros, %d elements differ" % ("mask >= 0", case, int(planted.sum()), int((wrong != canon).sum())))
    assert np.array_equal(wrong != canon, planted), case


@pytest.mark.parametrize("M", model.DGRAD1_M)
@pytest.mark.parametrize("Cin", model.DGRAD1_CIN)
@pytest.mark.parametrize("Cout", model.DGRAD1_COUT)
def test_dgrad1x1_orders_show_in_the_data(Cout, Cin, M):
    _, _, add, mask, v = model.dgrad1_case(Cin, Cout)
    case = "dgrad1x1 M=%d Cin=%d Cout=%d" % (M, Cin, Cout)
    v, add, mask = v[:M], add[:M], mask[:M]
    _mask_variant(case, v, mask, model.dgrad1_want(Cin, Cout, M, False, True))
    _mask_variant(case + " +add", v + add, mask, model.dgrad1_want(Cin, Cout, M, True, True))
    _share("add applied after the mask", case, model.dgrad1_want(Cin, Cout, M, True, True), model.masked(v, mask) + add)


def _two_level(rows, w, chunk=64):
    """WRONG for the gradients: the inference trunk's sum -- a chain per 64 terms, the chains added in order from +0."""
    tot = np.zeros((rows.shape[0], w.shape[0]), F)
    for k in range(0, rows.shape[1], chunk):
        tot = tot + chains(rows[:, k:k + chunk], w[:, k:k + chunk])
    return tot


@pytest.mark.parametrize("name", model.DGRAD3_CASES)
def test_dgrad3x3_orders_show_in_the_data(name):
    dz, wt, mask, v = model.dgrad3_case(name)
    _share("two-level sum, chunks of 64", "dgrad3x3 " + name, v, _two_level(model.dgrad3x3_rows(dz), wt.reshape(wt.shape[0], -1)).reshape(v.shape))
    _mask_variant("dgrad3x3 " + name, v, mask, model.dgrad3x3(dz, wt, mask))


@pytest.mark.parametrize("B,H,W,Cin", model.COL2IM_CASES)
def test_col2im_orders_show_in_the_data(B, H, W, Cin):
    dcol, mask, v = model.col2im_case(B, H, W, Cin)
    case = "col2im %dx%dx%dx%d" % (B, H, W, Cin)
    if H >= 3 and W >= 3:                         # below that no pixel collects four taps, and up to two taps commute
        _share("taps in (kw, kh) order", case, v, model.col2im_s2(dcol, B, H, W, Cin, order=[(a, b) for b in range(3) for a in range(3)]))
    _mask_variant(case, v, mask, model.col2im_s2(dcol, B, H, W, Cin, mask))


@pytest.mark.parametrize("n", model.RELU_N[1:])
def test_relu_mask_shows_in_the_data(n):
    dy, y, dz = model.relu_case(n)
    _mask_variant("relu_grad n=%d" % n, dy, y, dz)
