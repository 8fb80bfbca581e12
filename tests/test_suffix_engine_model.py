"""CPU side of the suffix-engine model (tests/_suffix_engine_model.py): the model is the operation (float64 autograd on the UNFOLDED blocks, the
project's 1e-5 criterion of tests/test_gpu_suffix.py), every wiring mistake of WRONGS moves at least one bit of at least one gradient on every
case it can apply to, a dropped eps moves istd by more than the GPU test's bound on it, the split rule and the tile choice of the 3x3 input
gradient are restated as host arithmetic.  The GPU side, which holds isx/suffix.py to the model bit for bit, is tests/test_gpu_suffix_engine.py."""
import copy

import numpy as np
import pytest
import torch

import _suffix_engine_model as EM
import _suffix_model as SM
from test_gpu_suffix import _ref64_with_masks, _rel           # the float64 arbiter and the criterion of the whole-step test (plain functions)

# what the GPU test allows between the engine's istd and float64 at most (tests/test_gpu_suffix_engine.py keeps its bound below this cap)
ISTD_CAP = 8 * 2.0 ** -24


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _nchw64(a):
    return torch.from_numpy(np.array(a)).permute(0, 3, 1, 2).double()


def _autograd64(cid, saved, x, r):
    """(y, [gradient per parameter in the engine's order]) of the unfolded blocks in float64 with the model's own ReLU pattern."""
    seq = torch.nn.Sequential(*copy.deepcopy(EM.make_blocks(cid))).double()
    masks = [tuple(_nchw64(t > 0) for t in (t1, t2, y)) for _, t1, t2, y in saved]
    y = _ref64_with_masks(seq, _nchw64(x), masks)
    (y * _nchw64(r)).sum().backward()
    grads = []
    for b in seq:
        for conv, bn in [(b.conv1, b.bn1), (b.conv2, b.bn2), (b.conv3, b.bn3)] + ([tuple(b.downsample)] if b.downsample is not None else []):
            grads += [conv.weight.grad, bn.weight.grad, bn.bias.grad]
    return y.detach(), grads


@pytest.mark.parametrize("cid", sorted(EM.CASES))
def test_model_is_the_operation(cid):
    """Output and every parameter gradient within 1e-5 of the tensor's largest entry of torch CPU float64 autograd on the unfolded blocks, the
    ReLUs replaced by the model's own masks.  A case of several leaves: every leaf against autograd on its own images, and the model of the
    whole batch has, leaf by leaf, the bits of the model of that leaf ALONE (what the GPU test compares the engine with)."""
    leaves = EM.CASES[cid]["leaves"]
    params = EM.case_params(cid)
    x, r = EM.case_inputs(cid)
    saved, grads = EM.case_cpu(cid)
    per = x.shape[0] // leaves
    for l in range(leaves):
        sl = slice(l * per, (l + 1) * per)
        sv = [tuple(t[sl] for t in s) for s in saved]
        y64, g64 = _autograd64(cid, sv, x[sl], r[sl])
        assert _rel(_nchw64(sv[-1][3]), y64) <= 1e-5
        assert len(g64) == len(grads)
        for i, (g, want) in enumerate(zip(grads, g64)):
            assert g.dtype == np.float32 and g[l].shape == tuple(want.shape), (cid, i)
            assert _rel(torch.from_numpy(g[l].copy()).double(), want) <= 1e-5, (cid, l, i)
        if leaves > 1:
            sv1, g1 = EM.run(params, EM.istd32(params), x[sl], r[sl])
            assert all(_same_bits(a, b) for s, t in zip(sv, sv1) for a, b in zip(s, t))
            assert all(_same_bits(g[l], h[0]) for g, h in zip(grads, g1)), (cid, l)


def _cannot_apply(case):
    """The WRONGS that the structure of a case leaves nothing to apply to."""
    blocks, leaves = case["blocks"], case["leaves"]
    out = set()
    if not any(proj for _, _, _, proj in blocks):                                    # no projection
        out |= {"w_cat_swapped", "proj_wgrad_reads_t2_rows", "add_unscattered_phase"}
    if not any(proj for _, _, _, proj in blocks[1:]):                                # projection only in the bottom block: its dd is never formed
        out.add("add_unscattered_phase")
    if not any(proj and stride == 2 for _, _, stride, proj in blocks[1:]):           # stride 1: no phase to misplace
        out.add("add_unscattered_phase")
    if not any(proj and stride == 2 for _, _, stride, proj in blocks):               # stride 1: t2's rows ARE the projection's
        out.add("proj_wgrad_reads_t2_rows")
    if len(blocks) == 1:                                                             # one block: no input gradient below it, nothing is added
        out.add("no_add")
    if all(stride == 2 for _, _, stride, _ in blocks):                               # w_dgrad of a 3x3 exists at stride 1 only,
        out.add("no_tap_flip")
    if all(stride == 1 for _, _, stride, _ in blocks):                               # w_col at stride 2 only
        out.add("w_col_tap_major_swapped")
    if leaves == 1:                                                                  # one leaf
        out |= {"leaves_share_one_sum", "leaf_rows_swapped"}
    else:                                                                            # per-leaf rows are written (accumulate = 0)
        out.add("accumulate_overwrites")
    return out


def test_every_wrong_applies_somewhere():
    assert set(EM.WRONGS).isdisjoint(EM.WRONGS_TOL)
    applies = set()
    for case in EM.CASES.values():
        applies |= set(EM.WRONGS) - _cannot_apply(case)
    assert applies == set(EM.WRONGS)
    assert _cannot_apply(EM.CASES["id_p2"]) == {"leaves_share_one_sum", "leaf_rows_swapped"}
    assert _cannot_apply(EM.CASES["id_p2_leaves"]) == {"accumulate_overwrites"}


@pytest.mark.parametrize("cid", sorted(EM.CASES))
def test_every_applicable_wrong_moves_a_bit(cid):
    """Non-vacuity at the bit level: each mistake that can apply to the case changes at least one bit of at least one gradient; each one that
    cannot (re-derived from the blocks, the strides and the leaf count above) changes none.  The gradients of a case of one leaf are those of
    a SECOND backward onto the first's (the only place where accumulate = 1 shows)."""
    case = EM.CASES[cid]
    params = EM.case_params(cid)
    istds = EM.istd32(params)
    x, r = EM.case_inputs(cid)
    _, first = EM.case_cpu(cid)
    prior = list(first) if case["leaves"] == 1 else None
    _, right = EM.run(params, istds, x, r, case["leaves"], prior)
    if prior is not None:
        assert not any(_same_bits(a, b) for a, b in zip(right, first))
    cannot = _cannot_apply(case)
    for wrong in sorted(EM.WRONGS):
        _, got = EM.run(params, istds, x, r, case["leaves"], prior, wrong)
        assert all(a.shape == b.shape and a.dtype == np.float32 for a, b in zip(got, right))
        moved = sum(not _same_bits(a, b) for a, b in zip(got, right))
        assert (moved == 0) == (wrong in cannot), (cid, wrong, moved)


@pytest.mark.parametrize("cid", ["id_p2", "p1_id"])
def test_model_fold_has_the_layouts_of_the_engines_fold_on_the_cpu(cid):
    """_Folded.refresh is plain torch: on CPU tensors, given ITS istd, scale, bias and every layout have the model's bits."""
    from isx.suffix import SuffixEngine
    blocks = EM.make_blocks(cid)
    eng = SuffixEngine(blocks)
    params = EM.case_params(cid)
    for (convs, down), blk in zip(eng.layers, params):
        for f, c in zip(list(convs) + ([down] if down is not None else []), blk):
            f.refresh()
            m = EM.fold(c, f.istd.numpy())
            for name in ("scale", "bias", "w_fwd", "w_dgrad", "w_col"):
                want = getattr(m, name)
                if want is not None:
                    assert _same_bits(getattr(f, name).numpy(), want), (cid, name)
            assert (m.w_col is None) == (c.taps == 1 or c.stride == 1) and (m.w_dgrad is None) == (c.taps == 9 and c.stride == 2)


def test_eps_dropped_moves_istd_beyond_the_gpu_bound():
    """istd without eps: |istd' - istd| / istd >= eps / (2 * 1.5) * (1 - 1e-3) for every channel -- 3.3e-6 at eps = 1e-5 and variances in
    [0.5, 1.5] -- a factor 6.98 above the cap of the GPU test's bound on istd; and the float32 values the model is handed differ in every channel."""
    for cid in sorted(EM.CASES):
        for blk in EM.case_params(cid):
            for c in blk:
                if c is None:
                    continue
                assert c.eps == 1e-5 and 0.5 <= c.var.min() and c.var.max() <= 1.5
                a, b = EM.istd64(c), EM.istd64(c, eps_dropped=True)
                moved = np.abs(b - a) / a
                assert moved.min() >= c.eps / (2 * 1.5) * (1 - 1e-3)
                assert c.eps / (2 * 1.5) * (1 - 1e-3) > 6.9 * ISTD_CAP
                assert (a.astype(np.float32) != b.astype(np.float32)).all()
    params = EM.case_params("id_id")
    x, r = EM.case_inputs("id_id")
    _, got = EM.run(params, EM.istd32(params, eps_dropped=True), x, r)
    # (gbeta of the top conv3 is the column sum of relu_grad(r, y): istd reaches it through the sign of y alone)
    assert not any(_same_bits(a, b) for i, (a, b) in enumerate(zip(got, EM.case_cpu("id_id")[1])) if i % 3 != 2)


def test_split_rule_restated():
    """wgrad_splits of csrc/backward.hip in Python: the three values tests/test_gpu_suffix_chains.py reads from the library, one split for an
    empty launch, and the bounds of the rule -- at least four k-tiles of 32 pixels per split, sixteen splits at most -- on layer4's shapes and on
    every convolution of the cases here.  The GPU test asserts equality with isx_conv_wgrad_splits for every convolution of every case."""
    assert EM.wgrad_splits(1300, 64, 64, 1) == 10 and EM.wgrad_splits(272, 128, 128, 9) == 2 and EM.wgrad_splits(1147, 256, 256, 1) == 8
    assert EM.wgrad_splits(0, 64, 64, 9) == 1
    for K, Cin, Cout, taps in SM.LAYER4_SHAPES:
        assert 1 <= EM.wgrad_splits(K, Cin, Cout, taps) <= 16
    shapes = [s for cid in EM.CASES for s in EM.conv_shapes(cid)]
    assert len(shapes) == 3 * 13 + 5
    for K, Cin, Cout, taps in shapes:
        S = EM.wgrad_splits(K, Cin, Cout, taps)
        assert 1 <= S <= max(1, ((K + 31) // 32) // 4)


# ---- the tile shape of isx_conv3x3_dgrad_nhwc ----------------------------------------------------------------------------------------------------
def test_dgrad3x3_tile_choice_restated():
    """What SM.pick_tile_cfg -- a restatement of csrc/gemm.hip that nobody can check against the library, the function is not exported -- says
    about isx_conv3x3_dgrad_nhwc (pick_tile_cfg(M, N, 0, kEff3x3, 0xD)):
      * layer4's launches take 64x64: 1176 x 512 for one leaf, 9408 x 512 for eight;
      * 128x128 first wins at M = 38 913 (N = 512), 77 825 (256), 155 649 (128);
      * 128x64 never wins for N = 64 .. 2048 and any M up to 3 000 000.  The estimate of a shape depends on M through ceil(M / 64) (64x64) or
        ceil(M / 128) alone, so it is constant on every interval (64 (j - 1), 64 j]: one M per interval is every M."""
    assert int(SM.pick_tile_cfg(1176, 512)) == 3 and int(SM.pick_tile_cfg(9408, 512)) == 3
    for N, first in ((512, 38913), (256, 77825), (128, 155649)):
        M = np.arange(1, first + 130, dtype=np.int64)
        cfg = SM.pick_tile_cfg(M, N)
        assert int(M[np.argmax(cfg == 0)]) == first and not (cfg[:first - 1] == 0).any() and (cfg[first - 1:] == 0).all()
        assert first % 128 == 1                                   # the first M of a new 128-row tile: that tile has one live row
    ends = np.arange(1, 3_000_000 // 64 + 2, dtype=np.int64) * 64
    t = SM.tile_times(np.arange(1, 1025), 512)
    assert all(np.array_equal(t[:, 64 * j:64 * j + 64], np.repeat(t[:, 64 * j:64 * j + 1], 64, 1)) for j in range(16))
    for N in range(64, 2049, 64):
        cfg = SM.pick_tile_cfg(ends, N)
        assert not (cfg == 2).any() and not (cfg == 1).any(), N
    # the case tests/test_gpu_suffix_engine.py runs: 109 images of 21 x 17, 512 columns
    assert 109 * 21 * 17 == 38913 == 304 * 128 + 1 and int(SM.pick_tile_cfg(38913, 512)) == 0 and int(SM.pick_tile_cfg(38912, 512)) == 3
    # The other launches of this entry in the suite, by tile.  DGRAD3_CASES (tests/test_gpu_suffix_chains.py, test_gpu_special_values.py,
    # test_gpu_stream_order.py) and the four 3x3 shapes of test_backward_kernels_vs_torch (tests/test_gpu_suffix.py: B, H, W, Cin) take 64x64 ...
    assert all(int(SM.pick_tile_cfg(B * H * W, Cin)) == 3 for B, H, W, _, Cin, _ in SM.DGRAD3_CASES.values())
    assert all(int(SM.pick_tile_cfg(B * H * W, Cin)) == 3 for B, H, W, Cin in ((2, 6, 5, 64), (3, 7, 7, 128), (8, 14, 14, 64), (2, 14, 14, 64)))
    # ... and ONE takes 128x128: the case of tests/test_gpu_large_tensors.py (171 199 images of 7 x 7, Cout = 64, Cin = 256, mask, compared with
    # dgrad3x3 on its period rows) -- the 128x128 gradient instance far inside its range, 65 537 full tiles and one of 15 rows; the case of
    # tests/test_gpu_suffix_engine.py is that instance at its FIRST row count.  No launch of the suite takes 128x64.
    from test_gpu_large_tensors import SMALL_MAPS
    B, Hh = SMALL_MAPS
    assert (B, Hh) == (171199, 7) and B * Hh * Hh == 8388751 == 65537 * 128 + 15 and B * Hh * Hh > 77825
    assert int(SM.pick_tile_cfg(B * Hh * Hh, 256)) == 0
