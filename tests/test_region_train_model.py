"""The CPU model of the region descriptor's training kernels (tests/_region_train_model.py) against float64 torch autograd within its derived
bounds and against the readings the GPU test must tell apart; argument validation of the two entries without a GPU; the two contract classes of
the training step; what train.siamese_regions declares to it."""
import numpy as np
import pytest
import torch

import _region_train_model as M
from _desc_model import F, gather_nhwc_ss



def _autograd64(fmap, idx, Wp, kh, kw, shift, g, add):
    """gather -> NormalizeL2 -> Shift -> sum over the windows with the library's own modules, float64."""
    from model.custom_modules import NormalizeL2, Shift
    x = torch.from_numpy(np.array(fmap)).double().requires_grad_(True)
    l2, sh = NormalizeL2(), None
    if shift is not None:
        sh = Shift(len(shift)).double()
        with torch.no_grad():
            sh.param.copy_(torch.from_numpy(np.array(shift)).double())
    rows = []
    for b in range(x.size(0)):
        acc = torch.zeros(x.size(1) * kh * kw, dtype=torch.float64)
        for fi in np.asarray(idx[b]).tolist():
            if fi < 0:
                continue
            r, c = fi // Wp, fi % Wp
            t = l2(x[b:b + 1, :, r:r + kh, c:c + kw].reshape(1, -1))
            acc = acc + (sh(t) if sh is not None else t)[0]
        rows.append(acc)
    rows = torch.stack(rows)
    obj = (rows * torch.from_numpy(np.array(g)).double()).sum()
    if add is not None:
        obj = obj + (x * torch.from_numpy(np.array(add)).double()).sum()
    obj.backward()
    return rows.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("with_opt", (True, False))
def test_model_within_derived_bound_of_float64_autograd(case, with_opt):
    B, Hf, Wf, C, kh, kw, k = case
    fmap, idx, Wp, shift, g, add = M.make_case(case)
    sh, ad = (shift, add) if with_opt else (None, None)
    rows, n2 = M.region_sum_l2(fmap, kh, kw, idx, Wp, sh)
    df, _ = M.region_sum_l2_bwd(fmap, g, n2, kh, kw, idx, Wp, ad)
    r64, d64 = _autograd64(fmap, idx, Wp, kh, kw, sh, g, ad)
    # the model's own float64 twin is the autograd result, up to eps: the kernels' eps is the fp32 nearest to 1e-10 (2^-25 relative to the
    # module's double; it matters where a window is all zero and n2 = eps)
    assert np.abs(M.region_sum_l2_64(fmap, kh, kw, idx, Wp, sh) - r64).max() <= 1e-7
    assert np.abs(M.region_sum_l2_bwd64(fmap, g, kh, kw, idx, Wp, ad) - d64).max() <= 1e-7 * max(1.0, np.abs(d64).max())
    rb = M.rows_bound(fmap, kh, kw, idx, Wp, sh)
    db = M.dfmap_bound(fmap, g, kh, kw, idx, Wp, ad)
    e_r, e_d = np.abs(rows.astype(np.float64) - r64), np.abs(df.astype(np.float64) - d64)
    print("model vs float64 %s opt=%d: rows %.3g (bound %.3g), dfmap %.3g (bound %.3g)" % (case, with_opt, e_r.max(), rb.max(), e_d.max(), db.max()))
    assert (e_r <= rb).all() and (e_d <= db).all()


def test_sum_of_squares_is_the_nhwc_gather_order():
    x = np.random.default_rng(3).standard_normal((3, 4 * 1500)).astype(F)
    assert np.array_equal(M.block_sum(M.one_by_one(x * x)), gather_nhwc_ss(x))


def test_other_window_orders_and_an_early_class_term_change_bits():
    """The readings the GPU test has to be able to see: windows added in descending order; `add` in front of the window terms."""
    fwd = bwd = early = 0
    for case in M.CASES:
        B, Hf, Wf, C, kh, kw, k = case
        fmap, idx, Wp, shift, g, add = M.make_case(case)
        rows, n2 = M.region_sum_l2(fmap, kh, kw, idx, Wp, shift)
        df, _ = M.region_sum_l2_bwd(fmap, g, n2, kh, kw, idx, Wp, add)
        rev = list(range(k))[::-1]
        fwd += int((M.region_sum_l2(fmap, kh, kw, idx, Wp, shift, order=rev)[0] != rows).sum())
        bwd += int((M.region_sum_l2_bwd(fmap, g, n2, kh, kw, idx, Wp, add, order=rev)[0] != df).sum())
        early += int((M.region_sum_l2_bwd(fmap, g, n2, kh, kw, idx, Wp, add, add_first=True)[0] != df).sum())
    assert fwd > 0 and bwd > 0 and early > 0, (fwd, bwd, early)


def test_skipped_entries_contribute_nothing():
    case = M.SKIP_CASE
    B, Hf, Wf, C, kh, kw, k = case
    fmap, idx, Wp, shift, g, add = M.make_case(case)
    rows, n2 = M.region_sum_l2(fmap, kh, kw, idx, Wp, shift)
    keep = [w for w in range(k) if idx[1, w] >= 0]
    r1, n1 = M.region_sum_l2(fmap[1:], kh, kw, idx[1:, keep], Wp, shift)
    assert np.array_equal(rows[1:], r1) and n2[1, 1] == 0 and np.array_equal(n2[1, keep], n1[0])
    out_of_range = idx.copy()
    out_of_range[1, 1] = (Hf - kh + 1) * Wp                                    # the first index past the map: skipped like -1
    assert np.array_equal(M.region_sum_l2(fmap, kh, kw, out_of_range, Wp, shift)[0], rows)


def test_argument_validation_without_gpu():
    from isx import _lib
    lib = _lib.lib()
    P = [256 * (i + 1) for i in range(8)]
    fwd = lambda **kw_: lib.isx_region_sum_l2_nhwc(*[kw_.get(n, d) for n, d in (
        ("fmap", P[0]), ("B", 2), ("C", 8), ("Hf", 9), ("Wf", 9), ("kh", 7), ("kw", 7), ("idx", P[1]), ("k", 6), ("Wp", 3), ("shift", P[2]), ("eps", 1e-10),
        ("rows", P[3]), ("n2", P[4]), ("stream", None))])
    bwd = lambda **kw_: lib.isx_region_sum_l2_bwd_nhwc(*[kw_.get(n, d) for n, d in (
        ("fmap", P[0]), ("g", P[1]), ("n2", P[2]), ("B", 2), ("C", 8), ("Hf", 9), ("Wf", 9), ("kh", 7), ("kw", 7), ("idx", P[3]), ("k", 6), ("Wp", 3),
        ("add", P[4]), ("add_every", 1), ("cw", P[5]), ("dfmap", P[6]), ("stream", None))])
    for entry, name in ((fwd, b"isx_region_sum_l2_nhwc"), (bwd, b"isx_region_sum_l2_bwd_nhwc")):
        for bad in (dict(Wp=4), dict(kh=10), dict(k=0), dict(B=65536), dict(C=0), dict(B=-1)):
            assert entry(**bad) == -1 and b"bad shape" in lib.isx_last_error() and name in lib.isx_last_error(), bad
        assert entry(C=6) == -1 and b"multiple of 4" in lib.isx_last_error()
        assert entry(fmap=24) == -1 and b"16-B aligned" in lib.isx_last_error() and name in lib.isx_last_error()
        assert entry(B=0) == 0                                                  # an empty problem is a no-op
        assert entry(fmap=None) == -1 and b"null" in lib.isx_last_error()
        assert entry(idx=None) == -1 and b"null" in lib.isx_last_error()
    assert fwd(rows=24) == -1 and fwd(shift=24) == -1 and fwd(n2=None) == -1 and fwd(shift=None, fmap=None) == -1
    assert bwd(g=24) == -1 and bwd(add=24) == -1 and bwd(dfmap=24) == -1 and b"16-B aligned" in lib.isx_last_error()
    assert bwd(cw=None) == -1 and bwd(dfmap=P[0]) == -1 and b"aliased" in lib.isx_last_error() and bwd(dfmap=P[1]) == -1 and bwd(dfmap=P[4]) == -1
    assert bwd(add_every=0) == -1 and b"bad shape" in lib.isx_last_error() and bwd(add_every=3) == -1 and bwd(add_every=2, fmap=None) == -1 and b"null" in lib.isx_last_error()
    # the LDS staging is checked in front of the pointers: a 57 x 57 map ((3249 x 5 + 12) x 4 = 65 028 bytes) passes it and is stopped at the NULL
    # pointer, a 58 x 58 map ((3364 x 5 + 12) x 4 = 67 328 bytes) does not fit 64 KB
    assert fwd(Hf=57, Wf=57, Wp=51, fmap=None) == -1 and b"null" in lib.isx_last_error()
    assert fwd(Hf=58, Wf=58, Wp=52, fmap=None) == -1 and b"LDS" in lib.isx_last_error()
    # backward: a 63 x 63 window of g ((3969 x 4 + 30) x 4 = 63 624 bytes) fits, 64 x 64 ((4096 x 4 + 30) x 4 = 65 656) does not
    assert bwd(Hf=64, Wf=64, kh=63, kw=63, Wp=2, fmap=None) == -1 and b"null" in lib.isx_last_error()
    assert bwd(Hf=64, Wf=64, kh=64, kw=64, Wp=1, fmap=None) == -1 and b"LDS" in lib.isx_last_error()


# ---- the step's two contracts, and what train.siamese_regions declares ---------------------------------------------------------------------------
def test_the_two_contract_classes():
    import torch.nn as nn
    from model.custom_modules import TripletLoss
    from model.siamese import DescriptorNet, RegionDescriptorNet, RegionHooks, TrunkHooks, TuneClassifSub
    from train.params import Params
    from utils.train_general import _Stepper
    assert issubclass(RegionDescriptorNet, RegionHooks) and not issubclass(RegionDescriptorNet, TrunkHooks)
    assert issubclass(DescriptorNet, TrunkHooks) and issubclass(TuneClassifSub, TrunkHooks) and not issubclass(DescriptorNet, RegionHooks)
    assert not issubclass(RegionHooks, TrunkHooks) and not issubclass(TrunkHooks, RegionHooks)
    for hook in ("trunk_precomputable", "precompute_trunk", "suffix_engine", "_tail_engine"):
        assert getattr(RegionHooks, hook) is getattr(TrunkHooks, hook)                 # one implementation, in the common base
    assert not hasattr(RegionHooks, "head_engine") and not hasattr(RegionHooks, "forward_features") and not hasattr(TrunkHooks, "region_head_engine")

    class Plain(nn.Module):                                                             # a plain module: no contract, no route, never asked
        def __init__(self):
            super().__init__()
            self.lin = nn.Linear(4, 4)

        def region_head_engine(self):
            raise AssertionError("a hook of a net outside the contracts was called")
        trunk_precomputable = precompute_trunk = suffix_engine = region_head_engine

    crit = TripletLoss(0.1, False, True)
    make_loss = lambda out, targets: (crit(*out), None)
    make_loss.region_triplet = (crit, nn.CrossEntropyLoss())
    P = Params(cuda_device=-1, train_batch_size=4, train_micro_batch=1, train_loss_avg=False)
    st = _Stepper(P, Plain(), lambda items, n: ([], []), make_loss)
    assert st.hooked is False and st.region is False and not st._prefix_ok(4) and st._region_engine() is None
    assert st._route([[0], [1]], 2, 1, ((torch.zeros(2, 3, 8, 8),) * 3, []), None) is None

    class OnCpu(RegionHooks):                                                           # in the contract, but nothing the engine takes: generic route
        def __init__(self):
            super().__init__()
            self.features = nn.Sequential(nn.Conv2d(3, 4, 1))

    st = _Stepper(P, OnCpu().train(), lambda items, n: ([], []), make_loss)
    assert st.hooked is False and st.region is True and st._region_engine() is None and not st._prefix_ok(4)
    assert st._route([[0], [1]], 2, 1, None, None) is None


def test_create_batch_builds_n_items_and_the_declarations_are_there(monkeypatch):
    import torch.nn as nn
    from model.custom_modules import TripletLoss
    from train import siamese_regions as sr
    from utils.dataset import synthetic_image_set
    tr = synthetic_image_set(8, 2, size=(3, 32, 32), seed=1)
    got = {}

    def fake_train_gen(train_type, P, test_print, test_net, net, train_set, testset_tuple, optimizer, create_epoch, create_batch, create_loss, best_score=0):
        got.update(create_batch=create_batch, create_loss=create_loss, couples=train_set)
        return best_score

    monkeypatch.setattr(sr, "train_gen", fake_train_gen)
    saved, saved_labels = dict(sr.P.__dict__), list(sr.labels)
    try:
        sr.P.cuda_device, sr.P.train_pre_proc = -1, True
        sr.labels[:] = sorted(set(l for _, l, _ in tr))
        crit, crit2 = TripletLoss(0.1, True), nn.CrossEntropyLoss()
        for one_shape in (True, False):
            sr.train_siam_triplets_pos_couples(None, tr, (tr, tr), crit, crit2, None, one_shape=one_shape)
            cb, cl = got["create_batch"], got["create_loss"]
            assert cb.deterministic is True and cl.region_triplet == (crit, crit2)
            items = [c + (i % len(tr),) for i, c in enumerate(sr.shuffle_couples(got["couples"]))][:3]
            assert len(items) == 3
            xs, ys = cb(items, len(items), epoch=0)
            n = 3 if one_shape else 1
            assert [tuple(x.shape) for x in xs] == [(n, 3, 32, 32)] * 3 and tuple(ys[0].shape) == (n,) and ys[0].dtype == torch.int64
            for j in range(n):                                                            # item j of the stacks is what a call on item j alone builds
                x1, y1 = cb(items[j:j + 1], 1, epoch=0)
                assert all(torch.equal(a[j:j + 1], b) for a, b in zip(xs, x1)) and torch.equal(ys[0][j:j + 1], y1[0])
    finally:
        sr.P.__dict__.clear(); sr.P.__dict__.update(saved); sr.labels[:] = saved_labels
