"""tests/_eval_model.py, the CPU restatements tests/test_gpu_eval_guards.py pins the DBA, class-max / region top-k, box-pool backward and
sharded average-precision kernels to, checked on their own (no GPU):

  * dba_chain against the oracle inside the tolerance the project already holds the kernel to, against the reference's own fixture, and against
    the wrong variants a bit-exact GPU comparison has to tell apart (on shapes of the GPU test);
  * class_max / region_topk / best_location against the oracle, NaN class scores included: index bits and score bits;
  * boxpool_bwd_canonical against float64 autograd, and against the variant that divides inside the loop;
  * the sharded average precision of utils/metrics.py on CPU tensors against the oracle's full ranking, as uint64 bits, with non-finite scores
    and at the 2048-positive boundary."""
import os

import numpy as np
import pytest
import torch

import _eval_model as model
import oracle as O

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- dba_chain ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,L,k", [(300, 64, 40, -1), (300, 64, 40, 3), (700, 2048, 5, -1), (257, 9, 1, 2), (1500, 32, 1, 4), (2600, 16, 2, -1), (400, 16384, 3, 2)])
def test_dba_chain_within_the_kernels_tolerance_of_the_oracle(N, D, L, k):
    """The shapes and the tolerance of tests/test_gpu_dropin.py::test_instance_avg_groups_kernel_vs_oracle."""
    rng = np.random.default_rng(N + D)
    E = rng.standard_normal((N, D)).astype(F)
    E /= np.linalg.norm(E, axis=1, keepdims=True)
    labs = rng.integers(0, L, N).astype(np.int32)
    labs[0] = L + 7
    got = model.dba_chain(E, labs, k)
    np.testing.assert_allclose(got, O.dba(E, labs, k), rtol=2e-6, atol=2e-7)
    np.testing.assert_array_equal(_bits(got[0]), _bits(E[0]))


def test_dba_chain_reproduces_the_reference_fixture():
    g = np.load(os.path.join(GOLDEN, "dba.npz"))
    for key, k in (("kall", -1), ("k0", 0), ("k1", 1), ("k2", 2), ("k5", 5)):
        np.testing.assert_allclose(model.dba_chain(g["emb"], g["labels"], k), g[key], rtol=1e-5, atol=1e-6, err_msg=key)
    np.testing.assert_array_equal(_bits(model.dba_chain(g["emb"], g["labels"], 0)), _bits(g["emb"]))


def test_dba_chain_differs_from_its_wrong_variants():
    """D = 1000 (four d per thread, every wave busy) and D = 9 with groups of 1, 2, 3, 5: the model is not the variant without the 1e-10, with
    nn under the weights, or with the wave sums in reverse order -- in bits, so a bit-exact GPU comparison on this data catches each."""
    rng = np.random.default_rng(5)
    E = rng.standard_normal((11, 1000)).astype(F)
    labs = np.array([0, 1, 1, 2, 2, 2, 3, 3, 3, 3, 3], np.int32)
    base = model.dba_chain(E, labs, -1)
    assert (_bits(base) == _bits(model.dba_chain(E, labs, -1, eps_outside=False))).all()       # norms of about 40: 1e-10 is below half an ulp
    for name, kw in (("nn", dict(denominator_plus=0)), ("reverse", dict(reverse_waves=True))):
        other = model.dba_chain(E, labs, -1, **kw)
        n = int((_bits(base) != _bits(other)).sum())
        print("dba_chain vs %s: %d of %d elements differ" % (name, n, base.size))
        assert n > 0, name
    # the 1e-10 only shows where the norm is small: rows scaled to 1e-6 (norms of about 5e-5: 1e-10 is 2e-6 of that, some 30 ulp), or zero
    # (0 / 1e-10 = 0, where 0 / 0 is a NaN); the GPU test carries both kinds of row
    small = (E * F(1e-6)).astype(F)
    assert (_bits(model.dba_chain(small, labs, -1)) != _bits(model.dba_chain(small, labs, -1, eps_outside=False))).sum() > small.size // 2
    zero = np.zeros((3, 9), F)
    assert not model.dba_chain(zero, [0, 0, 0], -1).any() and np.isnan(model.dba_chain(zero, [0, 0, 0], -1, eps_outside=False)).all()


def test_dba_groups_of():
    order, begin, size, mx = model.dba_groups_of(np.array([5, 2, 5, 9, 2, 5]))
    assert order.tolist() == [1, 4, 0, 2, 5, 3] and mx == 3
    assert begin.tolist() == [2, 0, 2, 5, 0, 2] and size.tolist() == [3, 2, 3, 1, 2, 3]


# ---- class-max ----------------------------------------------------------------------------------------------------------------------------------------
_oracle_topk = model.oracle_region_topk


@pytest.mark.parametrize("K,Hp,Wp,k", [(5, 3, 4, 3), (5, 3, 4, 12), (9, 4, 5, 30), (3, 2, 6, 5)])
def test_nan_rule_model_and_oracle(K, Hp, Wp, k):
    cls = model.nan_case(K, Hp, Wp)
    want_i, want_s = _oracle_topk(cls, k)
    for layout, c in (("nchw", cls), ("nhwc", model.to_nhwc(cls))):
        idx, sc = model.region_topk(c, k, layout)
        np.testing.assert_array_equal(idx, want_i)
        np.testing.assert_array_equal(_bits(sc), _bits(want_s))
        np.testing.assert_array_equal(model.best_location(c, layout), np.stack([O.best_location_desc(cls[b])[1] for b in range(3)]))
    # what the rule says, spelled out on image 0: the NaN locations first, by index, each with the canonical NaN, then the +inf
    n = min(k, 5)
    assert want_i[0, :n].tolist() == [2, 4, 7, 9, 1][:n]
    assert (_bits(want_s[0, :min(k, 4)]) == 0x7FC00000).all()
    assert k < 5 or want_s[0, 4] == np.inf
    P = Hp * Wp
    nn = min(k, P - 1)
    assert want_i[1, :nn].tolist() == list(range(nn)) and (_bits(want_s[1, :nn]) == 0x7FC00000).all()      # more NaN locations than k
    assert not np.isnan(want_s[2, :min(k, P)]).any()
    first = min((2, 4, 7, 9), key=lambda p: (p % Wp) * Hp + p // Wp)                                       # the lowest column, then the lowest row
    assert model.best_location(cls)[0].tolist() == [first // Wp, first % Wp]


def test_best_location_ties_among_nan_locations_go_to_the_lowest_column():
    cls = np.zeros((1, 2, 3, 3), F)
    cls[0, 1, 0, 2] = np.nan                       # (row 0, col 2): flat 2
    cls[0, 0, 2, 1] = model.nan_f32(True, 7)       # (row 2, col 1): flat 7 -- the lower column wins, where the flat index would take (0, 2)
    assert model.best_location(cls)[0].tolist() == [2, 1]
    assert O.best_location_desc(cls[0])[1].tolist() == [2, 1]
    assert model.region_topk(cls, 2)[0][0].tolist() == [2, 7]


@pytest.mark.parametrize("shape,k", [((1, 5, 1, 1), 6), ((1, 9, 1, 3), 3), ((1, 7, 5, 3), 300), ((3, 17, 8, 6), 7)])
def test_region_topk_model_is_the_oracle_without_nan(shape, k):
    cls = model.topk_case(*shape, True)
    want_i, want_s = _oracle_topk(cls, k)
    for layout, c in (("nchw", cls), ("nhwc", model.to_nhwc(cls))):
        idx, sc = model.region_topk(c, k, layout)
        np.testing.assert_array_equal(idx, want_i)
        np.testing.assert_array_equal(_bits(sc), _bits(want_s))


# ---- box-pool backward -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,kh,kw", [(7, 5, 3, 2), (6, 6, 6, 6), (5, 4, 1, 1)])
def test_boxpool_bwd_canonical(H, W, kh, kw):
    rng = np.random.default_rng(H * W)
    g = rng.standard_normal((2, H - kh + 1, W - kw + 1, 4)).astype(F)
    got = model.boxpool_bwd_canonical(g, H, W, kh, kw)
    x = torch.zeros(2, 4, H, W, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.avg_pool2d(x, (kh, kw), 1).backward(torch.from_numpy(g).permute(0, 3, 1, 2).double())
    ref = x.grad.permute(0, 2, 3, 1).numpy()
    # at most kh kw adds of terms of one magnitude and one division: (kh kw + 1) 2^-24 of the sum of magnitudes
    bound = (kh * kw + 1) * 2.0 ** -24 * model.boxpool_bwd_canonical(np.abs(g), H, W, kh, kw).astype(np.float64)
    assert (np.abs(got - ref) <= bound).all()
    if kh * kw == 6:                                # 1 / 6 is not exact: dividing every term is another result
        assert (_bits(got) != _bits(model.boxpool_bwd_canonical(g, H, W, kh, kw, divide_inside=True))).any()


# ---- sharded average precision -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kth", [1, 2])
def test_sharded_ap_with_non_finite_scores(kth):
    sim, ql, gl = model.nonfinite_case()
    assert np.isnan(sim).sum() > 500 and (np.signbit(sim) & np.isnan(sim)).any() and (~np.signbit(sim) & np.isnan(sim)).any()
    want = model.oracle_ap(sim, ql, gl, kth)
    assert not np.isnan(want).any()
    got = model.sharded_ap_cpu(sim, ql, gl, model.NONFINITE_BOUNDS, kth)
    np.testing.assert_array_equal(_bits(got), _bits(want))
    np.testing.assert_array_equal(_bits(model.sharded_ap_cpu(sim, ql, gl, ((0, 3001),), kth)), _bits(want))


@pytest.mark.parametrize("kth", [1, 2])
def test_sharded_ap_at_the_2048_positive_boundary(kth):
    sim, ql, gl = model.boundary_case()
    assert [int((gl == q).sum()) for q in ql] == [2047, 2048, 2049, 0]
    want = model.oracle_ap(sim, ql, gl, kth)
    got, pos, keys_all, hists, n_lab = model.sharded_ap_cpu(sim, ql, gl, model.BOUNDARY_BOUNDS, kth, steps=True)
    np.testing.assert_array_equal(_bits(got[:2]), _bits(want[:2]))
    assert got[2] == -1.0 and np.isnan(got[3]) and np.isnan(want[3]) and want[2] > 0
    assert n_lab.tolist() == [2047, 2048, 2049, 0]
    assert int((keys_all[2] != 0).sum()) == 2049 and all(not h[2].any() for h in hists)        # over the limit: an all-zero histogram


def test_sharded_evaluation_refuses_a_query_above_the_limit():
    """test/_common.py dp_metrics_sharded: 11 positives give a mean AP, 2049 raise (the unsharded evaluation takes the sorted fallback there)."""
    from test._common import GalleryShard, dp_metrics_sharded
    N = 2060
    E = torch.nn.functional.normalize(torch.randn(N, 4, generator=torch.Generator().manual_seed(0)), dim=1)
    ref = [(None, "a" if i < 2049 else "b", None) for i in range(N)]
    queries = [(None, "b", None), (None, "a", None)]
    Q = E[[2055, 3]]
    m = dp_metrics_sharded(Q[:1], GalleryShard(E, 0, N), queries[:1], ref)
    assert len(m["aps"]) == 1 and 0.0 < m["aps"][0] <= 1.0 and m["mAP"] == m["aps"][0]
    with pytest.raises(NotImplementedError, match="2048 positives"):
        dp_metrics_sharded(Q, GalleryShard(E, 0, N), queries, ref)
