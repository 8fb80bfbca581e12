"""The box-pool, region top-k, DBA, sharded average-precision and tree-sum kernels called through the C ABI on buffers the TEST owns
(tests/_guards.py), as tests/test_gpu_retrieval_guards.py does for the retrieval kernels: every output is a poisoned body between sentinel
guards, every operand sits between NaN (labels, indices, keys: impossible-value) guards, and every result equals a CPU restatement bit for bit
(the oracle, tests/_eval_model.py, the numpy side of utils/metrics.py, isx.dp.tree_sum).  Through isx.ops these kernels only ever write
torch.empty outputs of exactly the right size: a store past the last row of the last block, an element never written or an operand read past
its end passes there.

Guards: at least 1024 elements on each side, and at least one staged unit (a plane or PP planes of the NCHW box pool, an image of the
channels-last kernels, a row of the row kernels) -- every address a dead thread of the last block could reach.  Alignment: where the ABI
does not ask for any (the NCHW box pool, the tree sum, region top-k, DBA, the score rows of the average precision) one case also runs one ELEMENT
past the 256-byte boundary and must give the bits of the aligned run.

Also here, because they need the same buffers: the one rule for NaN class scores in both layouts against the oracle (include/isx.h), the
2048-positive boundary of the sort-free average precision, sharded and unsharded, and the refusals of these entry points (a non-zero code,
isx_last_error set, every output byte still poison, every guard intact)."""
import time

import numpy as np
import pytest
import torch

import _desc_model as dm
import _eval_model as model
import _guards as G
import oracle as O

pytestmark = pytest.mark.gpu

F = np.float32
EPS = 1e-10
AP_MAXP = 2048


def _lib():
    from isx._lib import lib
    return lib(), torch.cuda.current_stream().cuda_stream


def _ok(rc, what=""):
    assert rc == 0, (what, rc, _lib()[0].isx_last_error())


def _refused(rc, name, outs, ins=(), what=""):
    assert rc != 0, (name, what)
    err = _lib()[0].isx_last_error()
    assert err and name.encode() in err, (name, what, err)
    torch.cuda.synchronize()
    for r in ins:
        assert r.guards_intact(), (name, what)
    for r in outs:
        assert r.guards_intact() and r.unwritten() == r.n, (name, what, "a refused call wrote its output")


def out_i32(shape, guard=1024):
    return G.Region("i32", shape, guard)


def u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---- isx_boxpool_s1 ---------------------------------------------------------------------------------------------------------------------------------
def _boxpool_plan(H, W):
    """launcher of isx_boxpool_s1: planes per block of the LDS kernel, 0 = the direct kernel."""
    plane = H * W * 4
    return min(64, 48 * 1024 // plane) if plane <= 48 * 1024 else 0


def _boxpool_nchw(fmap, kh, kw, off=0):
    L, st = _lib()
    B, C, H, W = fmap.shape
    Ho, Wo = H - kh + 1, W - kw + 1
    pp = max(_boxpool_plan(H, W), 1)
    x = G.in_f32(fmap, max(1024, pp * H * W), off)
    y = G.out_f32((B, C, Ho, Wo), max(1024, pp * Ho * Wo), off)
    _ok(L.isx_boxpool_s1(x.ptr, B, C, H, W, kh, kw, y.ptr, st), (fmap.shape, kh, kw, off))
    G.assert_clean([y], [x], (fmap.shape, kh, kw, off))
    return y.host()


@pytest.mark.parametrize("B,C,H,W,kh,kw,pp,offsets", [
    (1, 3, 7, 7, 7, 7, 64, (0,)),                  # one partial block (3 planes of 64), a single output per plane
    (2, 67, 13, 11, 3, 2, 64, (0, 1)),             # PP = 64: a last block of 6 planes
    (1, 2, 96, 128, 5, 5, 1, (0,)),                # a plane of exactly 48 KiB: PP = 1
    (1, 2, 97, 128, 5, 5, 0, (0, 1)),              # just above: boxpool_s1_direct_kernel
    (1, 176, 97, 128, 3, 3, 0, (0,)),              # 2 106 720 outputs > 8192 * 256: the direct kernel's grid-stride loop
    (2, 5, 6, 9, 1, 1, 64, (0,)),                  # kh = kw = 1: the map itself
])
def test_boxpool_s1(B, C, H, W, kh, kw, pp, offsets):
    """Against the oracle's in-order window walk, bit for bit, the WHOLE output in every case (the largest: 2.1 M outputs, about 0.01 s of
    oracle; the time is printed)."""
    assert _boxpool_plan(H, W) == pp
    rng = np.random.default_rng(H * W + C)
    fmap = rng.standard_normal((B, C, H, W), dtype=F)
    t0 = time.perf_counter()
    want = O.boxpool_s1(fmap, kh, kw)
    print("oracle box pool %s: %.3f s on the CPU" % ((B, C, H, W, kh, kw), time.perf_counter() - t0))
    if pp == 0 and C == 176:
        assert want.size > 8192 * 256
    if (kh, kw) == (1, 1):
        G.assert_bits(want, fmap)
    for off in offsets:
        G.assert_bits(_boxpool_nchw(fmap, kh, kw, off), want, off)


# ---- isx_boxpool_s1_nhwc ------------------------------------------------------------------------------------------------------------------------------
def _slice(C, units):
    """The channel slice both channels-last box-pool launchers choose: the largest of 64, 32, ..., 4 that divides C and whose `units` pixels fit 64 KiB."""
    cs = 64
    while cs > 4 and (C % cs != 0 or units * cs * 4 > 64 * 1024):
        cs >>= 1
    return cs


@pytest.mark.parametrize("B,C,H,W,kh,kw,cs", [(1, 64, 14, 14, 7, 7, 64), (1, 64, 20, 20, 7, 7, 32), (3, 96, 7, 5, 3, 2, 32), (2, 36, 12, 13, 5, 4, 4)])
def test_boxpool_s1_nhwc(B, C, H, W, kh, kw, cs):
    """CS = 64; the LDS limit forcing two slices of 32; 32 by divisibility; 4; grid.y.  The oracle's values and the NCHW kernel's bits."""
    L, st = _lib()
    assert _slice(C, H * W) == cs
    rng = np.random.default_rng(H * W + C)
    fmap = rng.standard_normal((B, C, H, W), dtype=F)
    want = O.boxpool_s1(fmap, kh, kw)
    Ho, Wo = H - kh + 1, W - kw + 1
    x = G.in_f32(model.to_nhwc(fmap), max(1024, H * W * C))
    y = G.out_f32((B, Ho, Wo, C), max(1024, Ho * Wo * C))
    _ok(L.isx_boxpool_s1_nhwc(x.ptr, B, C, H, W, kh, kw, y.ptr, st))
    G.assert_clean([y], [x])
    G.assert_bits(y, model.to_nhwc(want))
    G.assert_bits(_boxpool_nchw(fmap, kh, kw), want)


# ---- isx_boxpool_s1_bwd_nhwc ------------------------------------------------------------------------------------------------------------------------------
def _boxpool_bwd(g, H, W, kh, kw):
    L, st = _lib()
    B, Ho, Wo, C = g.shape
    x = G.in_f32(g, max(1024, Ho * Wo * C))
    dx = G.out_f32((B, H, W, C), max(1024, H * W * C))
    _ok(L.isx_boxpool_s1_bwd_nhwc(x.ptr, B, C, H, W, kh, kw, dx.ptr, st), (g.shape, H, W, kh, kw))
    G.assert_clean([dx], [x], (g.shape, H, W, kh, kw))
    return dx.host()


@pytest.mark.parametrize("C", [4, 64, 96])
@pytest.mark.parametrize("H,W,kh,kw", [(7, 5, 3, 2), (6, 6, 6, 6), (5, 4, 1, 1)])
def test_boxpool_s1_bwd_nhwc(H, W, kh, kw, C):
    """Ho = Wo = 1 (one window covers everything), kh = kw = 1 (the gradient itself), a 3 x 2 window whose divisor 6 is no power of two; one, one
    and three channel slices.  Image b of a batch has the bits of the single-image call."""
    Ho, Wo = H - kh + 1, W - kw + 1
    assert C // _slice(C, Ho * Wo) == {4: 1, 64: 1, 96: 3}[C]
    rng = np.random.default_rng(100 * H + C)
    g = rng.standard_normal((3, Ho, Wo, C), dtype=F)
    want = model.boxpool_bwd_canonical(g, H, W, kh, kw)
    G.assert_bits(_boxpool_bwd(g, H, W, kh, kw), want)
    if (kh, kw) == (1, 1):
        G.assert_bits(want, g)
    for b in range(3):
        G.assert_bits(_boxpool_bwd(g[b:b + 1], H, W, kh, kw), want[b:b + 1], b)


# ---- isx_region_topk / isx_region_topk_nhwc -------------------------------------------------------------------------------------------------------------
def _region_topk(cls, k, layout, off=0):
    L, st = _lib()
    B, K, Hp, Wp = cls.shape
    x = G.in_f32(np.array(cls) if layout == "nchw" else model.to_nhwc(cls), max(1024, K * Hp * Wp), off)
    idx, sc = G.out_i64((B, k), max(1024, k), off), G.out_f32((B, k), max(1024, k), off)
    fn = L.isx_region_topk if layout == "nchw" else L.isx_region_topk_nhwc
    _ok(fn(x.ptr, B, K, Hp, Wp, k, idx.ptr, sc.ptr, st), (cls.shape, k, layout, off))
    G.assert_clean([idx, sc], [x], (cls.shape, k, layout, off))
    return idx.host(), sc.host()


def _check_topk(cls, k, offsets=(0,)):
    want_i, want_s = model.oracle_region_topk(cls, k)
    mi, ms = model.region_topk(cls, k)
    np.testing.assert_array_equal(mi, want_i)
    G.assert_bits(ms, want_s, "the model against the oracle")
    for off in offsets:
        for layout in ("nchw", "nhwc"):
            gi, gs = _region_topk(cls, k, layout, off)
            np.testing.assert_array_equal(gi, want_i, err_msg=str((layout, off)))
            G.assert_bits(gs, want_s, (layout, off))
    return want_i, want_s


@pytest.mark.parametrize("B,K,Hp,Wp,k", [
    (2, 5, 1, 1, 6),                               # P = 1: PP2 = 2, one padding key, a tail of (-1, -inf)
    (2, 9, 1, 3, 3),                               # P = 3 padded to 4
    (2, 2, 64, 64, 10),                            # P = 4096, the maximum: 32 KiB of keys
    (2, 7, 5, 3, 300),                             # k > 256: more than one output per thread, a padded tail
    (2, 3, 40, 25, 600),
    (3, 17, 8, 6, 7),                              # grid.x = 3
])
def test_region_topk(B, K, Hp, Wp, k):
    """Scores in quarters (the index tie-break decides); the last image is ONE value (the order is the index order); image 0 holds +-inf, +-0
    and denormals at class 0 and at the last class.  Both layouts against the oracle: index bits and score bits, hence against each other."""
    cls = model.topk_case(B, K, Hp, Wp, True)
    P = Hp * Wp
    want_i, want_s = _check_topk(cls, k, (0, 1))
    n = min(k, P)
    assert want_i[B - 1, :n].tolist() == list(range(n)) and (want_i[:, n:] == -1).all() and np.isneginf(want_s[:, n:]).all()
    assert not np.signbit(want_s[want_s == 0]).any()                    # a zero maximum is emitted as +0


@pytest.mark.parametrize("K,Hp,Wp", [(5, 3, 4), (130, 4, 5)])
def test_nan_class_scores_follow_one_rule(K, Hp, Wp):
    """include/isx.h: a NaN in ANY class (class 0, a middle class, the last class, either sign, any payload, every class) makes the location's
    maximum 0x7FC00000; it ranks first, ties by the index; the emitted score is that NaN.  K = 130: a NaN in a lane's second and third round
    of the channels-last wave.  Both layouts and the oracle: the same index bits and score bits; the image without a NaN is not touched."""
    L, st = _lib()
    cls = model.nan_case(K, Hp, Wp)
    P = Hp * Wp
    for k in (3, P - 1, P + 4):
        want_i, want_s = _check_topk(cls, k)
        assert want_i[0, :3].tolist() == [2, 4, 7] and (G.bits(want_s[0, :3]) == 0x7FC00000).all()
        assert want_i[1, :3].tolist() == [0, 1, 2] and (G.bits(want_s[1, :min(k, P - 1)]) == 0x7FC00000).all()
        assert not np.isnan(want_s[2]).any()
    want_loc = np.stack([O.best_location_desc(cls[b])[1] for b in range(3)])
    np.testing.assert_array_equal(model.best_location(cls), want_loc)
    for layout in ("nchw", "nhwc"):
        x = G.in_f32(np.array(cls) if layout == "nchw" else model.to_nhwc(cls), max(1024, K * P))
        desc, loc = G.out_f32((3, K), max(1024, K)), G.out_i64((3, 2), 1024)
        fn = L.isx_best_location_desc if layout == "nchw" else L.isx_best_location_desc_nhwc
        _ok(fn(x.ptr, 3, K, Hp, Wp, EPS, desc.ptr, loc.ptr, st), layout)
        G.assert_clean([desc, loc], [x], layout)
        np.testing.assert_array_equal(loc.host(), want_loc, err_msg=layout)
        d = desc.host()
        assert np.isnan(d[:2]).all(), layout                             # the chosen locations hold a NaN: so does their descriptor
        G.assert_bits(d[2:], dm.best_location_desc(cls[2:])[0], layout)


# ---- isx_dba_groups ---------------------------------------------------------------------------------------------------------------------------------------
def _dba_data(D, sizes, seed, extras=True):
    """Unit rows in groups of `sizes`, the items of the groups interleaved; extras: a group of three rows scaled to 1e-6 (the 1e-10 on the norm
    is 30 ulp there, and nothing at a norm of 1) and a group of three all-zero rows."""
    rng = np.random.default_rng(seed)
    labels = np.concatenate([np.full(s, g, np.int32) for g, s in enumerate(sizes)] + ([np.full(3, 100, np.int32), np.full(3, 101, np.int32)] if extras else []))
    labels = labels[rng.permutation(len(labels))]
    E = rng.standard_normal((len(labels), D)).astype(F)
    E /= np.linalg.norm(E, axis=1, keepdims=True)
    E[labels == 100] *= F(1e-6)
    E[labels == 101] = 0
    return E, labels


def _dba(E, labels, k, off=0):
    L, st = _lib()
    N, D = E.shape
    order, begin, size, mg = model.dba_groups_of(labels)
    ins = [G.in_f32(E, max(1024, D), off), G.in_i32(order), G.in_i32(begin), G.in_i32(size)]
    out = G.out_f32((N, D), max(1024, D), off)
    _ok(L.isx_dba_groups(ins[0].ptr, N, D, ins[1].ptr, ins[2].ptr, ins[3].ptr, mg, k, out.ptr, st), (E.shape, k, off))
    G.assert_clean([out], ins, (E.shape, k, off))
    return out.host()


@pytest.mark.parametrize("D,sizes,offsets", [
    (9, (1, 2, 3, 5), (0, 1)),                     # the scalar score path, e_lds padded to 12 floats in front of the keys
    (64, (1, 2, 3, 5), (0, 1)),                    # aligned: the vec4 path; one float off: the scalar path, the same bits
    (1000, (1, 2, 3, 5), (0,)),                    # four d per thread in the norm
])
def test_dba_groups_small(D, sizes, offsets):
    E, labels = _dba_data(D, sizes, D)
    want = model.dba_chain(E, labels, -1)
    G.assert_bits(want[labels == 0], E[labels == 0])                     # the singleton: kept
    assert not want[labels == 101].any() and not np.signbit(want[labels == 101]).any()      # all-zero rows: every score ties, 0 / 1e-10 = +0
    for off in offsets:
        G.assert_bits(_dba(E, labels, -1, off), want, off)


def test_dba_groups_above_256_members():
    """Groups of 256, 257 and 1024: n2 = 256 / 512 / 1024, up to four members per thread in the score and sort loops, 1023 neighbours."""
    E, labels = _dba_data(16, (256, 257, 1024), 3, extras=False)
    G.assert_bits(_dba(E, labels, -1), model.dba_chain(E, labels, -1))
    G.assert_bits(_dba(E, labels, 300), model.dba_chain(E, labels, 300))


def test_dba_groups_raised_lds_limit():
    """D = 16384 with a group of 3: 65 584 B of dynamic LDS, above the 48 KiB default, so the launcher raises the kernel's limit -- which then
    STAYS raised: a small launch follows."""
    E, labels = _dba_data(16384, (1, 3), 16384, extras=False)
    G.assert_bits(_dba(E, labels, -1), model.dba_chain(E, labels, -1))
    E, labels = _dba_data(9, (1, 2, 3, 5), 9)
    G.assert_bits(_dba(E, labels, -1), model.dba_chain(E, labels, -1))


def test_dba_groups_every_k():
    """One group of 5: k = -1 (all four), 0 (unchanged), 1, 2, n - 1, n, n + 5."""
    E, labels = _dba_data(33, (5,), 33, extras=False)
    for k in (-1, 0, 1, 2, 4, 5, 10):
        want = model.dba_chain(E, labels, k)
        G.assert_bits(_dba(E, labels, k), want, k)
        if k == 0:
            G.assert_bits(want, E)
        if k in (4, 5, 10):
            G.assert_bits(want, model.dba_chain(E, labels, -1), k)


def test_dba_groups_ties_go_to_the_lower_item():
    """Rows 1 and 3 are identical; rows 4 and 5 differ only where row 0 is zero, so they tie as neighbours of row 0 and the order in which
    they enter its weighted sum shows in the result: the lower item index first."""
    rng = np.random.default_rng(12)
    E = rng.standard_normal((6, 24)).astype(F)
    E[3] = E[1]
    E[0, :2] = 0
    E[5] = E[4]
    E[5, :2] = E[4, 1::-1] * F(3)
    labels = np.zeros(6, np.int32)
    want = model.dba_chain(E, labels, 2)
    G.assert_bits(_dba(E, labels, 2), want)
    G.assert_bits(_dba(E, labels, -1), model.dba_chain(E, labels, -1))
    s = O.cosine_sim(E[:1], E)[0]
    assert s[4] == s[5]


# ---- isx_ap_shard_positives / isx_ap_shard_hist / isx_ap_from_hist -----------------------------------------------------------------------------------------
def _positives(sim, idx_base, ql, gl, cap, off=0):
    L, st = _lib()
    M, N = sim.shape
    ins = [G.in_f32(np.array(sim), max(1024, N), off), G.in_i32(np.array(ql)), G.in_i32(np.array(gl), max(1024, N))]
    keys, count = G.out_i64((M, cap), max(1024, cap)), out_i32((M,))
    _ok(L.isx_ap_shard_positives(ins[0].ptr, M, N, idx_base, ins[1].ptr, ins[2].ptr, cap, keys.ptr, count.ptr, st), (sim.shape, idx_base, cap, off))
    G.assert_clean([keys, count], ins, (sim.shape, idx_base, cap, off))
    return u64(keys.host()), count.host()


def _hist(sim, idx_base, keys_all, off=0):
    L, st = _lib()
    M, N = sim.shape
    W = keys_all.shape[1]
    ins = [G.in_f32(np.array(sim), max(1024, N), off), G.in_i64(np.ascontiguousarray(keys_all).view(np.int64), max(1024, W))]
    hist = out_i32((M, AP_MAXP), AP_MAXP)
    _ok(L.isx_ap_shard_hist(ins[0].ptr, M, N, idx_base, ins[1].ptr, W, hist.ptr, st), (sim.shape, idx_base, W, off))
    G.assert_clean([hist], ins, (sim.shape, idx_base, W, off))                      # all M x 2048 entries written
    return hist.host()


def _from_hist(hist, n_lab, kth):
    L, st = _lib()
    M, ld = hist.shape
    ins = [G.in_i32(hist, max(1024, ld)), G.in_i32(n_lab)]
    ap = G.out_f64((M,), 1024)
    _ok(L.isx_ap_from_hist(ins[0].ptr, ld, ins[1].ptr, M, kth, ap.ptr, st), (hist.shape, kth))
    G.assert_clean([ap], ins, (hist.shape, kth))
    return ap.host()


def _same_ap(got, want, what=""):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=str(what))
    ok = ~np.isnan(want)
    G.assert_bits(got[ok], want[ok], what)


def _cpu_hist(sim, idx_base, keys_all):
    from utils import metrics
    return metrics.ap_shard_hist(torch.from_numpy(np.ascontiguousarray(sim)), idx_base, torch.from_numpy(np.ascontiguousarray(keys_all).view(np.int64))).numpy()


@pytest.mark.parametrize("case", ["nonfinite", "boundary"])
def test_sharded_ap_steps_and_chain(case):
    """Each step on the GPU against the same step of the CPU restatement (keys as sorted sets per row, counts and histograms exactly), and the
    chain against the oracle's full ranking and ops.average_precision_sim on the whole matrix, as uint64 bits.  The shards include an empty
    one, one of a single row, and bases off the 16-byte grid (1001, 1002, 4103)."""
    from isx import ops
    sim, ql, gl = model.nonfinite_case() if case == "nonfinite" else model.boundary_case()
    bounds = model.NONFINITE_BOUNDS if case == "nonfinite" else model.BOUNDARY_BOUNDS
    M = sim.shape[0]
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    for kth in (1, 2):
        want = model.oracle_ap(sim, ql, gl, kth)
        cpu_ap, cpu_pos, cpu_keys_all, cpu_hists, cpu_n_lab = model.sharded_ap_cpu(sim, ql, gl, bounds, kth, steps=True)
        pos = [_positives(sim[:, a:b], a, ql, gl[a:b], AP_MAXP) for a, b in bounds]
        for (k, c), (ck, cc), ab in zip(pos, cpu_pos, bounds):
            np.testing.assert_array_equal(c, cc, err_msg=str(ab))
            np.testing.assert_array_equal(np.sort(k, axis=1), np.sort(ck, axis=1), err_msg=str(ab))
        cap = model.shard_caps([c for _, c in pos])
        keys_all = np.ascontiguousarray(np.concatenate([k[:, :cap] for k, _ in pos], 1))
        # the slots a shard filled are its first count[row] ones, in any order: the cut at `cap` keeps them all
        np.testing.assert_array_equal(np.sort(keys_all, axis=1), np.sort(cpu_keys_all, axis=1))
        n_lab = sum(c for _, c in pos).astype(np.int32)
        hists = [_hist(sim[:, a:b], a, keys_all) for a, b in bounds]
        for h, ch, ab in zip(hists, cpu_hists, bounds):
            np.testing.assert_array_equal(h, ch, err_msg=str(ab))
        ld = max(1, min(int(n_lab.max()), AP_MAXP))
        got = _from_hist(np.ascontiguousarray(sum(hists)[:, :ld]), n_lab, kth)
        _same_ap(got, cpu_ap, (case, kth))
        whole = ops.average_precision_sim(dev(sim), dev(ql), dev(gl), kth).cpu().numpy()
        _same_ap(whole, want, (case, kth, "ops.average_precision_sim"))              # 2049 positives: through the sorted fallback
        if case == "boundary":
            assert n_lab.tolist() == [2047, 2048, 2049, 0]
            G.assert_bits(got[:2], want[:2], kth)
            assert got[2] == -1.0 and np.isnan(got[3]) and want[2] > 0 and np.isnan(want[3])
            assert not hists[0][2].any() and not hists[1][2].any() and not hists[2][2].any()     # 2049 gathered keys: all-zero histograms
        else:
            _same_ap(got, want, (case, kth))


def test_ap_shard_positives_cap_and_empty_rows():
    """cap = 4 on a row with 9 positives: exactly four of ITS keys, count = 9, nothing past the row's four slots; a row without positives: all
    its slots zero (the poison shows a slot left alone).  idx_base = 1001 is off the 16-byte grid; an empty shard gives zeros."""
    rng = np.random.default_rng(4)
    N, base = 40, 1001
    sim = rng.standard_normal((3, N), dtype=F)
    gl = np.full(N, 7, np.int32)
    where = rng.choice(N, 9, replace=False)
    gl[where] = 0
    ql = np.array([0, 5, 7], np.int32)
    valid = set(model.rank_keys(sim[0, where], base + where).tolist())
    for off in (0, 1):
        keys, count = _positives(sim, base, ql, gl, 4, off)
        assert count.tolist() == [9, 0, N - 9]
        assert len(set(keys[0].tolist())) == 4 and set(keys[0].tolist()) <= valid
        assert not keys[1].any()
        assert (keys[2] != 0).all()
    keys, count = _positives(sim, base, ql, gl, AP_MAXP)
    assert sorted(keys[0][keys[0] != 0].tolist()) == sorted(valid) and int((keys[2] != 0).sum()) == N - 9 and not keys[1].any()
    keys, count = _positives(sim[:, :0], base, ql, gl[:0], 8)
    assert not keys.any() and not count.any()


@pytest.mark.parametrize("M,N,W,npos", [(3, 64, 1, (1, 0, 1)), (3, 2000, 300, (137, 300, 1)), (3, 6200, 8 * AP_MAXP, (2048, 2049, 5))])
def test_ap_shard_hist_widths(M, N, W, npos):
    """W = 1, 300 and 8 x 2048 gathered slots with the keys scattered among empty ones; scores in halves, so many gallery scores TIE with the
    smallest positive (the float pre-reject of the vector launch must keep them); a row with 2049 keys gives an all-zero histogram, the row
    with 2048 next to it a full one.  The vector launch (base 0, aligned) and the scalar launches (the row pointer one float off; a base of 2 with
    the same scores, i.e. other keys) against the CPU histograms."""
    rng = np.random.default_rng(W)
    sim = (np.round(rng.standard_normal((M, N)) * 2) / 2).astype(F)
    where = [rng.choice(N, n, replace=False) for n in npos]
    for r, j in enumerate(where):
        if len(j) == 1:                                      # a single positive: the three scores that share its 16 bytes tie with it
            sim[r, j[0] // 4 * 4:j[0] // 4 * 4 + 4] = sim[r, j[0]]
    for base in (0, 2):
        keys_all = np.zeros((M, W), np.uint64)
        for r, j in enumerate(where):
            keys_all[r, rng.choice(W, len(j), replace=False)] = model.rank_keys(sim[r, j], base + j)
        want = _cpu_hist(sim, base, keys_all)
        for r, n in enumerate(npos):
            assert int(want[r].sum()) > 0 if 0 < n <= AP_MAXP else not want[r].any()
        for off in ((0, 1) if base == 0 else (0,)):
            np.testing.assert_array_equal(_hist(sim, base, keys_all, off), want, err_msg=str((base, off)))


def test_ap_shard_hist_vector_and_scalar_launch_on_non_finite_scores():
    """Columns 1000 .. 2999 of the non-finite case as one shard at base 1000 (the vector launch) and columns 1001 .. 3000 at base 1001 (N % 4 == 0
    but the base is not a multiple of 4: the scalar launch) against the keys of the whole gallery."""
    sim, ql, gl = model.nonfinite_case()
    _, _, keys_all, _, _ = model.sharded_ap_cpu(sim, ql, gl, model.NONFINITE_BOUNDS, 1, steps=True)
    for a, b in ((1000, 3000), (1001, 3001)):
        s = np.ascontiguousarray(sim[:, a:b])
        want = _cpu_hist(s, a, keys_all)
        for off in (0, 1):
            np.testing.assert_array_equal(_hist(s, a, keys_all, off), want, err_msg=str((a, off)))


@pytest.mark.parametrize("M", [1, 64, 65])
def test_ap_from_hist(M):
    """One block of 64 threads, exactly full, and a second block of one row; ld = 40 below some rows' n_lab (-1), rows without a (remaining)
    positive (NaN), rows whose best positive has rank 0 (the first term), kth = 1, 2, 3."""
    from utils import metrics
    rng = np.random.default_rng(65)
    ld = 40
    n_lab = rng.integers(0, 46, 65).astype(np.int32)
    n_lab[:6] = [3, 0, 41, 40, 1, 2]
    hist = np.zeros((65, ld), np.int32)
    for r in range(65):
        n = min(int(n_lab[r]), ld)
        hist[r, :n] = 1 + rng.integers(0, 4, n) * rng.integers(0, 2, n)             # every positive sits in its own bucket
    hist[::2, 0] = 1                                                                # rank 0 is a positive
    hist, n_lab = hist[:M].copy(), n_lab[:M].copy()
    for kth in (1, 2, 3):
        want = metrics.ap_from_hist(torch.from_numpy(hist), torch.from_numpy(n_lab), kth).numpy()
        got = _from_hist(hist, n_lab, kth)
        _same_ap(got, want, (M, kth))
        if M == 65:
            assert want[2] == -1.0 and np.isnan(want[1]) and (want[[0, 3]] > 0).all() and np.isnan(want[4]) == (kth > 1)


def test_average_precision_sim_at_the_2048_positive_boundary():
    """isx_average_precision_sim on the queries with 2047 / 2048 / 2049 / 0 positives: the oracle's bits, the oracle's bits, -1.0 (over the
    limit: the caller's sorted fallback), NaN.  N = 6200: the float4 instance on the boundary, the scalar one a float off it."""
    L, st = _lib()
    assert L.isx_ap_shard_max_positives() == AP_MAXP == model.AP_MAXP             # one limit for the sharded and the unsharded kernels
    sim, ql, gl = model.boundary_case()
    M, N = sim.shape
    for kth in (1, 2):
        want = model.oracle_ap(sim, ql, gl, kth)
        for osim, olab in ((0, 0), (1, 0), (0, 1)):
            ins = [G.in_f32(np.array(sim), N, osim), G.in_i32(np.array(ql)), G.in_i32(np.array(gl), N, olab)]
            ap = G.out_f64((M,), 1024)
            _ok(L.isx_average_precision_sim(ins[0].ptr, M, N, ins[1].ptr, ins[2].ptr, kth, ap.ptr, st), (kth, osim, olab))
            G.assert_clean([ap], ins, (kth, osim, olab))
            got = ap.host()
            G.assert_bits(got[:2], want[:2], (kth, osim, olab))
            assert got[2] == -1.0 and np.isnan(got[3]) and want[2] > 0 and np.isnan(want[3])


# ---- isx_tree_sum_rows ------------------------------------------------------------------------------------------------------------------------------------
def _tree_ref(rows):
    from isx import dp
    t = torch.from_numpy(np.ascontiguousarray(rows))
    return dp.tree_sum(0, t.shape[0], lambda i: t[i].clone()).numpy()


def _tree_rows(L, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((L, n)) * 10.0 ** rng.integers(-3, 4, (L, n))).astype(F)          # magnitudes apart: the order of the adds shows


def _tree_sum(rows, n, off=0, guard=None):
    """rows: (L, stride) with stride >= n."""
    L, st = _lib()
    Lr, stride = rows.shape
    x = G.in_f32(rows, guard or max(1024, stride), off)
    y = G.out_f32((n,), guard or max(1024, n), off)
    _ok(L.isx_tree_sum_rows(x.ptr, Lr, stride, n, y.ptr, st), (rows.shape, n, off))
    G.assert_clean([y], [x], (rows.shape, n, off))
    return y.host()


@pytest.mark.parametrize("n", [1, 7, 1024, 1027])
def test_tree_sum_rows(n):
    """L = 1 .. 16 (every instantiation); n = 1024: the float4 launch, the others the scalar one."""
    for Lr in range(1, 17):
        rows = _tree_rows(Lr, n, 100 * Lr + n)
        G.assert_bits(_tree_sum(rows, n), _tree_ref(rows), (Lr, n))


def test_tree_sum_rows_strides_alignment_and_in_place():
    L, st = _lib()
    rows = _tree_rows(5, 1024, 5)
    want = _tree_ref(rows)
    G.assert_bits(_tree_sum(rows, 1024, 1), want, "one float off the boundary: the scalar launch")
    wide = np.full((5, 1027), np.nan, F)                                             # a stride that is no multiple of 4: the scalar launch
    wide[:, :1024] = rows
    G.assert_bits(_tree_sum(wide, 1024), want, "stride 1027")
    wide = np.full((5, 1028), np.nan, F)                                             # a multiple of 4: the float4 launch with stride > n
    wide[:, :1024] = rows
    G.assert_bits(_tree_sum(wide, 1024), want, "stride 1028")
    for n in (1024, 1027):                                                          # in place, out = rows[0]: the guards around the WHOLE allocation
        rows = _tree_rows(7, n, n)
        io = G.in_f32_io(rows, 2048)
        _ok(L.isx_tree_sum_rows(io.ptr, 7, n, n, io.ptr, st), ("in place", n))
        assert io.guards_intact(), n
        got = io.host()
        G.assert_bits(got[0], _tree_ref(rows), ("in place", n))
        G.assert_bits(got[1:], rows[1:], ("in place: the other rows", n))


@pytest.mark.parametrize("L_,n", [(2, 8192 * 256 * 4 + 4), (3, 8192 * 256 + 1)])
def test_tree_sum_rows_grid_stride_tail(L_, n):
    """One item more than 8192 blocks of 256 threads cover in one pass: float4 items (L = 2), scalar items (L = 3, n odd)."""
    rows = _tree_rows(L_, n, n % 1000)
    got = _tree_sum(rows, n, guard=4096)
    G.assert_bits(got, _tree_ref(rows))


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    L, st = _lib()
    # isx_region_topk: Hp * Wp = 4097
    cls = G.in_f32(np.zeros((1, 1, 17, 241), F))
    idx, sc = G.out_i64((1, 4), 1024), G.out_f32((1, 4), 1024)
    _refused(L.isx_region_topk(cls.ptr, 1, 1, 17, 241, 4, idx.ptr, sc.ptr, st), "isx_region_topk", [idx, sc], [cls])
    _refused(L.isx_region_topk_nhwc(cls.ptr, 1, 1, 17, 241, 4, idx.ptr, sc.ptr, st), "isx_region_topk_nhwc", [idx, sc], [cls])
    # isx_boxpool_s1_nhwc: four channels of a 65 x 64 map exceed 64 KiB; a pointer that is only 4-byte aligned
    x = G.in_f32(np.zeros((1, 65, 64, 4), F))
    y = G.out_f32((1, 64, 63, 4), 1024)
    _refused(L.isx_boxpool_s1_nhwc(x.ptr, 1, 4, 65, 64, 2, 2, y.ptr, st), "isx_boxpool_s1_nhwc", [y], [x], "65 x 64")
    x1, y1 = G.in_f32(np.zeros((1, 6, 6, 4), F), 1024, 1), G.out_f32((1, 5, 5, 4), 1024, 1)
    y0 = G.out_f32((1, 5, 5, 4), 1024)
    _refused(L.isx_boxpool_s1_nhwc(x1.ptr, 1, 4, 6, 6, 2, 2, y0.ptr, st), "isx_boxpool_s1_nhwc", [y0], [x1], "fmap off the boundary")
    x0 = G.in_f32(np.zeros((1, 6, 6, 4), F))
    _refused(L.isx_boxpool_s1_nhwc(x0.ptr, 1, 4, 6, 6, 2, 2, y1.ptr, st), "isx_boxpool_s1_nhwc", [y1], [x0], "out off the boundary")
    # isx_dba_groups: an instance above 1024 items; out == emb
    E, labels = _dba_data(9, (1, 2, 3), 1, extras=False)
    order, begin, size, mg = model.dba_groups_of(labels)
    ins = [G.in_f32_io(E, 1024), G.in_i32(order), G.in_i32(begin), G.in_i32(size)]
    out = G.out_f32(E.shape, 1024)
    _refused(L.isx_dba_groups(ins[0].ptr, 6, 9, ins[1].ptr, ins[2].ptr, ins[3].ptr, 1025, -1, out.ptr, st), "isx_dba_groups", [out], ins, "max_group")
    _refused(L.isx_dba_groups(ins[0].ptr, 6, 9, ins[1].ptr, ins[2].ptr, ins[3].ptr, mg, -1, ins[0].ptr, st), "isx_dba_groups", [out], ins, "out == emb")
    G.assert_bits(ins[0], E, "a refused in-place call changed emb")
    # isx_ap_shard_positives: cap 0, cap 2049, a global index above 2^32 - 1
    sim, ql, gl = G.in_f32(np.zeros((2, 8), F)), G.in_i32(np.zeros(2, np.int32)), G.in_i32(np.zeros(8, np.int32))
    keys, count = G.out_i64((2, 2049), 2049), out_i32((2,))
    for cap, base in ((0, 0), (2049, 0), (4, (1 << 32) - 8)):
        _refused(L.isx_ap_shard_positives(sim.ptr, 2, 8, base, ql.ptr, gl.ptr, cap, keys.ptr, count.ptr, st), "isx_ap_shard_positives", [keys, count],
                 [sim, ql, gl], (cap, base))
    # isx_ap_shard_hist: no gathered slot
    hist = out_i32((2, AP_MAXP), AP_MAXP)
    ka = G.in_i64(np.zeros((2, 4), np.int64))
    _refused(L.isx_ap_shard_hist(sim.ptr, 2, 8, 0, ka.ptr, 0, hist.ptr, st), "isx_ap_shard_hist", [hist], [sim, ka])
    # isx_tree_sum_rows: 17 rows; rows that overlap
    rows = G.in_f32(np.zeros((17, 8), F))
    o = G.out_f32((8,), 1024)
    _refused(L.isx_tree_sum_rows(rows.ptr, 17, 8, 8, o.ptr, st), "isx_tree_sum_rows", [o], [rows], "L = 17")
    _refused(L.isx_tree_sum_rows(rows.ptr, 2, 7, 8, o.ptr, st), "isx_tree_sum_rows", [o], [rows], "stride < n")
