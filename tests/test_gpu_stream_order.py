"""Every launching entry of include/isx.h on a SIDE stream behind a late producer (tests/_streams.py), and the Python layer above them.

The guard and chain files launch on torch's current stream with nothing else in flight: the `isx_stream_t stream` argument carries no
information there.  Here every function of the header whose last parameter is `isx_stream_t stream` has a row in TABLE (or a reason in
NOT_HERE; test_every_stream_taking_entry_has_a_case parses the header): the entry is called on a fresh non-blocking stream while its operands do
not exist yet -- a launch that drops its stream, a stage of a multi-launch entry on another stream, a memset on the null stream or a hidden
synchronisation shows as wrong bits, a poisoned output or as "delay too short".  The data and the references are the guard and chain files'
own (oracle, _eval_model, _head_model, _desc_model, _suffix_model, _xent_model, _triplet_model, _region_train_model, _augment_model),
compared as they are compared there: bit for bit, and inside the documented bound where an entry has no bit-exact reference (the fp16
conversions' norm2 / gstats, isx_cosine_sim_f16, isx_masked_sums).  No new tolerance.

Multi-launch entries run at the smallest existing shape at which they really issue several launches; the case asserts it with the host
arithmetic of _guards.py where that is restated.

The second half runs wrappers of isx.ops, isx/suffix.py, isx/dp.py, isx/shard_head.py, train/_common.py and ShardedGallery.local_search the same
way under torch.cuda.stream(S), and checks the device buffers that the Python layer keeps between calls or hands out per call (head_linear's split-K workspace, ops._MEAN_STD,
ShardedGallery's workspace and fp16 gallery, slab._STAGE) for what happens when a second stream uses them."""
import math
import os
import re
import time
import types

import numpy as np
import pytest
import torch

import _desc_model as dm
import _eval_model as em
import _guards as G
import _head_model as hm
import _region_train_model as rm
import _streams as S
import _suffix_model as sm
import _triplet_model as tm
import _xent_model as xm
import oracle as O

F = np.float32
H16 = np.float16
EPS = dm.EPS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

# entries that take a stream and have no row in TABLE, each with its reason
NOT_HERE = {
    "isx_comm_allgather_rows": "a collective: tests/_rccl_worker.py alternates it between a side stream and the current stream on two or more GPUs",
    "isx_shard_topk_allgather": "a collective: tests/_rccl_worker.py alternates it between a side stream and the current stream on two or more GPUs",
    "isx_debug_fast_fallback_rows": "takes no stream and blocks the host by contract -- include/isx.h: 'Synchronises the device.' -- so it cannot return before a "
                                    "late producer; the fallback_rows case calls it after its stream has drained",
    "isx_debug_expf_logf": "a debug probe with no CPU reference of its own (it IS the reference of the cross-entropy cases here, which read expf and "
                           "logf through it on the default stream)",
}

TABLE = []                                         # (id, entry, builder of the Case)


def case(entry, tag=None, level="abi"):
    def deco(fn):
        TABLE.append(((entry[4:] if level == "abi" else "ops_" + entry) + ("_" + tag if tag else ""), entry, fn))
        return fn
    return deco


def _rng(*seed):
    return np.random.default_rng(list(seed))


def _normal(rng, *shape):
    return rng.standard_normal(shape, dtype=F)


def _nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def _nchw(a):
    return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))


def _rows_of(rows):
    return lambda y: y[torch.from_numpy(np.asarray(rows)).to(y.device)]


def _same_ap(got, want, a):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    G.assert_bits(got[ok], np.asarray(want)[ok])


def _lib():
    from isx._lib import lib
    return lib()


# ==== descriptor head ===============================================================================================================================
@case("isx_l2norm_rows")
def _():
    x, _ = dm.row_case(5, 260)
    return S.Case(dict(x=x), lambda L, p, st: L.isx_l2norm_rows(p.x, 5, 260, EPS, p.y, st), lambda a: dict(y=dm.l2norm_rows(a.x)), outs=dict(y=("f32", (5, 260))))


@case("isx_l2norm_shift_rows")
def _():
    x, shift = dm.row_case(5, 2052)                                          # the block kernel
    return S.Case(dict(x=x, shift=shift), lambda L, p, st: L.isx_l2norm_shift_rows(p.x, p.shift, 5, 2052, EPS, p.y, st),
                  lambda a: dict(y=dm.l2norm_rows(a.x, shift=a.shift)), outs=dict(y=("f32", (5, 2052))))


@case("isx_l2norm_rows_bwd")
def _():
    x, dy = dm.bwd_case(3, 1025)
    return S.Case(dict(x=x, dy=dy), lambda L, p, st: L.isx_l2norm_rows_bwd(p.x, p.dy, 3, 1025, EPS, p.dx, st),
                  lambda a: dict(dx=dm.l2norm_rows_bwd(a.x, a.dy)), outs=dict(dx=("f32", (3, 1025))))


def _gap(B, C, Hh, W, path):
    f = dm.map_case(B, C, Hh, W)
    assert dm.gap_plan(B, C, Hh * W)[0] == path                                # "fallback": the pooling kernel, then the row kernel -- two launches
    return S.Case(dict(f=f), lambda L, p, st: L.isx_gap_l2(p.f, B, C, Hh, W, EPS, p.y, st), lambda a: dict(y=dm.gap_l2(a.f)), outs=dict(y=("f32", (B, C))))


case("isx_gap_l2", "fused")(lambda: _gap(3, 24, 7, 7, "fused"))
case("isx_gap_l2", "two_launches")(lambda: _gap(1, 8, 40, 40, "fallback"))


def _gap_nhwc(C, HW, plan):
    f = dm.map_case(2, C, HW, 1)
    m = np.ascontiguousarray(f.reshape(2, C, HW).transpose(0, 2, 1))
    assert dm.gap_nhwc_plan(C) == plan                                        # "generic": pooling kernel + row kernel
    return S.Case(dict(f=m), lambda L, p, st: L.isx_gap_l2_nhwc(p.f, 2, C, HW, 1, EPS, p.y, st), lambda a: dict(y=dm.gap_l2_nhwc(a.f)),
                  outs=dict(y=("f32", (2, C))))


case("isx_gap_l2_nhwc", "float4")(lambda: _gap_nhwc(2048, 49, "qpt1"))
case("isx_gap_l2_nhwc", "two_launches")(lambda: _gap_nhwc(30, 49, "generic"))


@case("isx_bias_act_inplace")
def _():
    n, C = 64, 8
    rng = _rng(n, C)
    y0, b, r = _normal(rng, n), _normal(rng, C), _normal(rng, n)
    return S.Case(dict(y=y0, b=b, r=r), lambda L, p, st: L.isx_bias_act_inplace(p.y, p.b, p.r, n, C, 1, 1, st),
                  lambda a: dict(y=np.maximum((a.y + a.b[np.arange(n) % C]) + a.r, F(0))), io=("y",))


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


@case("isx_images_u8_to_f32")
def _():
    B, Hh, W = 2, 5, 7
    img = _rng(5).integers(0, 256, (B, Hh, W, 3), dtype=np.uint8)
    return S.Case(dict(img=img), lambda L, p, st: L.isx_images_u8_to_f32(p.img, B, Hh, W, *MEAN, *STD, 1, p.out, st),
                  lambda a: dict(out=_nhwc(O.images_u8_to_f32(a.img, MEAN, STD))), outs=dict(out=("f32", (B, Hh, W, 3))))


def _affine_inputs():
    import _augment_model as am
    import test_gpu_augment as ta
    fx = ta.fixture()
    rows = np.array([3, 1], np.int64)
    return am, ta, fx["img0"], rows, np.ascontiguousarray(fx["mat0"][rows], np.float64), ta.noise_ids(5)[rows]


def _affine_ref(am, seed, cl):
    def ref(a):
        u8 = np.stack([am.affine_noisy(a.img[a.rows[i]], a.mat[i], seed, a.ids[i])[0] for i in range(len(a.rows))])
        return dict(u8=u8, f32=am.normalise(u8, a.mean, a.std, cl))
    return ref


@case("isx_affine_noisy_u8")
def _():
    """W > 1: the column filter, the row filter and the warp -- three kernels through one workspace.  Zero matrices, rows and noise ids are valid:
    every output pixel reads input pixel (0, 0) of image 0."""
    am, ta, img, rows, mat, ids = _affine_inputs()
    N, Hh, W, _ = img.shape
    B = len(rows)
    assert W > 1
    need = _lib().isx_affine_noisy_workspace(B, Hh, W)
    return S.Case(dict(img=img, rows=rows, mat=mat, ids=ids, mean=np.array(MEAN, F), std=np.array(STD, F)),
                  lambda L, p, st: L.isx_affine_noisy_u8(p.img, p.rows, B, Hh, W, p.mat, ta.SEED, p.ids, p.mean, p.std, 1, p.u8, p.f32, p.ws, need, st),
                  _affine_ref(am, ta.SEED, True), outs=dict(u8=("u8", (B, Hh, W, 3)), f32=("f32", (B, Hh, W, 3))), ws=dict(ws=need), guard=dict(mat=64, ids=64, rows=64))


# ==== inference trunk ===============================================================================================================================
@case("isx_bias_relu_maxpool_nhwc")
def _():
    B, Hh, W, C = 2, 7, 9, 8
    rng = _rng(Hh, C)
    y, b = _normal(rng, B, Hh, W, C), _normal(rng, C)
    want = O.bias_relu_maxpool_nhwc(y, b)
    return S.Case(dict(y=y, b=b), lambda L, p, st: L.isx_bias_relu_maxpool_nhwc(p.y, p.b, B, Hh, W, C, p.out, st),
                  lambda a: dict(out=O.bias_relu_maxpool_nhwc(a.y, a.b)), outs=dict(out=("f32", want.shape)))


@case("isx_stem7x7_pool_nhwc")
def _():
    B, Hh, W = 1, 17, 12
    rng = _rng(Hh, W)
    x, w, b = _normal(rng, B, Hh, W, 3), _normal(rng, 64, 7, 7, 3) * F(147 ** -0.5), _normal(rng, 64)
    want = O.stem7x7_pool_nhwc(x, w, b)
    return S.Case(dict(x=x, w=w, b=b), lambda L, p, st: L.isx_stem7x7_pool_nhwc(p.x, B, Hh, W, p.w, p.b, p.out, st),
                  lambda a: dict(out=O.stem7x7_pool_nhwc(a.x, a.w, a.b)), outs=dict(out=("f32", want.shape)), guard=dict(out=128 * 64, w=64 * 147))


@case("isx_conv1x1_nhwc", "tail_grid")
def _():
    """test_gpu_trunk_guards.py::test_conv1x1_tail_grid: 1047 row tiles, the rows past the whole rounds as 64x64 tiles in the same grid."""
    import test_gpu_trunk_guards as T
    M, Cin, Cout = 133956, 32, 128
    split = G.tail_split_rows(M, Cout, T.SLOTS)
    assert split == 131072 and not G.stream_applicable(M, Cin, Cout, 0), "the shape must take the tail split"
    x, w, b, _ = T._c1_case(M, Cin, Cout)
    rows = np.r_[0:100, split - 100:split + 100, M - 100:M]
    return S.Case(dict(x=x, w=w, b=b), lambda L, p, st: L.isx_conv1x1_nhwc(p.x, M, Cin, p.w, Cout, p.b, None, 1, p.y, st),
                  lambda a: dict(y=O.conv1x1_nhwc(a.x[rows], a.w, a.b, None, True)), outs=dict(y=("f32", (M, Cout))), sample=dict(y=_rows_of(rows)),
                  guard=dict(x=128 * Cin, w=128 * Cin, y=128 * Cout), hooks=(0, -1, -1))


@case("isx_conv3x3_nhwc", "tail_grid")
def _():
    """test_conv3x3_tail_grid at Cout = 128, stride 1: 128x128 tiles + 64x64 tail (conv cfg 0); the image that holds the split against the oracle."""
    import test_gpu_trunk_guards as T
    B, Ho, Cin, Cout = 9, 122, 32, 128
    M = B * Ho * Ho
    split = G.tail_split_rows(M, Cout, T.SLOTS)
    assert (B - 1) * Ho * Ho <= split < M, "the shape must take the tail split, and the split must fall inside the last image"
    x, w, b, _ = T._c3_case(B, Ho, Ho, Cin, Cout, 1)
    ch = T._channels(Cout)
    pick = lambda y: y[B - 1:B][..., torch.from_numpy(ch).to(y.device)]
    return S.Case(dict(x=x, w=w, b=b), lambda L, p, st: L.isx_conv3x3_nhwc(p.x, B, Ho, Ho, Cin, p.w, Cout, 1, p.b, None, 1, p.y, st),
                  lambda a: dict(y=O.conv3x3_nhwc(a.x[B - 1:B], a.w[ch], a.b[ch], 1, None, True)), outs=dict(y=("f32", (B, Ho, Ho, Cout))), sample=dict(y=pick),
                  guard=dict(x=128 * Cin * 64, w=128 * 9 * Cin, y=128 * Cout), hooks=(-1, 0, -1))


@case("isx_conv1x1_dual_nhwc", "tail_grid")
def _():
    import test_gpu_trunk_guards as T
    B, Ho, K1, K2, Cout = 9, 122, 32, 64, 128
    split = G.tail_split_rows(B * Ho * Ho, Cout, T.SLOTS)
    assert (B - 1) * Ho * Ho <= split < B * Ho * Ho, "the shape must take the tail split, and the split must fall inside the last image"
    t, x, w, b = T._dual_case(B, Ho, Ho, K1, K2, Cout, 1)
    return S.Case(dict(t=t, x=x, w=w, b=b), lambda L, p, st: L.isx_conv1x1_dual_nhwc(p.t, K1, p.x, B, Ho, Ho, K2, 1, p.w, Cout, p.b, 1, p.y, st),
                  lambda a: dict(y=O.conv1x1_dual_nhwc(a.t[B - 1:B], a.x[B - 1:B], a.w, a.b, 1, True)), outs=dict(y=("f32", (B, Ho, Ho, Cout))),
                  sample=dict(y=lambda y: y[B - 1:B]), guard=dict(t=128 * K1, x=128 * K2, w=128 * (K1 + K2), y=128 * Cout), hooks=(-1, 0, -1))


@case("isx_conv3x3_expand128_nhwc", "tail_grid")
def _():
    """test_conv3x3_expand128_tail_grid: position-major tiles AND the tail split, the last group ONE image."""
    import test_gpu_trunk_guards as T
    B, P, Cin, Cout = 13 * 128 + 1, 49, 64, 128
    groups = (B + 127) // 128
    Mv = G.pos_major_rows(B, 7, 7, Cin, 7, 7, Cout, 2)
    split = G.tail_split_rows(Mv, 128, T.SLOTS)
    assert Mv == groups * P * 128 and 0 < split < Mv, "position-major AND the tail split"
    g_big, g_tail = split // 128 // P - 1, -(-(split // 128) // P)
    images = [g_big * 128 + 5, g_tail * 128 + 3, g_tail * 128 + 64 + 28, B - 1]
    x, w2, b2, w3, b3, r = T._e128_case(B, 7, 7, Cin, Cout)
    ref = lambda a: dict(y=T._e128_oracle((a.x, a.w2, a.b2, np.ascontiguousarray(a.w3t.T), a.b3, a.r), True, True, images))
    og = T._out_guard(B, 7, 7, Cout)
    return S.Case(dict(x=x, w2=w2, b2=b2, w3t=np.ascontiguousarray(w3.T), b3=b3, r=r),
                  lambda L, p, st: L.isx_conv3x3_expand128_nhwc(p.x, B, 7, 7, Cin, p.w2, p.b2, p.w3t, Cout, p.b3, p.r, 1, p.y, st), ref,
                  outs=dict(y=("f32", (B, 7, 7, Cout))), sample=dict(y=_rows_of(images)), guard=dict(x=128 * Cin * 49, w2=128 * 9 * Cin, w3t=128 * Cout, r=og, y=og))


@case("isx_conv3x3_expand_nhwc")
def _():
    B, Hh, W, Cin = 2, 7, 7, 64
    rng = _rng(B, Hh, Cin)
    x = np.maximum(_normal(rng, B, Hh, W, Cin), 0)
    w2, b2 = _normal(rng, 64, 3, 3, Cin) * F((9 * Cin) ** -0.5), _normal(rng, 64)
    w3, b3, r = _normal(rng, 256, 64) * F(0.125), _normal(rng, 256), _normal(rng, B, Hh, W, 256)

    def ref(a):
        mid = O.conv3x3_nhwc(a.x, a.w2, a.b2, 1, None, True)
        return dict(y=O.conv1x1_nhwc(mid.reshape(-1, 64), np.ascontiguousarray(a.w3t.T), a.b3, a.r.reshape(-1, 256), True).reshape(B, Hh, W, 256))
    return S.Case(dict(x=x, w2=w2, b2=b2, w3t=np.ascontiguousarray(w3.T), b3=b3, r=r),
                  lambda L, p, st: L.isx_conv3x3_expand_nhwc(p.x, B, Hh, W, Cin, p.w2, p.b2, 1, p.w3t, 256, p.b3, p.r, 1, p.y, st), ref,
                  outs=dict(y=("f32", (B, Hh, W, 256))), guard=dict(x=128 * Cin, w2=64 * 9 * Cin, w3t=64 * 256, r=128 * 256, y=128 * 256))


@case("isx_conv3x3_expand_dual_nhwc")
def _():
    B, Hh, W, Cin = 2, 7, 7, 64
    rng = _rng(B, Hh, Cin, 1)
    t, x2 = np.maximum(_normal(rng, B, Hh, W, Cin), 0), np.maximum(_normal(rng, B, Hh, W, 64), 0)
    w2, b2 = _normal(rng, 64, 3, 3, Cin) * F((9 * Cin) ** -0.5), _normal(rng, 64)
    wc, b = _normal(rng, 256, 128) * F(128 ** -0.5), _normal(rng, 256)
    ref = lambda a: dict(y=O.conv1x1_dual_nhwc(O.conv3x3_nhwc(a.t, a.w2, a.b2, 1, None, True), a.x2, np.ascontiguousarray(a.wct.T), a.b, 1, True))
    return S.Case(dict(t=t, w2=w2, b2=b2, x2=x2, wct=np.ascontiguousarray(wc.T), b=b),
                  lambda L, p, st: L.isx_conv3x3_expand_dual_nhwc(p.t, B, Hh, W, Cin, p.w2, p.b2, p.x2, p.wct, 256, p.b, 1, p.y, st), ref,
                  outs=dict(y=("f32", (B, Hh, W, 256))), guard=dict(t=128 * Cin, w2=64 * 9 * Cin, x2=128 * 64, wct=64 * 256, y=128 * 256))


@case("isx_boxpool_s1")
def _():
    B, C, Hh, W, kh, kw = 2, 67, 13, 11, 3, 2
    fmap = _normal(_rng(Hh * W, C), B, C, Hh, W)
    return S.Case(dict(f=fmap), lambda L, p, st: L.isx_boxpool_s1(p.f, B, C, Hh, W, kh, kw, p.out, st), lambda a: dict(out=O.boxpool_s1(a.f, kh, kw)),
                  outs=dict(out=("f32", (B, C, Hh - kh + 1, W - kw + 1))), guard=dict(f=64 * Hh * W, out=64 * Hh * W))


@case("isx_boxpool_s1_nhwc")
def _():
    B, C, Hh, W, kh, kw = 3, 96, 7, 5, 3, 2
    fmap = _normal(_rng(Hh * W, C, 1), B, C, Hh, W)
    return S.Case(dict(f=_nhwc(fmap)), lambda L, p, st: L.isx_boxpool_s1_nhwc(p.f, B, C, Hh, W, kh, kw, p.out, st),
                  lambda a: dict(out=_nhwc(O.boxpool_s1(_nchw(a.f), kh, kw))), outs=dict(out=("f32", (B, Hh - kh + 1, W - kw + 1, C))))


@case("isx_boxpool_s1_bwd_nhwc")
def _():
    Hh, W, kh, kw, C = 7, 5, 3, 2, 96
    g = _normal(_rng(100 * Hh + C), 3, Hh - kh + 1, W - kw + 1, C)
    return S.Case(dict(g=g), lambda L, p, st: L.isx_boxpool_s1_bwd_nhwc(p.g, 3, C, Hh, W, kh, kw, p.dx, st),
                  lambda a: dict(dx=em.boxpool_bwd_canonical(a.g, Hh, W, kh, kw)), outs=dict(dx=("f32", (3, Hh, W, C))))


@case("isx_gap_bwd_nhwc")
def _():
    B, Hh, W, C = 3, 2, 5, 12
    g = _normal(_rng(B), B, C)
    return S.Case(dict(g=g), lambda L, p, st: L.isx_gap_bwd_nhwc(p.g, B, Hh, W, C, p.dx, st),
                  lambda a: dict(dx=np.ascontiguousarray(np.broadcast_to((a.g / F(Hh * W))[:, None, None, :], (B, Hh, W, C)))), outs=dict(dx=("f32", (B, Hh, W, C))))


# ==== region path ===================================================================================================================================
def _best(nhwc):
    K, Hp, Wp = 17, 3, 2
    cls = dm.best_case(K, Hp, Wp)
    B = cls.shape[0]
    fn = "isx_best_location_desc_nhwc" if nhwc else "isx_best_location_desc"

    def ref(a):
        desc, loc = dm.best_location_desc(_nchw(a.cls) if nhwc else a.cls)
        return dict(desc=desc, loc=np.ascontiguousarray(loc, np.int64))
    return S.Case(dict(cls=_nhwc(cls) if nhwc else np.array(cls)), lambda L, p, st: getattr(L, fn)(p.cls, B, K, Hp, Wp, EPS, p.desc, p.loc, st), ref,
                  outs=dict(desc=("f32", (B, K)), loc=("i64", (B, 2))))


case("isx_best_location_desc")(lambda: _best(False))
case("isx_best_location_desc_nhwc")(lambda: _best(True))


def _region_topk(nhwc):
    B, K, Hp, Wp, k = 3, 17, 8, 6, 7
    cls = em.topk_case(B, K, Hp, Wp, True)
    fn = "isx_region_topk_nhwc" if nhwc else "isx_region_topk"

    def ref(a):
        idx, sc = em.oracle_region_topk(_nchw(a.cls) if nhwc else a.cls, k)
        return dict(idx=np.ascontiguousarray(idx, np.int64), sc=sc)
    return S.Case(dict(cls=em.to_nhwc(cls) if nhwc else np.array(cls)), lambda L, p, st: getattr(L, fn)(p.cls, B, K, Hp, Wp, k, p.idx, p.sc, st), ref,
                  outs=dict(idx=("i64", (B, k)), sc=("f32", (B, k))))


case("isx_region_topk")(lambda: _region_topk(False))
case("isx_region_topk_nhwc")(lambda: _region_topk(True))


def _gather(nhwc):
    """Six windows per image, among them -1 and the first index past the map; as decoys the indices are zeros: window 0."""
    C, kh, kw = dm.GATHER[0]
    fmap, idx, Wp, shift = dm.gather_case(C, kh, kw)
    B, _, Hf, Wf = fmap.shape
    k = idx.shape[1]
    fn = "isx_region_gather_l2_nhwc" if nhwc else "isx_region_gather_l2"
    ref = lambda a: dict(rows=dm.region_gather_l2(_nchw(a.f) if nhwc else a.f, kh, kw, a.idx, Wp, shift=a.shift, order="hwc" if nhwc else "chw"))
    return S.Case(dict(f=_nhwc(fmap) if nhwc else np.array(fmap), idx=np.ascontiguousarray(idx, np.int64), shift=dm.shift_hwc(shift, C, kh, kw) if nhwc else np.array(shift)),
                  lambda L, p, st: getattr(L, fn)(p.f, B, C, Hf, Wf, kh, kw, p.idx, k, Wp, p.shift, EPS, p.rows, st), ref, outs=dict(rows=("f32", (B, k, C * kh * kw))))


case("isx_region_gather_l2")(lambda: _gather(False))
case("isx_region_gather_l2_nhwc")(lambda: _gather(True))


@case("isx_region_sum_l2_nhwc")
def _():
    B, Hf, Wf, C, kh, kw, k = c = rm.CASES[0]
    fmap, idx, Wp, shift, g, add = rm.make_case(c)

    def ref(a):
        rows, n2 = rm.region_sum_l2(_nchw(a.f), kh, kw, a.idx, Wp, a.shift)
        return dict(rows=rows, n2=n2)
    return S.Case(dict(f=_nhwc(fmap), idx=np.array(idx), shift=np.array(shift)),
                  lambda L, p, st: L.isx_region_sum_l2_nhwc(p.f, B, C, Hf, Wf, kh, kw, p.idx, k, Wp, p.shift, EPS, p.rows, p.n2, st), ref,
                  outs=dict(rows=("f32", (B, C * kh * kw)), n2=("f32", (B, k))))


@case("isx_region_sum_l2_bwd_nhwc")
def _():
    B, Hf, Wf, C, kh, kw, k = c = rm.CASES[0]
    fmap, idx, Wp, shift, g, add = rm.make_case(c)
    _, n2 = rm.region_sum_l2(fmap, kh, kw, idx, Wp, shift)

    def ref(a):
        df, cw = rm.region_sum_l2_bwd(_nchw(a.f), a.g, a.n2, kh, kw, a.idx, Wp, _nchw(a.add))
        return dict(dfmap=_nhwc(df), cw=cw)
    return S.Case(dict(f=_nhwc(fmap), g=np.array(g), n2=n2, idx=np.array(idx), add=_nhwc(add)),
                  lambda L, p, st: L.isx_region_sum_l2_bwd_nhwc(p.f, p.g, p.n2, B, C, Hf, Wf, kh, kw, p.idx, k, Wp, p.add, 1, p.cw, p.dfmap, st), ref,
                  outs=dict(cw=("f32", (B, k)), dfmap=("f32", (B, Hf, Wf, C))))


# ==== retrieval =====================================================================================================================================
def _unit(rng, n, d):
    return O.l2norm_rows(_normal(rng, n, d))


@case("isx_cosine_sim")
def _():
    M, N, D = 33, 129, 17
    rng = _rng(M, N, D)
    Q, Gm = _unit(rng, M, D), _unit(rng, N, D)
    return S.Case(dict(q=Q, g=Gm), lambda L, p, st: L.isx_cosine_sim(p.q, M, p.g, N, D, p.sim, st), lambda a: dict(sim=O.cosine_sim(a.q, a.g)),
                  outs=dict(sim=("f32", (M, N))), guard=dict(sim=128 * N))


SEARCH = (37, 9000, 64, 10)                        # tests/test_gpu_fast_guards.py TOPK_CASES[0]
NC = 2432                                          # its narrow chunk width
IDX_BASE = 11


def _search_data(shape, seed):
    M, N, D, k = shape
    rng = _rng(seed)
    Q, Gm = _unit(rng, M, D), _unit(rng, N, D)
    Gm[N // 2] = Gm[3]
    Gm[N - 1] = Gm[3]
    return Q, Gm


def _topk_ref(k):
    def ref(a):
        s, i = O.cosine_topk(a.q, a.g, k, idx_base=IDX_BASE)
        return dict(ts=s, ti=np.ascontiguousarray(i, np.int64))
    return ref


@case("isx_cosine_topk", "chunks")
def _():
    """A workspace that holds 2432-column chunks: four chunks, the carry (zeroed by the memset on the stream) merged into every later one.  k > 1
    and the later chunks contribute to the lists."""
    M, N, D, k = SEARCH
    nbytes = G.topk_fixed_bytes(M, k) + 4 * M * (NC + 128)
    chunks = G.topk_chunks(M, N, k, nbytes, False)
    assert len(chunks) >= 2 and all(w == NC for _, w, _ in chunks[:-1]) and all(f for _, _, f in chunks[1:]), chunks
    Q, Gm = _search_data(SEARCH, 1)
    want = O.cosine_topk(Q, Gm, k, idx_base=IDX_BASE)[1]
    assert k > 1 and (want - IDX_BASE >= NC).any() and (want - IDX_BASE < NC).any(), "later chunks must contribute"
    return S.Case(dict(q=Q, g=Gm), lambda L, p, st: L.isx_cosine_topk(p.q, M, p.g, N, D, k, IDX_BASE, p.ts, p.ti, p.ws, nbytes, st), _topk_ref(k),
                  outs=dict(ts=("f32", (M, k)), ti=("i64", (M, k))), ws=dict(ws=nbytes), guard=dict(q=128 * D, g=128 * D))


def _fast(shape, nc, data, post=None):
    import test_gpu_fast_guards as TF
    M, N, D, k = shape
    Q, Gm = data
    L = _lib()
    assert L.isx_cosine_topk_fast_fallback_offset(M, N, D, k, 0) != TF.NO_WS, "the shape must take the fp16 filter path"
    nbytes = TF._ws_bytes(M, N, D, k, False, nc)
    c = S.Case(dict(q=Q, g=Gm), lambda L, p, st: L.isx_cosine_topk_fast(p.q, M, p.g, N, D, k, IDX_BASE, None, None, p.ts, p.ti, p.ws, nbytes, st), _topk_ref(k),
               outs=dict(ts=("f32", (M, k)), ti=("i64", (M, k))), ws=dict(ws=nbytes), guard=dict(q=256 * D, g=256 * D), hooks=(-1, -1, 1))
    c.post = post
    return c


@case("isx_cosine_topk_fast", "chunks")
def _():
    """The gallery converted into the workspace (two conversions, the approximate pass in filtered chunks with its carry memset, window, rescore,
    compact, the exact pass over the fallback rows, gather): every stage through the one workspace the late producer has just refilled."""
    import test_gpu_fast_guards as TF
    TF._topk_plan(TF.TOPK_CASES[0], False)                                     # asserts >= 3 chunks of 2432 columns, all but the first filtered
    assert TF.TOPK_CASES[0][0] == SEARCH and NC in TF.TOPK_CASES[0][1]
    return _fast(SEARCH, NC, _search_data(SEARCH, 2))


FALLBACK = (9, 1024, 64, 20)                       # tests/test_gpu_fast_guards.py FALLBACK_SHAPE: dense clusters, every row takes the exact pass


@case("isx_cosine_topk_fast", "fallback_rows")
def _():
    import test_gpu_fast_guards as TF
    assert TF.FALLBACK_SHAPE == FALLBACK
    M, N, D, k = FALLBACK
    Q, Gm = TF.fallback_case()

    def post(L, p):                                                          # after the stream has drained: rows did take the fallback
        assert L.isx_debug_fast_fallback_rows(p.ws, M, N, D, k, 0) > 0
    return _fast(FALLBACK, None, (Q, Gm), post)


@case("isx_rows_to_f16")
def _():
    B, D = 5, 200
    x = _normal(_rng(20 + B * D), B, D)
    x[1, :8] = [65504.0, -65504.0, 6.1e-5, 5.96e-8, 2.9e-8, 0.0, -0.0, 1.0009765625]

    import test_gpu_fast_guards as TF
    norm2 = lambda got, exact, a: TF.norm2_within(got, a.x)                  # the bound of test_rows_to_f16
    return S.Case(dict(x=x), lambda L, p, st: L.isx_rows_to_f16(p.x, B, D, p.h, p.n2, p.am, st),
                  lambda a: dict(h=a.x.astype(H16), am=np.abs(a.x).max(1), n2=(a.x.astype(np.float64) ** 2).sum(1)),
                  outs=dict(h=("f16", (B, D)), n2=("f32", (B,)), am=("f32", (B,))), check=dict(n2=norm2))


@case("isx_gallery_to_f16")
def _():
    N, D = 5, 200
    Gm = _unit(_rng(21 + N * D), N, D) * F(0.3)
    Gm[3, 1:6] = F(1e-12) * np.arange(1, 6, dtype=F)
    Gm[3, 6] = F(-1e-12)

    import test_gpu_fast_guards as TF

    def ref(a):                                                              # the model and the bounds of test_gallery_to_f16
        want, n2max, amax, lost = TF.gallery_f16_model(a.g)
        return dict(gh=want, gs=np.array([n2max, amax, lost, 0.0]))
    gstats = lambda s_, want, a: TF.gstats_within(s_, want[0], want[1], want[2], D)
    return S.Case(dict(g=Gm), lambda L, p, st: L.isx_gallery_to_f16(p.g, N, D, p.gh, p.gs, st), ref, outs=dict(gh=("f16", (N, D)), gs=("f32", (4,))),
                  check=dict(gs=gstats))


@case("isx_cosine_sim_f16")
def _():
    M, N, D = 130, 257, 64
    rng = np.random.default_rng(M + N + D)
    q, g = rng.standard_normal((M, D)).astype(H16), rng.standard_normal((N, D)).astype(H16)

    import test_gpu_fast_guards as TF

    def within(got, want, a):                                                # the bound of test_cosine_sim_f16
        assert not np.isnan(got).any() and (np.abs(got - want) <= TF.sim_f16_bound(a.q, a.g)[1]).all()
    return S.Case(dict(q=q, g=g), lambda L, p, st: L.isx_cosine_sim_f16(p.q, M, p.g, N, D, p.sim, st),
                  lambda a: dict(sim=TF.sim_f16_bound(a.q, a.g)[0]), outs=dict(sim=("f32", (M, N))), check=dict(sim=within),
                  guard=dict(q=256 * D, g=256 * D, sim=256 * N))


@case("isx_topk_rows")
def _():
    M, N, k = 3, 300, 64
    sim = _normal(_rng(N + k), M, N)
    sim[:, N // 3] = sim[:, 1]

    def ref(a):
        s, i = O.topk_rows(a.sim, k, idx_base=3)
        return dict(ts=s, ti=np.ascontiguousarray(i, np.int64))
    return S.Case(dict(sim=sim), lambda L, p, st: L.isx_topk_rows(p.sim, M, N, k, 3, p.ts, p.ti, st), ref, outs=dict(ts=("f32", (M, k)), ti=("i64", (M, k))),
                  guard=dict(ts=128 * k, ti=128 * k))


def _merge_lists(P, M, k, N=400, D=32):
    rng = _rng(P * k)
    Q, Gm = _unit(rng, M, D), _unit(rng, N, D)
    Gm[100] = Gm[390]
    bounds = np.linspace(0, N, P + 1).astype(int)
    parts = [O.cosine_topk(Q, Gm[a:b], k, idx_base=a) for a, b in zip(bounds[:-1], bounds[1:])]
    return np.stack([p[0] for p in parts]), np.ascontiguousarray(np.stack([p[1] for p in parts]), np.int64)


def _merge_ref(a):
    s, i = O.topk_merge(a.s, a.i)
    return dict(ts=s, ti=np.ascontiguousarray(i, np.int64))


@case("isx_topk_merge")
def _():
    P, M, k = 3, 9, 4
    Sc, I = _merge_lists(P, M, k)
    return S.Case(dict(s=Sc, i=I), lambda L, p, st: L.isx_topk_merge(p.s, p.i, P, M, k, p.ts, p.ti, st), _merge_ref, outs=dict(ts=("f32", (M, k)), ti=("i64", (M, k))))


def _rank_case(M, N):
    import test_gpu_retrieval_guards as TR
    return TR._rank_case(M, N)


@case("isx_rank_full", "global_network")
def _():
    """N = 4097 pads to 8192: the LDS sort of the blocks, then the passes of the global bitonic network -- several launches through the workspace."""
    M, N = 4, 4097
    sim = _rank_case(M, N)
    nbytes = _lib().isx_rank_full_workspace(M, N)
    return S.Case(dict(sim=sim), lambda L, p, st: L.isx_rank_full(p.sim, M, N, p.ranked, p.ws, nbytes, st),
                  lambda a: dict(ranked=np.ascontiguousarray(O.rank_full(a.sim), np.int64)), outs=dict(ranked=("i64", (M, N))), ws=dict(ws=nbytes))


def _ap_labels(M, N):
    Lb = max(1, N // 10)
    gl, ql = (np.arange(N) % Lb).astype(np.int32), (np.arange(M) % (Lb + 1)).astype(np.int32)
    ql[M - 1] = Lb                                                           # absent from the gallery: NaN
    return ql, gl


@case("isx_average_precision")
def _():
    M, N = 5, 24
    ranked = np.ascontiguousarray(O.rank_full(_rank_case(M, N)), np.int64)
    ql, gl = _ap_labels(M, N)
    return S.Case(dict(ranked=ranked, ql=ql, gl=gl), lambda L, p, st: L.isx_average_precision(p.ranked, M, N, p.ql, p.gl, 2, p.ap, st),
                  lambda a: dict(ap=O.average_precision(a.ranked, a.ql, a.gl, 2)), outs=dict(ap=("f64", (M,))), check=dict(ap=_same_ap))


@case("isx_average_precision_sim")
def _():
    M, N = 4, 4097
    sim = _rank_case(M, N)
    ql, gl = _ap_labels(M, N)
    return S.Case(dict(sim=sim, ql=ql, gl=gl), lambda L, p, st: L.isx_average_precision_sim(p.sim, M, N, p.ql, p.gl, 1, p.ap, st),
                  lambda a: dict(ap=O.average_precision(O.rank_full(a.sim), a.ql, a.gl, 1)), outs=dict(ap=("f64", (M,))), check=dict(ap=_same_ap))


@case("isx_masked_sums")
def _():
    M, N, nlab = 20, 777, 5
    sim = _normal(_rng(N + M), M, N)
    gl, ql = (np.arange(N) % nlab).astype(np.int32), (np.arange(M) % nlab).astype(np.int32)
    ql[M - 1] = nlab

    def ref(a):
        rows = [[float(v) for v in r] for r in a.sim]
        return dict(out=np.array([[math.fsum(v for v, l in zip(row, a.gl) if l == a.ql[i]), math.fsum(row)] for i, row in enumerate(rows)]))

    def within(got, want, a):                                                # tests/test_gpu_retrieval_guards.py: N float64 adds in any order
        bound = N * 2.0 ** -52 * np.abs(a.sim.astype(np.float64)).sum(1)
        assert (np.abs(got - want) <= bound[:, None]).all() and got[M - 1, 0] == 0.0
    return S.Case(dict(sim=sim, ql=ql, gl=gl), lambda L, p, st: L.isx_masked_sums(p.sim, M, N, p.ql, p.gl, p.out, st), ref, outs=dict(out=("f64", (M, 2))),
                  check=dict(out=within))


@case("isx_dba_groups")
def _():
    """Decoys: order = grp_begin = 0, grp_size = 1 -- every item a singleton of item 0's slot: in range whenever it is read."""
    import test_gpu_eval_guards as EG
    D = 64
    E, labels = EG._dba_data(D, (1, 2, 3, 5), D)
    N = len(labels)
    order, begin, size, mg = em.dba_groups_of(labels)
    ref = lambda a: dict(out=em.dba_chain(a.emb, np.ascontiguousarray(a.begin, np.int32), -1))      # items of one instance share grp_begin
    G.assert_bits(ref(types.SimpleNamespace(emb=E, begin=begin))["out"], em.dba_chain(E, labels, -1))
    return S.Case(dict(emb=E, order=np.ascontiguousarray(order, np.int32), begin=np.ascontiguousarray(begin, np.int32), size=np.ascontiguousarray(size, np.int32)),
                  lambda L, p, st: L.isx_dba_groups(p.emb, N, D, p.order, p.begin, p.size, mg, -1, p.out, st), ref, outs=dict(out=("f32", (N, D))),
                  decoy=dict(size=np.ones(N, np.int32)))


AP_MAXP = em.AP_MAXP


@case("isx_ap_shard_positives")
def _():
    rng = np.random.default_rng(4)
    N, base, M = 40, 1001, 3
    sim = rng.standard_normal((M, N), dtype=F)
    gl = np.full(N, 7, np.int32)
    gl[rng.choice(N, 9, replace=False)] = 0
    ql = np.array([0, 5, 7], np.int32)

    def ref(a):
        keys, count = np.zeros((M, AP_MAXP), np.uint64), np.zeros(M, np.int32)
        for r in range(M):
            j = np.flatnonzero(a.gl == a.ql[r])
            keys[r, :len(j)] = em.rank_keys(a.sim[r, j], base + j)
            count[r] = len(j)
        return dict(keys=np.sort(keys, axis=1), count=count)

    def as_sets(got, want, a):                                               # "any order" (include/isx.h): the rows as sorted sets
        np.testing.assert_array_equal(np.sort(got.view(np.uint64), axis=1), want)
    return S.Case(dict(sim=sim, ql=ql, gl=gl), lambda L, p, st: L.isx_ap_shard_positives(p.sim, M, N, base, p.ql, p.gl, AP_MAXP, p.keys, p.count, st), ref,
                  outs=dict(keys=("i64", (M, AP_MAXP)), count=("i32", (M,))), check=dict(keys=as_sets))


@case("isx_ap_shard_hist")
def _():
    import test_gpu_eval_guards as EG
    M, N, W, npos = 3, 2000, 300, (137, 300, 1)
    rng = np.random.default_rng(W)
    sim = (np.round(rng.standard_normal((M, N)) * 2) / 2).astype(F)
    keys_all = np.zeros((M, W), np.uint64)
    for r, n in enumerate(npos):
        j = rng.choice(N, n, replace=False)
        keys_all[r, rng.choice(W, n, replace=False)] = em.rank_keys(sim[r, j], j)
    return S.Case(dict(sim=sim, keys=keys_all), lambda L, p, st: L.isx_ap_shard_hist(p.sim, M, N, 0, p.keys, W, p.hist, st),
                  lambda a: dict(hist=np.ascontiguousarray(EG._cpu_hist(a.sim, 0, a.keys), np.int32)), outs=dict(hist=("i32", (M, AP_MAXP))))


@case("isx_ap_from_hist")
def _():
    from utils import metrics
    rng = np.random.default_rng(65)
    M, ld = 65, 40
    n_lab = rng.integers(0, 46, M).astype(np.int32)
    n_lab[:6] = [3, 0, 41, 40, 1, 2]
    hist = np.zeros((M, ld), np.int32)
    for r in range(M):
        n = min(int(n_lab[r]), ld)
        hist[r, :n] = 1 + rng.integers(0, 4, n) * rng.integers(0, 2, n)
    hist[::2, 0] = 1
    return S.Case(dict(hist=hist, n_lab=n_lab), lambda L, p, st: L.isx_ap_from_hist(p.hist, ld, p.n_lab, M, 2, p.ap, st),
                  lambda a: dict(ap=metrics.ap_from_hist(torch.from_numpy(a.hist), torch.from_numpy(a.n_lab), 2).numpy()), outs=dict(ap=("f64", (M,))),
                  check=dict(ap=_same_ap))


# ==== triplet training ==============================================================================================================================
MINE_N = 257


def _mine_ref(N, row_base):
    return lambda a: dict(neg=np.ascontiguousarray(tm.mine(a.sim, N, row_base, a.labels, a.i1, a.i2, 1), np.int64))


@case("isx_mine_negatives")
def _():
    c = tm.mine_case(MINE_N)
    i1, i2, _ = tm.all_couples(c)
    i1, i2 = np.ascontiguousarray(i1, np.int64), np.ascontiguousarray(i2, np.int64)
    n = len(i1)
    return S.Case(dict(sim=np.array(c.sim, F), labels=np.ascontiguousarray(c.labels, np.int32), i1=i1, i2=i2),
                  lambda L, p, st: L.isx_mine_negatives(p.sim, MINE_N, p.labels, p.i1, p.i2, n, 1, p.neg, st), _mine_ref(MINE_N, 0), outs=dict(neg=("i64", (n,))))


@case("isx_mine_negatives_rows")
def _():
    """Rows [1, 8) of the matrix.  The anchors index the block: as a decoy i1 is the block's first row, not zero."""
    c = tm.mine_case(MINE_N)
    i1, i2, _ = tm.all_couples(c)
    r0, r1 = 1, 8
    sel = np.flatnonzero((i1 >= r0) & (i1 < r1))
    assert len(sel)
    i1, i2 = np.ascontiguousarray(i1[sel], np.int64), np.ascontiguousarray(i2[sel], np.int64)
    n = len(i1)
    return S.Case(dict(sim=np.ascontiguousarray(c.sim[r0:r1], F), labels=np.ascontiguousarray(c.labels, np.int32), i1=i1, i2=i2),
                  lambda L, p, st: L.isx_mine_negatives_rows(p.sim, MINE_N, r0, r1 - r0, p.labels, p.i1, p.i2, n, 1, p.neg, st), _mine_ref(MINE_N, r0),
                  outs=dict(neg=("i64", (n,))), decoy=dict(i1=np.full(n, r0, np.int64)))


TRIPLET = (7, 100)


@case("isx_triplet_loss_fwd")
def _():
    B, D = TRIPLET
    a_, p_, n_ = tm.row_case(B, D)
    return S.Case(dict(a=a_, p=p_, n=n_), lambda L, p, st: L.isx_triplet_loss_fwd(p.a, p.p, p.n, B, D, tm.MARGIN, 1, p.rows, st),
                  lambda a: dict(rows=tm.loss_rows(a.a, a.p, a.n, tm.MARGIN, True)), outs=dict(rows=("f32", (B,))))


def _triplet_bwd(dev):
    B, D = TRIPLET
    a_, p_, n_ = tm.row_case(B, D)
    rows = tm.loss_rows(a_, p_, n_, tm.MARGIN, True)
    assert (rows > 0).any() and (rows == 0).any()

    def ref(a):
        scale = tm.scale_dev(1.0 / B, float(a.sd[0])) if dev else tm.scale_host(1.0 / B)
        return dict(zip(("ga", "gp", "gn"), tm.grads(a.a, a.p, a.n, a.rows, scale, True)))
    ins = dict(a=a_, p=p_, n=n_, rows=rows)
    if dev:
        ins["sd"] = np.array([tm.SCALE_DEV], F)
        call = lambda L, p, st: L.isx_triplet_loss_bwd_dev(p.a, p.p, p.n, p.rows, B, D, 1.0 / B, p.sd, 1, p.ga, p.gp, p.gn, st)
    else:
        call = lambda L, p, st: L.isx_triplet_loss_bwd(p.a, p.p, p.n, p.rows, B, D, 1.0 / B, 1, p.ga, p.gp, p.gn, st)
    return S.Case(ins, call, ref, outs=dict(ga=("f32", (B, D)), gp=("f32", (B, D)), gn=("f32", (B, D))))


case("isx_triplet_loss_bwd")(lambda: _triplet_bwd(False))
case("isx_triplet_loss_bwd_dev")(lambda: _triplet_bwd(True))


@case("isx_triplet_leaves")
def _():
    Lv, k, D = 3, 5, 100
    d = tm.leaf_case(Lv, k, D)
    sa, sb = tm.leaf_scales(Lv, k, True)

    def ref(a):
        loss, dd, _ = tm.leaves(a.d, Lv, k, tm.MARGIN, True, sa, sb)
        return dict(loss=loss, dd=dd)
    return S.Case(dict(d=d), lambda L, p, st: L.isx_triplet_leaves(p.d, Lv, k, D, tm.MARGIN, 1, sa, sb, p.loss, p.dd, st), ref,
                  outs=dict(loss=("f32", (Lv,)), dd=("f32", (Lv * 3 * k, D))))


# ==== classification fine-tuning ====================================================================================================================
def _xent():
    import test_gpu_xent_chains as XC                                         # EXP / LOG: the device's expf and logf, read through isx_debug_expf_logf
    return XC.EXP, XC.LOG


@case("isx_softmax_xent_fwd")
def _():
    B, C = 5, 311
    z, y, _ = xm.batch_case(B, C)
    EXP, LOG = _xent()
    return S.Case(dict(z=z, y=np.ascontiguousarray(y, np.int32)), lambda L, p, st: L.isx_softmax_xent_fwd(p.z, p.y, B, C, p.rows, st),
                  lambda a: dict(rows=np.asarray(xm.forward(a.z, a.y, EXP, LOG), F)), outs=dict(rows=("f32", (B,))))


@case("isx_softmax_xent_bwd")
def _():
    B, C = 5, 311
    z, y, _ = xm.batch_case(B, C)
    EXP, LOG = _xent()
    return S.Case(dict(z=z, y=np.ascontiguousarray(y, np.int32), sd=np.array([xm.SCALE_DEV], F)),
                  lambda L, p, st: L.isx_softmax_xent_bwd(p.z, p.y, B, C, 0.2, p.sd, p.dz, st),
                  lambda a: dict(dz=np.asarray(xm.backward(a.z, a.y, xm.scale_of(0.2, float(a.sd[0])), EXP), F)), outs=dict(dz=("f32", (B, C))))


@case("isx_softmax_xent_leaves")
def _():
    Lv, k, C = 3, 4, 129
    z, y = xm.leaf_case(Lv, k, C)
    EXP, LOG = _xent()

    def ref(a):
        loss, dz, _ = xm.leaves(a.z, a.y, Lv, k, 0.2, xm.SCALE_DEV, EXP, LOG)
        return dict(loss=np.asarray(loss, F), dz=np.asarray(dz, F))
    return S.Case(dict(z=z, y=np.ascontiguousarray(y, np.int32)), lambda L, p, st: L.isx_softmax_xent_leaves(p.z, p.y, Lv, k, C, 0.2, xm.SCALE_DEV, p.loss, p.dz, st),
                  ref, outs=dict(loss=("f32", (Lv,)), dz=("f32", (Lv * k, C))))


@case("isx_linear_wgrad_leaves")
def _():
    Lv, R, N, K = 2, 3, 18, 260
    rng = np.random.default_rng(100 * N + K)
    dy, x = rng.standard_normal((Lv * R, N)).astype(F), rng.standard_normal((Lv * R, K)).astype(F)
    ref = lambda a: dict(dw=np.stack([O.cosine_sim(np.ascontiguousarray(a.dy[l * R:(l + 1) * R].T), np.ascontiguousarray(a.x[l * R:(l + 1) * R].T)) for l in range(Lv)]))
    return S.Case(dict(dy=dy, x=x), lambda L, p, st: L.isx_linear_wgrad_leaves(p.dy, p.x, Lv, R, N, K, p.dw, st), ref, outs=dict(dw=("f32", (Lv, N, K))))


# ==== trunk-suffix backward =========================================================================================================================
@case("isx_conv1x1_dgrad_nhwc")
def _():
    Cin, Cout, M = 100, 80, 65
    dz, wt, add, mask, _ = sm.dgrad1_case(Cin, Cout)
    return S.Case(dict(dz=np.array(dz[:M]), wt=np.array(wt), add=np.array(add[:M]), mask=np.array(mask[:M])),
                  lambda L, p, st: L.isx_conv1x1_dgrad_nhwc(p.dz, M, Cout, p.wt, Cin, p.add, p.mask, p.dx, st),
                  lambda a: dict(dx=sm.dgrad1x1(a.dz, a.wt, a.add, a.mask)), outs=dict(dx=("f32", (M, Cin))), guard=dict(dx=128 * Cin, dz=128 * Cout, wt=128 * Cout))


@case("isx_conv3x3_dgrad_nhwc")
def _():
    name = "9x8_three_row_tiles"
    B, Hh, W, Cout, Cin, _ = sm.DGRAD3_CASES[name]
    dz, wt, mask, _ = sm.dgrad3_case(name)
    return S.Case(dict(dz=np.array(dz), wt=np.array(wt), mask=np.array(mask)), lambda L, p, st: L.isx_conv3x3_dgrad_nhwc(p.dz, B, Hh, W, Cout, p.wt, Cin, p.mask, p.dx, st),
                  lambda a: dict(dx=sm.dgrad3x3(a.dz, a.wt, a.mask)), outs=dict(dx=("f32", (B, Hh, W, Cin))),
                  guard=dict(dx=128 * Cin, dz=128 * Cout * 64, wt=128 * 9 * Cout))


@case("isx_conv3x3_s2_col2im_nhwc")
def _():
    B, Hh, W, Cin = 2, 7, 9, 8
    dcol, mask, _ = sm.col2im_case(B, Hh, W, Cin)
    return S.Case(dict(dcol=np.array(dcol), mask=np.array(mask)), lambda L, p, st: L.isx_conv3x3_s2_col2im_nhwc(p.dcol, B, Hh, W, Cin, p.mask, p.dx, st),
                  lambda a: dict(dx=sm.col2im_s2(a.dcol, B, Hh, W, Cin, a.mask)), outs=dict(dx=("f32", (B, Hh, W, Cin))))


@case("isx_conv_wgrad_nhwc", "splits")
def _():
    name = "1x1_short_and_empty_split"
    g, Cin, Cout, leaves, _ = sm.WGRAD_CASES[name]
    K = sm.wgrad_K(name)
    Sp = _lib().isx_conv_wgrad_splits(K, Cin, Cout, g.taps)
    assert Sp > 1, "the shape must split its pixels"
    dz, x = sm.wgrad_inputs(name)
    return S.Case(dict(dz=np.array(dz), x=np.array(x)),
                  lambda L, p, st: L.isx_conv_wgrad_nhwc(p.dz, p.x, g.B, leaves, g.H, g.W, Cin, Cout, g.taps, g.stride, p.dw, p.db, st),
                  lambda a: dict(zip(("dw", "db"), sm.wgrad_partials(a.dz, a.x, g, leaves, Sp))),
                  outs=dict(dw=("f32", (leaves, Sp, Cout, g.taps, Cin)), db=("f32", (leaves, Sp, Cout))), guard=dict(dz=128 * Cout, x=128 * Cin))


@case("isx_relu_grad")
def _():
    n = 1028
    dy, y, _ = sm.relu_case(n)
    return S.Case(dict(dy=np.array(dy), y=np.array(y)), lambda L, p, st: L.isx_relu_grad(p.dy, p.y, n, p.dz, st), lambda a: dict(dz=sm.relu_grad(a.dy, a.y)),
                  outs=dict(dz=("f32", (n,))))


@case("isx_bn_fold_backward")
def _():
    taps, Cin, Sp, Cout = 9, 64, 3, sm.FOLD_COUT
    dwp, db = sm.fold_case(taps, Cin, 1, Sp)[:2]
    w, scale, mean, istd = sm.fold_params(taps, Cin)
    ref = lambda a: dict(zip(("gw", "gg", "gb"), sm.fold_backward(a.dwp, a.db, a.w, a.scale, a.mean, a.istd, taps)))
    return S.Case(dict(dwp=np.array(dwp), db=np.array(db), w=np.array(w), scale=np.array(scale), mean=np.array(mean), istd=np.array(istd)),
                  lambda L, p, st: L.isx_bn_fold_backward(p.dwp, p.db, 1, Sp, p.w, p.scale, p.mean, p.istd, Cout, Cin, taps, 0, 0, p.gw, p.gg, p.gb, st), ref,
                  outs=dict(gw=("f32", (1, Cout, Cin, taps)), gg=("f32", (1, Cout)), gb=("f32", (1, Cout))))


# ==== descriptor head training ======================================================================================================================
HEAD = (65, 64, 4256)                              # (M, N, K): S = 2 splits, 67 + 66 k-tiles


def _head_inputs():
    M, N, K = HEAD
    x, w, bias = hm.fwd_case(K)[:3]
    assert hm.splits(K)[0] == _lib().isx_head_linear_splits(K) == 2, "more than one split: the partials go through the workspace"
    return np.array(x[:M]), np.array(w[:N]), np.array(bias[:N])


@case("isx_head_linear_fwd", "splits")
def _():
    M, N, K = HEAD
    x, w, bias = _head_inputs()
    Mp = (M + 63) // 64 * 64
    xT = np.full((K, Mp), 1e30, F)                                           # padding columns: "any finite values"
    xT[:, :M] = x.T
    nbytes = 2 * Mp * N * 4
    return S.Case(dict(xT=xT, w=w, bias=bias), lambda L, p, st: L.isx_head_linear_fwd(p.xT, M, Mp, K, p.w, N, p.bias, p.y, p.ws, nbytes, st),
                  lambda a: dict(y=hm.linear_fwd(np.ascontiguousarray(a.xT[:, :M].T), a.w, a.bias)), outs=dict(y=("f32", (M, N))), ws=dict(ws=nbytes))


@case("isx_head_linear_fwd_rows", "splits")
def _():
    M, N, K = HEAD
    x, w, bias = _head_inputs()
    nbytes = _lib().isx_head_linear_rows_workspace(M, K, N)
    assert nbytes >= 2 * M * N * 4
    return S.Case(dict(x=x, w=w, bias=bias), lambda L, p, st: L.isx_head_linear_fwd_rows(p.x, M, K, p.w, N, p.bias, p.y, p.ws, nbytes, st),
                  lambda a: dict(y=hm.linear_fwd(a.x, a.w, a.bias)), outs=dict(y=("f32", (M, N))), ws=dict(ws=nbytes))


def _dyT(dy):
    M, N = dy.shape
    t = np.zeros((N, (M + 63) // 64 * 64), F)
    t[:, :M] = dy.T
    return t


@case("isx_head_linear_dgrad", "groups")
def _():
    N, K, M = 256, 64, 24
    dy, w, _, _ = hm.dgrad_case(N, K, M)
    assert hm.groups(N) == _lib().isx_head_groups(N) == 8
    Mp = 64

    def ref(a):
        dx = np.zeros((Mp, K), F)
        dx[:M] = hm.dgrad(np.ascontiguousarray(a.dyT[:, :M].T), a.w)
        return dict(dx=dx)
    return S.Case(dict(dyT=_dyT(dy), w=np.array(w)), lambda L, p, st: L.isx_head_linear_dgrad(p.dyT, Mp, N, p.w, K, p.dx, st), ref, outs=dict(dx=("f32", (Mp, K))))


@case("isx_head_linear_dgrad_parts", "groups")
def _():
    Ng, Gr, K, M = hm.PARTS_EXTRA
    dy, w, _ = hm.parts_extra_case()
    assert Gr > 1
    Mp = 64

    def ref(a):
        parts = np.zeros((Gr, Mp, K), F)
        parts[:, :M] = hm.dgrad_parts(np.ascontiguousarray(a.dyT[:, :M].T), a.w, Ng)
        return dict(parts=parts)
    return S.Case(dict(dyT=_dyT(dy), w=np.array(w)), lambda L, p, st: L.isx_head_linear_dgrad_parts(p.dyT, Mp, Ng, Gr, p.w, K, p.parts, st), ref,
                  outs=dict(parts=("f32", (Gr, Mp, K))))


SGD = hm.SGD_SETS[3]                               # momentum_decay


@case("isx_head_sgd_step")
def _():
    """A second step (first = 0): the weight AND the momentum buffer are read and updated in place; both arrive with the late producer."""
    N, K, R = 192, 384, 33
    _, lr, mom, damp, wd, nest = SGD
    dy, x, _ = hm.rows_case(N, K, R, seed=1)
    w0, m0 = hm.sgd_w0(N, K), hm.inputs(N, K, 6, special_rows=False)
    ref = lambda a: dict(zip(("w", "mom"), hm.sgd_step(a.w, a.mom, hm.wgrad_rows(a.dy, a.x), False, lr, mom, damp, wd, nest)))
    return S.Case(dict(dy=np.array(dy), x=np.array(x), w=np.array(w0), mom=np.array(m0)),
                  lambda L, p, st: L.isx_head_sgd_step(p.dy, p.x, R, N, K, p.w, p.mom, 0, lr, mom, damp, wd, nest, st), ref, io=("w", "mom"))


@case("isx_colsum_leaves")
def _():
    Lv, R, C = 3, 5, 7
    x, _ = hm.colsum_case(Lv, R, C)
    return S.Case(dict(x=np.array(x)), lambda L, p, st: L.isx_colsum_leaves(p.x, Lv, R, C, p.out, st), lambda a: dict(out=hm.colsum_leaves(a.x, Lv, R)),
                  outs=dict(out=("f32", (Lv, C))))


def _tree_ref(rows):
    import test_gpu_eval_guards as EG
    return EG._tree_ref(rows)


@case("isx_tree_sum_rows", "in_place")
def _():
    Lr, n = 7, 1027
    rng = np.random.default_rng(n)
    rows = (rng.standard_normal((Lr, n)) * 10.0 ** rng.integers(-3, 4, (Lr, n))).astype(F)

    def ref(a):
        out = a.rows.copy()
        out[0] = _tree_ref(a.rows)
        return dict(rows=out)
    return S.Case(dict(rows=rows), lambda L, p, st: L.isx_tree_sum_rows(p.rows, Lr, n, n, p.rows, st), ref, io=("rows",))


# ==== the Python layer: wrappers under torch.cuda.stream(S) =========================================================================================
def ops_case(name):
    return case(name, level="ops")


@ops_case("gap_l2")
def _():
    from isx import ops
    f = dm.map_case(3, 24, 7, 7)
    return S.Case(dict(f=np.array(f)), lambda r: (ops.gap_l2(r.f.body, out=r.y.body), None)[1], lambda a: dict(y=dm.gap_l2(a.f)), outs=dict(y=("f32", (3, 24))), level="ops")


@ops_case("cosine_sim")
def _():
    from isx import ops
    M, N, D = 33, 129, 17
    rng = _rng(M, N, D, 1)
    Q, Gm = _unit(rng, M, D), _unit(rng, N, D)
    return S.Case(dict(q=Q, g=Gm), lambda r: (ops.cosine_sim(r.q.body, r.g.body, out=r.sim.body), None)[1], lambda a: dict(sim=O.cosine_sim(a.q, a.g)),
                  outs=dict(sim=("f32", (M, N))), level="ops")


@ops_case("search_sequence")
def _():
    """bench.py's search(): gap_l2(out=) -> cosine_sim(out=) -> topk_rows per shard -> topk_merge, every launch on the current stream."""
    from isx import ops
    M, C, N, k = 9, 64, 600, 5
    f = dm.map_case(M, C, 7, 7)
    Gm = _unit(_rng(N), N, C)
    Gm[500] = Gm[20]

    def call(r):
        q = ops.gap_l2(r.f.body, out=r.q.body)
        lists = []
        for lo in (0, N // 2):
            sim = ops.cosine_sim(q, r.g.body[lo:lo + N // 2], out=r.sim.body)
            lists.append(ops.topk_rows(sim, k, idx_base=lo))
        ts, ti = ops.topk_merge(torch.stack([l[0] for l in lists]), torch.stack([l[1] for l in lists]))
        return dict(ts=ts, ti=ti)

    def ref(a):
        q = dm.gap_l2(a.f)
        parts = [O.topk_rows(O.cosine_sim(q, a.g[lo:lo + N // 2]), k, idx_base=lo) for lo in (0, N // 2)]
        s, i = O.topk_merge(np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]))
        return dict(q=q, sim=O.cosine_sim(q, a.g[N // 2:]), ts=s, ti=np.ascontiguousarray(i, np.int64))
    return S.Case(dict(f=np.array(f), g=Gm), call, ref, outs=dict(q=("f32", (M, C)), sim=("f32", (M, N // 2))), level="ops")


@ops_case("cosine_topk_ws")
def _():
    from isx import ops
    M, N, D, k = 9, 3000, 32, 6
    Q, Gm = _search_data((M, N, D, k), 3)
    nbytes = G.topk_fixed_bytes(M, k) + 4 * M * (1024 + 128)                   # a caller's workspace of three chunks
    assert len(G.topk_chunks(M, N, k, nbytes, False)) >= 2

    def call(r):
        ts, ti = ops.cosine_topk(r.q.body, r.g.body, k, idx_base=IDX_BASE, ws=r.ws.body)
        return dict(ts=ts, ti=ti)
    return S.Case(dict(q=Q, g=Gm), call, _topk_ref(k), ws=dict(ws=nbytes), level="ops")


@ops_case("head_linear")
def _():
    from isx import ops
    x, w, bias = _head_inputs()
    return S.Case(dict(x=x, w=w, bias=bias), lambda r: dict(y=ops.head_linear(r.x.body, r.w.body, r.bias.body)), lambda a: dict(y=hm.linear_fwd(a.x, a.w, a.bias)),
                  level="ops")


@ops_case("affine_noisy_host_parameters")
def _():
    """mats, noise ids and rows on the HOST (one pinned block, one asynchronous copy); the cached mean | std constant dropped first, so that it is
    created under the side stream, behind the delay."""
    from isx import ops
    am, ta, img, rows, mat, ids = _affine_inputs()

    def call(r):
        ops._MEAN_STD.clear()
        out, u8 = ops.affine_noisy(r.img.body, rows, mat, ta.SEED, ids, MEAN, STD, channels_last=True, want_u8=True)
        return dict(f32=out.permute(0, 2, 3, 1), u8=u8)
    host = types.SimpleNamespace(rows=rows, mat=mat, ids=ids, mean=np.array(MEAN, F), std=np.array(STD, F))
    model = _affine_ref(am, ta.SEED, True)
    return S.Case(dict(img=img), call, lambda a: model(types.SimpleNamespace(img=a.img, **vars(host))), level="ops")


@ops_case("normalise_u8_batch")
def _():
    from train import _common
    img = _rng(6).integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)

    def call(r):
        old = dict(_common.RAW_INGEST)
        _common.RAW_INGEST.update(mean=MEAN, std=STD)
        try:
            return dict(out=_common.normalise_u8_batch(r.img.body, torch.cuda.current_device()).permute(0, 2, 3, 1))
        finally:
            _common.RAW_INGEST.update(old)
    return S.Case(dict(img=img), call, lambda a: dict(out=_nhwc(O.images_u8_to_f32(a.img, MEAN, STD))), level="ops")


@ops_case("suffix_conv1x1")
def _():
    """isx/suffix.py fetches the current stream itself: SuffixEngine._conv1x1, the smallest of its ctypes calls."""
    from isx.suffix import SuffixEngine
    B, Hh, W, Cin, Cout = 2, 3, 3, 64, 64
    rng = _rng(B, Cin, Cout)
    x, w, b = np.maximum(_normal(rng, B, Hh, W, Cin), 0), _normal(rng, Cout, Cin) * F(Cin ** -0.5), _normal(rng, Cout)

    def call(r):
        f = types.SimpleNamespace(cin=Cin, cout=Cout, w_fwd=r.w.body, bias=r.b.body)
        return dict(y=SuffixEngine._conv1x1(r.x.body, f, None, True))
    return S.Case(dict(x=x, w=w, b=b), call, lambda a: dict(y=O.conv1x1_nhwc(a.x.reshape(-1, Cin), a.w, a.b, None, True).reshape(B, Hh, W, Cout)), level="ops")


@ops_case("dp_weight_gradient_from_rows")
def _():
    from isx import dp
    N, K, R = 64, 128, 24
    dy, x, _ = hm.rows_case(N, K, R)
    assert _lib().isx_conv_wgrad_splits(R, K, N, 1) == 1, "the shape must take the libisx kernel, not torch's GEMM"
    return S.Case(dict(dy=np.array(dy), x=np.array(x)), lambda r: dict(g=dp.weight_gradient_from_rows(r.dy.body, r.x.body)),
                  lambda a: dict(g=hm.wgrad_rows(a.dy, a.x)), level="ops")


@ops_case("shard_head_sgd_update_rows")
def _():
    """tests/test_gpu_head_chains.py::test_head_sgd_step_on_a_shard...: rows [64, 128) of a (192, K) weight, first step; the other rows keep their bits."""
    from isx import shard_head
    lo, hi, N, K, R = 64, 128, 192, 128, 24
    _, lr, mom, damp, wd, nest = SGD
    dy, x, _ = hm.rows_case(N, K, R, seed=0)

    def call(r):
        w = torch.nn.Parameter(r.w.body)
        opt = torch.optim.SGD([w], lr=lr, momentum=mom, dampening=damp, weight_decay=wd, nesterov=bool(nest))
        shard_head.sgd_update_rows(opt, w, r.dy.body[:, lo:hi].contiguous(), r.x.body, lo, hi, 64)
        return dict(mom=opt.state[w]["momentum_buffer"][lo:hi])

    def ref(a):
        ws, buf = hm.sgd_step(a.w[lo:hi], None, hm.wgrad_rows(a.dy[:, lo:hi], a.x), True, lr, mom, damp, wd, nest)
        w = a.w.copy()
        w[lo:hi] = ws
        return dict(w=w, mom=buf)
    return S.Case(dict(dy=np.array(dy), x=np.array(x), w=np.array(hm.sgd_w0(N, K))), call, ref, io=("w",), level="ops")


@ops_case("sharded_gallery_local_search_twice")
def _():
    """Two searches in a row on S: the first converts the gallery (cached fp16 image), allocates the cached workspace and starts the asynchronous
    read of the fallback counter; the second reuses all three.  Both lists are the unsharded oracle's."""
    from isx import retrieval
    M, N, D, k = 16, 4096, 64, 10
    Q, Gm = _search_data((M, N, D, k), 4)

    def call(r):
        gal = retrieval.ShardedGallery(r.g.body, idx_base=IDX_BASE)
        assert gal.fast
        a = gal.local_search(r.q.body, k)
        b = gal.local_search(r.q.body, k)
        assert gal._f16 is not None and gal.fast
        return dict(ts=a[0], ti=a[1], ts2=b[0], ti2=b[1])

    def ref(a):
        s, i = O.cosine_topk(a.q, a.g, k, idx_base=IDX_BASE)
        i = np.ascontiguousarray(i, np.int64)
        return dict(ts=s, ti=i, ts2=s, ti2=i)
    return S.Case(dict(q=Q, g=Gm), call, ref, level="ops")


# ==== the tests =====================================================================================================================================
def stream_entries():
    """Names of the prototypes of include/isx.h whose last parameter is `isx_stream_t stream`."""
    text = open(os.path.join(ROOT, "include", "isx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(isx_\w+)\s*\([^;{}]*?isx_stream_t\s+stream\s*\)\s*;", text)))


def test_every_stream_taking_entry_has_a_case():
    names = stream_entries()
    assert len(names) >= 70 and "isx_l2norm_rows" in names and "isx_tree_sum_rows" in names and "isx_version" not in names, names
    tabled = {entry for _, entry, _ in TABLE if entry.startswith("isx_")}
    assert not tabled & set(NOT_HERE), sorted(tabled & set(NOT_HERE))
    header = open(os.path.join(ROOT, "include", "isx.h")).read()
    for n, reason in NOT_HERE.items():                                       # an exception is a stream-taking entry, or one the header documents as blocking
        assert n in names or (re.search(r"\b%s\(" % n, header) and "Synchronises the device" in reason and "Synchronises the device" in header), n
    missing = [n for n in names if n not in tabled and n not in NOT_HERE]
    assert not missing, ("stream-taking entries with neither a case nor a reason", missing)
    assert all(isinstance(r, str) and len(r) > 20 for r in NOT_HERE.values())
    assert tabled <= set(names), sorted(tabled - set(names))
    ids = [i for i, _, _ in TABLE]
    assert len(ids) == len(set(ids)) and len(ids) < 120


_BUILT = {}
_PLAIN_FAILED = {}


def _built(cid):
    """A case is built once per process (its operands and the closures of its references), and torn down with the module."""
    if cid not in _BUILT:
        _BUILT[cid] = next(b for i, _, b in TABLE if i == cid)()
    return _BUILT[cid]


@pytest.fixture(scope="module")
def delay():
    """The delay of every case of this file: 20 x the slowest host-side call, measured on the DEFAULT stream at the file's own shapes (second call of
    every case: the first loads the kernels), and not less than 20 ms; in cycles of torch.cuda._sleep, calibrated with two events on an idle GPU."""
    t0 = time.perf_counter()
    slowest, who = 0.0, None
    for cid, _, _ in TABLE:
        try:
            took = _built(cid).run_plain()
        except AssertionError as e:                                          # a wrong result: reported by the case's own test, the pass goes on
            _PLAIN_FAILED[cid] = e
            continue
        except Exception as e:                                               # anything else may be the device: nothing more is launched
            _PLAIN_FAILED[cid] = e
            aborted = RuntimeError("default-stream pass aborted at %s: %r" % (cid, e))
            for later in [i for i, _, _ in TABLE][[i for i, _, _ in TABLE].index(cid) + 1:]:
                _PLAIN_FAILED[later] = aborted
            yield None
            _BUILT.clear()
            _PLAIN_FAILED.clear()
            return
        if took > slowest:
            slowest, who = took, cid
    rate = S.sleep_cycles_per_second()
    cycles, seconds = S.delay_cycles(slowest, rate)
    print("stream order: slowest host-side call %.3f ms (%s); delay %.1f ms = %d cycles at %.1f MHz; default-stream pass of %d cases %.1f s"
          % (slowest * 1e3, who, seconds * 1e3, cycles, rate * 1e-6, len(TABLE), time.perf_counter() - t0))
    yield cycles
    _BUILT.clear()
    _PLAIN_FAILED.clear()


@gpu
@pytest.mark.parametrize("cid", [i for i, _, _ in TABLE])
def test_behind_a_late_producer(cid, delay):
    if cid in _PLAIN_FAILED:
        raise AssertionError("the case fails on the default stream already: %r" % (_PLAIN_FAILED[cid],)) from _PLAIN_FAILED[cid]
    c = _built(cid)
    assert delay is not None, "default-stream pass aborted"
    took = c.run_late(delay)
    print("%s: host call %.3f ms behind the late producer" % (cid, took * 1e3))


@pytest.fixture
def drained():
    """Whatever a test below leaves on its side streams has completed before its tensors go back to the allocator, also when it fails."""
    yield
    torch.cuda.synchronize()


# ---- device buffers the Python layer keeps between calls ----------------------------------------------------------------------------------------
def _ranges_overlap(a, b):
    return a[0] < b[0] + b[1] and b[0] < a[0] + a[1]


@gpu
def test_head_linear_under_two_streams_does_not_share_its_workspace(monkeypatch, drained):
    """ops.head_linear used to keep one split-K workspace per device.  Two calls issued under two different current streams must not be handed
    overlapping scratch memory unless the wrapper has ordered the second stream behind the first with an event wait."""
    from isx import ops
    x, w, bias = (torch.from_numpy(a).cuda() for a in _head_inputs())
    seen, waits = [], []
    real_call, real_wait = ops._call, torch.cuda.Stream.wait_event

    def call(name, *args):
        if name == "isx_head_linear_fwd_rows":
            seen.append((args[7], args[8], args[-1]))
        return real_call(name, *args)

    def wait_event(self, event):
        waits.append(self.cuda_stream)
        return real_wait(self, event)
    monkeypatch.setattr(ops, "_call", call)
    monkeypatch.setattr(torch.cuda.Stream, "wait_event", wait_event)
    torch.cuda.synchronize()
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(A):
        ya = ops.head_linear(x, w, bias)
    with torch.cuda.stream(B):
        yb = ops.head_linear(x, w, bias)
    torch.cuda.synchronize()
    (pa, na, sa), (pb, nb, sb) = seen
    assert (sa, sb) == (A.cuda_stream, B.cuda_stream) and sa != sb
    assert not _ranges_overlap((pa, na), (pb, nb)) or B.cuda_stream in waits, "two streams share one split-K workspace with nothing ordering them"
    want = hm.linear_fwd(*_head_inputs())
    G.assert_bits(ya, want)
    G.assert_bits(yb, want)


@gpu
def test_mean_std_constant_is_ordered_before_a_read_on_another_stream(monkeypatch, drained):
    """ops._mean_std_device caches a device constant.  Created under stream A (behind whatever A is doing), it must not be read under stream B
    before its copy has run: B waits for the creation event -- and a creation that blocks the host would show as `delay too short` in the
    affine_noisy case above."""
    from isx import ops
    waits = []
    real_wait = torch.cuda.Stream.wait_event

    def wait_event(self, event):
        waits.append(self.cuda_stream)
        return real_wait(self, event)
    monkeypatch.setattr(torch.cuda.Stream, "wait_event", wait_event)
    mean, std = (0.25, 0.5, 0.75), (0.5, 0.25, 0.125)
    dev = torch.device("cuda", torch.cuda.current_device())
    ops._MEAN_STD.clear()
    torch.cuda.synchronize()
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    cycles = int(S.MIN_DELAY_S * S.sleep_cycles_per_second())
    with torch.cuda.stream(A):
        torch.cuda._sleep(cycles)
        ta = ops._mean_std_device(mean, std, dev)
        created = torch.cuda.Event()
        created.record(A)
    with torch.cuda.stream(B):
        tb = ops._mean_std_device(mean, std, dev)
        got = tb.clone()                                                     # a read on B
    assert not created.query(), "delay too short: A had created the constant before B asked for it"
    assert ta.data_ptr() == tb.data_ptr(), "one cached constant"
    assert B.cuda_stream in waits, "stream B reads the constant with nothing ordering it behind its creation on stream A"
    B.synchronize()
    assert got.cpu().tolist() == [float(np.float32(v)) for v in mean + std]
    torch.cuda.synchronize()
    with torch.cuda.stream(B):                                               # once the creation has completed nobody waits any more
        n = len(waits)
        ops._mean_std_device(mean, std, dev)
        assert len(waits) == n
    ops._MEAN_STD.clear()


@gpu
def test_sharded_gallery_orders_a_second_stream_behind_the_first(monkeypatch, drained):
    """ShardedGallery keeps a workspace, the fp16 image of its shard and the fallback counter's event between searches: a search under another
    stream than the previous one waits for that one's last launch."""
    from isx import retrieval
    waits = []
    real_wait = torch.cuda.Stream.wait_event

    def wait_event(self, event):
        waits.append(self.cuda_stream)
        return real_wait(self, event)
    monkeypatch.setattr(torch.cuda.Stream, "wait_event", wait_event)
    M, N, D, k = 16, 4096, 64, 10
    Q, Gm = _search_data((M, N, D, k), 4)
    want = O.cosine_topk(Q, Gm, k, idx_base=IDX_BASE)
    q, g = torch.from_numpy(Q).cuda(), torch.from_numpy(Gm).cuda()
    gal = retrieval.ShardedGallery(g, idx_base=IDX_BASE)
    torch.cuda.synchronize()
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    cycles = int(S.MIN_DELAY_S * S.sleep_cycles_per_second())
    with torch.cuda.stream(A):
        torch.cuda._sleep(cycles)
        ra = gal.local_search(q, k)
        done = torch.cuda.Event()
        done.record(A)
        assert A.cuda_stream not in waits, "the first search has nothing to wait for"
        n = len(waits)
        gal.local_search(q, k)
        assert len(waits) == n, "the same stream again: stream order is enough"
    with torch.cuda.stream(B):
        rb = gal.local_search(q, k)
    assert not done.query(), "delay too short"
    assert B.cuda_stream in waits, "a search on stream B shares the workspace and the fp16 gallery of the search still pending on stream A"
    torch.cuda.synchronize()
    for s, i in (ra, rb):
        G.assert_bits(s, want[0])
        np.testing.assert_array_equal(i.cpu().numpy(), want[1])


@gpu
def test_tree_exchange_refuses_a_second_stream(drained):
    """TreeExchange reuses one padded staging buffer and nothing orders two streams on it: the object belongs to the stream of its first device
    call (its docstring) and refuses any other, before anything is enqueued -- also at a world size of one, where the check is all that runs."""
    from isx import dp
    from isx._lib import IsxError
    ex = dp.TreeExchange()
    flat = torch.arange(8, dtype=torch.float32, device="cuda")
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(A):
        assert ex.allreduce_(flat) is flat
        assert ex.allreduce_(flat) is flat                                   # the same stream again
    with torch.cuda.stream(B):
        with pytest.raises(IsxError, match="belongs to stream"):
            ex.allreduce_(flat)
    with pytest.raises(IsxError, match="belongs to stream"):               # the default stream is another stream too
        ex.allreduce_(flat)
    with torch.cuda.stream(A):
        assert ex.allreduce_(flat) is flat                                   # a refusal changes nothing
    assert dp.TreeExchange().allreduce_(torch.zeros(4)).tolist() == [0.0] * 4   # host buffers have no stream
    assert flat.cpu().tolist() == list(range(8))


@gpu
def test_load_slab_under_two_streams(tmp_path, drained):
    """slab._STAGE (two pinned staging buffers kept for the process) belongs to load_slab, which drains the device before it returns (its
    docstring): a second load under another stream finds both buffers free.  Two loads in a row under two streams give the file's rows."""
    from isx import slab
    rows = _normal(_rng(8), 300, 16)
    path = str(tmp_path / "g.slab")
    slab.save_slab(path, torch.from_numpy(rows))
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(A):
        a, _ = slab.load_slab(path, "cuda", rows=(0, 200))
        assert A.query(), "load_slab returns with its copies done: the staging buffers are free"
    with torch.cuda.stream(B):
        b, _ = slab.load_slab(path, "cuda", rows=(100, 300))
        assert B.query()
    G.assert_bits(a, rows[:200])
    G.assert_bits(b, rows[100:])
