"""The argument contract of isx/ops.py, on CPU tensors: neither libisx nor a GPU is touched.

Every wrapper checks what tensor metadata decides (rank, dtype, shapes, lengths, memory layout) BEFORE device residency, so a call built from
CPU tensors of the smallest legal shapes is refused with "CUDA" exactly when everything else is right (GOOD), and with a message that opens
with the name of the one wrong argument otherwise (BAD).  libisx sees raw pointers: each BAD row is a buffer the kernel would have read or
written past its end."""
import ast
import inspect
import re

import pytest
import torch

from isx import ops
from isx._lib import IsxError


def f(*shape):
    return torch.zeros(shape)


def cl(*shape):
    return torch.zeros(shape).contiguous(memory_format=torch.channels_last)


def typed(dtype):
    return lambda *shape: torch.zeros(shape, dtype=dtype)


i64, i32, u8, h, f64 = (typed(d) for d in (torch.int64, torch.int32, torch.uint8, torch.float16, torch.float64))
UNIT = dict(mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0))
REGION = dict(fmap=lambda: cl(1, 4, 2, 2), kh=1, kw=1, flat_idx=lambda: i64(1, 1), Wp=2)
SIM = dict(sim=lambda: f(2, 3), qlab=lambda: i32(2), glab=lambda: i32(3))
QG = dict(Q=lambda: f(2, 8), G=lambda: f(3, 8))
TOPK = dict(QG, k=2, ws=lambda: u8(16), out=lambda: (f(2, 2), i64(2, 2)))
TRIPLET = dict(anchor=lambda: f(2, 4), pos=lambda: f(2, 4), neg=lambda: f(2, 4))
XENT = dict(logits=lambda: f(2, 3), labels=lambda: i64(2))

# wrapper -> its smallest legal call (a callable value is built per test, so no row sees another's tensors)
GOOD = {
    "l2norm_rows": dict(x=lambda: f(2, 4), out=lambda: f(2, 4)),
    "l2norm_rows_bwd": dict(x=lambda: f(2, 4), dy=lambda: f(2, 4)),
    "l2norm_shift_rows": dict(x=lambda: f(2, 4), shift=lambda: f(4)),
    "head_linear": dict(rows=lambda: f(1, 32), weight=lambda: f(64, 32), bias=lambda: f(64)),
    "gap_l2": dict(fmap=lambda: cl(2, 4, 3, 3), out=lambda: f(2, 4)),
    "bias_act_": dict(y=lambda: cl(1, 4, 2, 2), bias=lambda: f(4), residual=lambda: cl(1, 4, 2, 2)),
    "images_u8_to_f32": dict(UNIT, img_u8=lambda: u8(1, 2, 2, 3)),
    "affine_noisy": dict(UNIT, img_u8=lambda: u8(1, 2, 2, 3), rows=None, mats=[[1, 0, 0, 0, 1, 0]], seed=0, noise_ids=[0]),
    "bias_relu_maxpool": dict(y=lambda: cl(1, 4, 2, 2), bias=lambda: f(4)),
    "stem7x7_pool": dict(x=lambda: cl(1, 3, 8, 8), w_ohwi=lambda: f(64, 7, 7, 3), bias=lambda: f(64)),
    "conv1x1_nhwc": dict(x=lambda: cl(1, 4, 2, 2), weight=lambda: f(8, 4, 1, 1), bias=lambda: f(8), residual=lambda: cl(1, 8, 2, 2)),
    "conv1x1_dual_nhwc": dict(t=lambda: cl(1, 32, 2, 2), x=lambda: cl(1, 32, 2, 2), w_cat=lambda: f(8, 64), bias=lambda: f(8)),
    "conv3x3_nhwc": dict(x=lambda: cl(1, 32, 2, 2), w_ohwi=lambda: f(8, 3, 3, 32), bias=lambda: f(8), residual=lambda: cl(1, 8, 2, 2)),
    "conv3x3_expand_nhwc": dict(x=lambda: cl(1, 32, 2, 2), w2_ohwi=lambda: f(64, 3, 3, 32), b2=lambda: f(64), stride=1, w3t=lambda: f(64, 256),
                                b3=lambda: f(256), residual=lambda: cl(1, 256, 2, 2)),
    "conv3x3_expand128_nhwc": dict(x=lambda: cl(1, 64, 2, 2), w2_ohwi=lambda: f(128, 3, 3, 64), b2=lambda: f(128), w3t=lambda: f(128, 128),
                                   b3=lambda: f(128), residual=lambda: cl(1, 128, 2, 2)),
    "conv3x3_expand_dual_nhwc": dict(t=lambda: cl(1, 32, 2, 2), w2_ohwi=lambda: f(64, 3, 3, 32), b2=lambda: f(64), x2=lambda: cl(1, 64, 2, 2),
                                     wcat_t=lambda: f(128, 256), bias=lambda: f(256)),
    "boxpool_s1": dict(fmap=lambda: f(1, 4, 2, 2), kh=1, kw=1),
    "boxpool_s1_nhwc": dict(fmap=lambda: cl(1, 4, 2, 2), kh=1, kw=1),
    "best_location_desc": dict(cls=lambda: f(1, 2, 2, 2)),
    "region_topk": dict(cls=lambda: f(1, 2, 2, 2), k=1),
    "region_gather_l2_nhwc": dict(REGION, shift_hwc=lambda: f(4)),
    "region_sum_l2_nhwc": dict(REGION, shift=lambda: f(4)),
    "region_sum_l2_bwd_nhwc": dict(REGION, g=lambda: f(1, 4), n2=lambda: f(1, 1), add=lambda: cl(1, 4, 2, 2)),
    "region_gather_l2": dict(REGION, fmap=lambda: f(1, 4, 2, 2), shift=lambda: f(4)),
    "cosine_sim": dict(QG, out=lambda: f(2, 3)),
    "cosine_topk": TOPK,
    "gallery_to_f16": dict(G=lambda: f(3, 8)),
    "cosine_topk_fast": dict(TOPK, gallery_f16=lambda: (h(3, 8), f(4))),
    "topk_rows": dict(sim=lambda: f(2, 3), k=2),
    "rank_full": dict(sim=lambda: f(2, 3)),
    "average_precision": dict(SIM, sim=None, ranked=lambda: i64(2, 3)),
    "average_precision_sim": SIM,
    "ap_shard_positives": dict(SIM, idx_base=0, cap=4),
    "ap_shard_hist": dict(sim=lambda: f(2, 3), idx_base=0, keys_all=lambda: i64(2, 4)),
    "ap_from_hist": dict(hist=lambda: i32(2, 4), n_lab=lambda: i32(2)),
    "masked_sums": SIM,
    "tree_sum_rows": dict(rows=lambda: f(2, 4), out=lambda: f(4)),
    "dba_groups": dict(emb=lambda: f(3, 8), order=lambda: i32(3), grp_begin=lambda: i32(3), grp_size=lambda: i32(3), max_group=1),
    "topk_merge": dict(scores=lambda: f(2, 2, 2), idx=lambda: i64(2, 2, 2)),
    "shard_topk_allgather": dict(comm=0, nranks=1, s_local=lambda: f(2, 2), i_local=lambda: i64(2, 2)),
    "comm_allgather_rows": dict(comm=0, nranks=1, rows_local=lambda: f(2, 4), out=lambda: f(2, 4)),
    "mine_negatives": dict(sim=lambda: f(3, 3), labels=lambda: i32(3), i1=lambda: i64(2), i2=lambda: i64(2), semi_hard=True),
    "triplet_loss_rows": dict(TRIPLET, margin=0.1),
    "triplet_loss_grads": dict(TRIPLET, loss_rows=lambda: f(2), scale=1.0, scale_dev=lambda: f(1)),
    "triplet_leaves": dict(d_all=lambda: f(3, 4), leaves=1, margin=0.1),
    "softmax_xent_rows": XENT,
    "softmax_xent_grad": dict(XENT, scale_dev=lambda: f(1)),
    "softmax_xent_leaves": dict(XENT, leaves=1),
    "gap_bwd_nhwc": dict(g=lambda: f(2, 4), H=2, W=2),
    "boxpool_s1_bwd_nhwc": dict(g=lambda: cl(1, 4, 2, 2), H=2, W=2, kh=1, kw=1),
    "linear_wgrad_leaves": dict(dy=lambda: f(2, 3), x=lambda: f(2, 4), leaves=1),
    "colsum_leaves": dict(x=lambda: f(2, 3), leaves=1),
    "head_linear_dgrad": dict(dy=lambda: f(2, 3), weight=lambda: f(3, 4)),
    "rows_to_f16": dict(x=lambda: f(2, 8)),
    "cosine_sim_f16": dict(Qh=lambda: h(2, 8), Gh=lambda: h(3, 8), out=lambda: f(2, 3)),
}
# public functions that take no tensor to check: predicates, workspace sizes, host-side communicator set-up, wrappers of other wrappers
NO_CONTRACT = {"check", "lib", "head_linear_applicable", "pad_rows_to_64", "head_linear_any", "stem7x7_pool_applicable", "boxpool_s1_applicable_nhwc",
               "cosine_topk_workspace", "cosine_topk_fast_workspace", "cosine_topk_fast_fallback_counter", "ap_shard_max_positives",
               "comm_unique_id", "comm_init_rank", "comm_destroy"}


def call(wrapper, **override):
    kw = {k: v for k, v in dict(GOOD[wrapper], **override).items() if not (k == "sim" and v is None)}
    return getattr(ops, wrapper)(**{k: v() if callable(v) else v for k, v in kw.items()})


def rows(wrappers, args, bad, named=None):
    """One BAD row per (wrapper, argument): the argument replaced by bad(); `named`: how the message names it when not by the argument."""
    return [(w, a, bad, named or a) for w in wrappers.split() for a in args.split()]


OUT_PAIR = "cosine_topk cosine_topk_fast"
NHWC_CONVS = "conv1x1_nhwc conv3x3_nhwc conv3x3_expand_nhwc conv3x3_expand128_nhwc"
BAD = (
    # per-channel / per-row vectors shorter than the kernel reads
    rows("bias_relu_maxpool stem7x7_pool conv1x1_nhwc conv1x1_dual_nhwc conv3x3_nhwc conv3x3_expand_dual_nhwc bias_act_ head_linear", "bias", lambda: f(3))
    + rows("conv3x3_expand_nhwc conv3x3_expand128_nhwc", "b2 b3", lambda: f(63)) + rows("conv3x3_expand_dual_nhwc", "b2", lambda: f(63))
    + rows("l2norm_shift_rows region_gather_l2 region_sum_l2_nhwc", "shift", lambda: f(3)) + rows("region_gather_l2_nhwc", "shift_hwc", lambda: f(3))
    # companion operands that do not match the first
    + rows("triplet_loss_rows triplet_loss_grads", "pos neg", lambda: f(1, 4)) + rows("triplet_loss_grads", "loss_rows", lambda: f(1))
    + rows("topk_merge", "idx", lambda: i64(2, 2, 1)) + rows("shard_topk_allgather", "i_local", lambda: i64(2, 1))
    + rows("mine_negatives", "i2", lambda: i64(1)) + rows("mine_negatives", "labels", lambda: i32(2))
    + rows("average_precision average_precision_sim masked_sums ap_shard_positives", "qlab", lambda: i32(1))
    + rows("average_precision average_precision_sim masked_sums ap_shard_positives", "glab", lambda: i32(2))
    + rows("ap_from_hist", "n_lab", lambda: i32(1)) + rows("ap_shard_hist", "keys_all", lambda: i64(1, 4))
    + rows("dba_groups", "order grp_begin grp_size", lambda: i32(2))
    + rows("region_sum_l2_bwd_nhwc", "g", lambda: f(1, 3)) + rows("region_sum_l2_bwd_nhwc", "n2", lambda: f(1, 2))
    + rows("region_gather_l2_nhwc region_sum_l2_nhwc region_gather_l2", "flat_idx", lambda: i64(2, 1))
    # caller-supplied outputs: one row short, another dtype, a strided view -- never copied, always refused
    + rows("l2norm_rows gap_l2 comm_allgather_rows", "out", lambda: f(1, 4)) + rows("cosine_sim cosine_sim_f16", "out", lambda: f(1, 3))
    + rows("l2norm_rows gap_l2", "out", lambda: f64(2, 4)) + rows("cosine_sim cosine_sim_f16", "out", lambda: f64(2, 3))
    + rows("l2norm_rows gap_l2", "out", lambda: f(2, 8)[:, ::2]) + rows("cosine_sim cosine_sim_f16", "out", lambda: f(2, 6)[:, ::2])
    + rows("tree_sum_rows", "out", lambda: f(3)) + rows("tree_sum_rows", "out", lambda: f64(4)) + rows("tree_sum_rows", "out", lambda: f(8)[::2])
    + rows(OUT_PAIR, "out", lambda: (f(1, 2), i64(2, 2)), "out[0]") + rows(OUT_PAIR, "out", lambda: (f(2, 2), i64(1, 2)), "out[1]")
    + rows(OUT_PAIR, "out", lambda: (f64(2, 2), i64(2, 2)), "out[0]") + rows(OUT_PAIR, "out", lambda: (f(2, 2), i32(2, 2)), "out[1]")
    + rows(OUT_PAIR, "out", lambda: (f(2, 4)[:, ::2], i64(2, 2)), "out[0]") + rows(OUT_PAIR, "out", lambda: (f(2, 2), i64(2, 4)[:, ::2]), "out[1]")
    # workspaces are bytes: ws.numel() is what libisx is told
    + rows(OUT_PAIR, "ws", lambda: f(16)) + rows(OUT_PAIR, "ws", lambda: u8(4, 4)) + rows(OUT_PAIR, "ws", lambda: u8(32)[::2])
    + rows("cosine_topk_fast", "gallery_f16", lambda: (f(3, 8), f(4)), "gallery_f16[0]")
    + rows("cosine_topk_fast", "gallery_f16", lambda: (h(2, 8), f(4)), "gallery_f16[0]")
    + rows("cosine_topk_fast", "gallery_f16", lambda: (h(3, 8), f(3)), "gallery_f16[1]")
    + rows("cosine_sim cosine_topk cosine_topk_fast", "G", lambda: f(3, 7)) + rows("cosine_sim_f16", "Gh", lambda: h(3, 7))
    + rows("cosine_sim_f16", "Qh", lambda: f(2, 8))
    # NCHW memory where the kernel walks NHWC
    + rows(NHWC_CONVS + " conv1x1_dual_nhwc", "x", lambda: f(1, 64, 2, 2)) + rows("stem7x7_pool", "x", lambda: f(1, 3, 8, 8))
    + rows("conv1x1_dual_nhwc conv3x3_expand_dual_nhwc", "t", lambda: f(1, 32, 2, 2)) + rows("conv3x3_expand_dual_nhwc", "x2", lambda: f(1, 64, 2, 2))
    + rows("bias_relu_maxpool", "y", lambda: f(1, 4, 2, 2))
    + rows("boxpool_s1_nhwc region_gather_l2_nhwc region_sum_l2_nhwc region_sum_l2_bwd_nhwc", "fmap", lambda: f(1, 4, 2, 2))
    + rows("region_sum_l2_bwd_nhwc", "add", lambda: f(1, 4, 2, 2))
    # the residual: the output's shape and memory format
    + rows(NHWC_CONVS + " bias_act_", "residual", lambda: cl(1, 4, 3, 2)) + rows("conv1x1_nhwc conv3x3_nhwc", "residual", lambda: f(1, 8, 2, 2))
    + rows("conv3x3_expand_nhwc", "residual", lambda: f(1, 256, 2, 2)) + rows("conv3x3_expand128_nhwc", "residual", lambda: f(1, 128, 2, 2))
    + rows("bias_act_", "residual", lambda: f(1, 4, 2, 2)) + rows("bias_act_", "residual", lambda: f64(1, 4, 2, 2).contiguous(memory_format=torch.channels_last))
    + rows("images_u8_to_f32 affine_noisy", "img_u8", lambda: u8(1, 2, 2, 4))
)


def test_every_public_wrapper_has_a_row():
    public = {n for n, v in vars(ops).items() if inspect.isfunction(v) and not n.startswith("_")}
    assert public == set(GOOD) | NO_CONTRACT, sorted(public ^ (set(GOOD) | NO_CONTRACT))


@pytest.mark.parametrize("wrapper", sorted(GOOD))
def test_device_check_is_there_and_comes_last(wrapper):
    with pytest.raises(IsxError, match="CUDA"):
        call(wrapper)


@pytest.mark.parametrize("wrapper,arg,bad,named", BAD, ids=["%s-%s-%d" % (r[0], r[1], i) for i, r in enumerate(BAD)])
def test_one_wrong_argument_is_named(wrapper, arg, bad, named):
    with pytest.raises(IsxError, match=r"^%s (has|must) " % re.escape(named)) as e:
        call(wrapper, **{arg: bad})
    assert "CUDA" not in str(e.value)


def test_no_assert_statement_in_ops():
    """An argument check spelled `assert` disappears under python -O."""
    tree = ast.parse(inspect.getsource(ops))
    assert not [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Assert)]
