"""Every launching entry of include/isx.h on operands past 2^31 elements (over 8 GiB of fp32, and with it the 2 GiB and 4 GiB byte lines).

The library's own workloads stop just short of those lines, and the kernels are the kind that break there: 32-bit voffset / soffset values
relative to a per-tile 64-bit base, 0x80000000 as the "outside" mark, num_records clamped at 0xFFFFFFFF, hand-derived limits in the entries,
int64 grid-stride loops that no test has driven past 2^31.  Each case here (TABLE) gives one entry the smallest shape whose largest operand
just passes 2^31 elements, every other dimension at the minimum, and checks EVERY element of the output:

  - the crossing operands are tiled on the device from a small period block of random rows (tests/_large.py: an odd prime number of rows,
    images or leaves, so that no shift of 2^29 .. 2^34 elements is a multiple of the period, and at least 99 % of the block's positions differ
    from the one such a shift away -- asserted on the host for every operand, on the CPU too: test_every_period_holds_the_rules);
  - the expected output of ONE period comes from the entry's existing CPU reference (oracle/oracle.py, tests/_*_model.py), compared as the
    entry's own GPU tests compare it: bit for bit;
  - outputs start as poison between guards; after one launch the whole output is compared on the device, as integers, with the period's block
    broadcast over the repeats.  A failure names the count of wrong elements, the first and last wrong flat index and those modulo 2^29, 2^30, 2^31.

tests/test_large_model.py proves on the CPU that this comparison flags wrapped loads, wrapped stores, an unwritten tail and a single wrong
element, and that it would NOT flag wrapped loads under a period that divides the modulus.  LIMITED names the stream-taking entries that
have no case here, each with the documented condition that keeps it from such sizes (test_every_stream_taking_entry_is_placed)."""
import os
import re
import types

import numpy as np
import pytest
import torch

import _desc_model as dm
import _guards as G
import _head_model as hm
import _large as LG
import _suffix_model as sm
import _triplet_model as tm
import _xent_model as xm
import oracle as O

F = np.float32
EPS = dm.EPS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
GB = 1 << 30
PEAK_BYTES = 48 * GB                               # no case may need more device memory than this

# stream-taking entries with no case in TABLE: the documented condition that keeps each from operands of this size
LIMITED = {
    "isx_comm_allgather_rows": "a collective over two or more GPUs (include/isx.h: 'OUTSIDE the contract: the isx_comm_* set-up calls ... and the two "
                               "collectives isx_comm_allgather_rows / isx_shard_topk_allgather'): tests/_rccl_worker.py runs it, one GPU cannot",
    "isx_shard_topk_allgather": "a collective over two or more GPUs (include/isx.h: 'OUTSIDE the contract: ... the two collectives "
                                "isx_comm_allgather_rows / isx_shard_topk_allgather'): tests/_rccl_worker.py runs it, one GPU cannot",
}

TABLE = []                                         # (id, entry, builder of the Case)


def case(entry, tag=None):
    def deco(fn):
        TABLE.append((entry.split("_", 1)[1] + ("_" + tag if tag else ""), entry, fn))
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


def _rows_past_line(row_elems, extra=0):
    """The smallest number of rows of row_elems elements whose total passes 2^31, plus `extra`."""
    return LG.LINE // row_elems + 1 + extra


class Out(object):
    """An output of `rows` rows of `row_shape`.  period: the rows of the expected block (the reference returns (period,) + row_shape), None: the
    reference returns the whole output (a small one).  own_period(first period of the output, want): for an entry whose existing test is a bound and
    not bits -- the bound is asserted on the first period, every later row must then repeat the device's own first period bit for bit."""
    def __init__(self, kind, rows, row_shape, period=None, guard=4096, own_period=None, parts=1):
        self.kind, self.rows, self.row_shape, self.period, self.guard, self.own_period, self.parts = kind, int(rows), tuple(row_shape), period, guard, own_period, parts
        self.shape = ((parts,) if parts > 1 else ()) + (self.rows,) + self.row_shape
        self.n = int(np.prod(self.shape))


class Case(object):
    """One entry at a size that crosses the line.
    ins    name -> LG.Periodic (tiled on the device) | host array (uploaded whole) | None (an optional operand left out)
    io     names of `ins` the entry updates in place: compared with ref()[name] afterwards
    outs   name -> Out
    ws     name -> bytes, or fn(L) -> bytes
    call   call(L, p, st) -> rc; p.<name>: device pointers
    ref    ref(a) -> {name: host array}; a.<name> is the PERIOD BLOCK of a Periodic operand, the array of a whole one
    hooks  (gemm, conv) debug settings around the call
    check  name -> fn(got, want): the comparison of the entry's existing test for an output that is not compared bit for bit (never a new tolerance)
    crossing  the operands (by name) that pass 2^31 elements: asserted"""
    def __init__(self, shape, ins, call, ref, outs=None, io=(), ws=None, hooks=None, crossing=(), guard=None, check=None, crossing_ws=None):
        self.shape, self.ins, self.call, self.ref, self.outs, self.io, self.ws = shape, ins, call, ref, outs or {}, tuple(io), ws or {}
        self.hooks, self.crossing, self.guard, self.check, self.crossing_ws = hooks, tuple(crossing), guard or {}, check or {}, crossing_ws
        assert self.crossing or crossing_ws, "a case names the operand that crosses the line (crossing_ws: a workspace, with the bytes it must pass)"
        for n in self.crossing:
            x = self.ins[n] if n in self.ins else self.outs[n]
            assert x.n > LG.LINE, (n, x.n, "does not pass 2^31 elements")
            assert isinstance(x, Out) or x.share is not None

    def periodic(self):
        return {n: x for n, x in self.ins.items() if isinstance(x, LG.Periodic)}

    def bytes_needed(self, L=None):
        size = lambda kind: torch.empty((), dtype=G._KIND[kind][0]).element_size()
        total = 0
        for x in self.ins.values():
            if isinstance(x, LG.Periodic):
                total += x.n * x.block.dtype.itemsize
            elif x is not None:
                total += x.nbytes
        total += sum(o.n * size(o.kind) for o in self.outs.values())
        total += sum((w(L) if callable(w) else w) for w in self.ws.values() if L is not None or not callable(w))
        return total + 2 * GB                      # the comparison's temporaries and the guards

    def table_row(self, cid, entry):
        per = ["%s: %d rows, %.4f" % (n, x.period, x.share) for n, x in self.periodic().items() if x.share is not None]
        crossing = ", ".join(self.crossing + (("%s (> %d bytes)" % self.crossing_ws,) if self.crossing_ws else ()))
        return "| %s | `%s` | %s | %s | %s |" % (cid, entry, self.shape, crossing, "; ".join(per))

    def run(self):
        from isx._lib import lib
        L = lib()
        need = self.bytes_needed(L)
        assert need <= PEAK_BYTES, ("the case needs %.1f GB" % (need / GB))
        total = torch.cuda.get_device_properties(0).total_memory
        if total < need:
            pytest.skip("the device has %.0f GB in all, the case needs %.1f GB" % (total / GB, need / GB))
        want = self.ref(types.SimpleNamespace(**{n: (x.block if isinstance(x, LG.Periodic) else x) for n, x in self.ins.items()}))
        assert set(want) == set(self.outs) | set(self.io), ("every output is compared", sorted(want))
        r = {}
        try:
            for n, x in self.ins.items():
                if x is None:
                    r[n] = None
                elif isinstance(x, LG.Periodic):
                    r[n] = x.region(io=n in self.io)
                else:
                    kind = LG._KIND[np.dtype(np.int64) if x.dtype == np.uint64 else x.dtype]
                    r[n] = G.Region(kind, x.shape, self.guard.get(n, 4096), data=LG.as_ints(x), guard_value=LG._IN_GUARD.get(kind))
            for n, o in self.outs.items():
                r[n] = G.Region(o.kind, o.shape, o.guard)
            for n, w in self.ws.items():
                r[n] = G.workspace(w(L) if callable(w) else w)
                assert self.crossing_ws is None or self.crossing_ws[0] != n or r[n].n > self.crossing_ws[1], (n, r[n].n, self.crossing_ws)
            torch.cuda.synchronize()
            if self.hooks is not None:
                L.isx_debug_set_gemm_cfg(self.hooks[0]); L.isx_debug_set_conv_cfg(self.hooks[1])
            try:
                rc = self.call(L, types.SimpleNamespace(**{n: G.ptr(x) for n, x in r.items()}), torch.cuda.current_stream().cuda_stream)
            finally:
                if self.hooks is not None:
                    L.isx_debug_set_gemm_cfg(-1); L.isx_debug_set_conv_cfg(-1)
            assert rc == 0, (rc, L.isx_last_error())
            torch.cuda.synchronize()
            for n, x in r.items():
                assert x is None or x.guards_intact(), ("store outside", n)
            for n in want:
                o = self.outs.get(n)
                if n in self.check:                                         # an output of a few MB with a comparison of its own: on the host, every row
                    G.assert_clean([r[n]], (), n)
                    self.check[n](r[n].host(), want[n])
                elif o is not None and o.own_period:                        # no bit-exact reference: the first period inside the entry's bound, the rest its repeats
                    G.assert_clean([r[n]], (), n)
                    first = r[n].body[:o.period].contiguous()
                    o.own_period(first.cpu().numpy(), want[n])
                    LG.assert_periodic(r[n].raw(), first.view(r[n].buf.dtype).reshape(-1), r[n].poison, "%s of %s against its own first period" % (n, self.shape))
                elif n in self.io or o.period is not None:
                    per = self.ins[n].period if n in self.io else o.period
                    parts = self.ins[n].parts if n in self.io else o.parts
                    assert np.asarray(want[n]).shape[0 if parts == 1 else 1] == per, (n, np.asarray(want[n]).shape, per)
                    LG.assert_region_periodic(r[n], want[n], "%s of %s" % (n, self.shape), parts)
                else:
                    G.assert_clean([r[n]], (), n)
                    got = r[n].host()
                    G.assert_bits(got, np.ascontiguousarray(want[n]).reshape(got.shape), n)
        finally:
            torch.cuda.synchronize()
            r.clear()
            torch.cuda.empty_cache()                # a case's 8 GB blocks are of no use to the next one


# ==== descriptor head ===============================================================================================================================
def _l2norm(D, period, shifted):
    B = _rows_past_line(D, 8)
    rng = _rng(D, period)
    x = LG.Periodic(_normal(rng, period, D), B, "x")
    shift = _normal(rng, D) * F(0.01) if shifted else None
    if shifted:
        call = lambda L, p, st: L.isx_l2norm_shift_rows(p.x, p.shift, B, D, EPS, p.y, st)
    else:
        call = lambda L, p, st: L.isx_l2norm_rows(p.x, B, D, EPS, p.y, st)
    ins = dict(x=x, shift=shift) if shifted else dict(x=x)
    return Case("B=%d D=%d (%s kernel)" % (B, D, dm.l2norm_kernel(D, True)), ins, call, lambda a: dict(y=dm.l2norm_rows(a.x, shift=getattr(a, "shift", None))),
                outs=dict(y=Out("f32", B, (D,), period)), crossing=("x", "y"))


case("isx_l2norm_rows", "wave")(lambda: _l2norm(2048, 131, False))
case("isx_l2norm_rows", "block")(lambda: _l2norm(100352, 3, False))
case("isx_l2norm_rows", "scalar")(lambda: _l2norm(100353, 3, False))
case("isx_l2norm_shift_rows", "wave")(lambda: _l2norm(2048, 131, True))
case("isx_l2norm_shift_rows", "block")(lambda: _l2norm(100352, 3, True))
case("isx_l2norm_shift_rows", "scalar")(lambda: _l2norm(100353, 3, True))


@case("isx_l2norm_rows_bwd")
def _():
    D, period = 2048, 131
    B = _rows_past_line(D, 8)
    rng = _rng(D, period, 1)
    x, dy = LG.Periodic(_normal(rng, period, D), B, "x"), LG.Periodic(_normal(rng, period, D), B, "dy")
    return Case("B=%d D=%d" % (B, D), dict(x=x, dy=dy), lambda L, p, st: L.isx_l2norm_rows_bwd(p.x, p.dy, B, D, EPS, p.dx, st),
                lambda a: dict(dx=dm.l2norm_rows_bwd(a.x, a.dy)), outs=dict(dx=Out("f32", B, (D,), period)), crossing=("x", "dy", "dx"))


GAP = (21400, 2048, 7, 7)                          # 21 400 x 100 352 = 2 147 532 800 elements


@case("isx_gap_l2")
def _():
    B, C, Hh, W = GAP
    f = LG.Periodic(_normal(_rng(B, C), 3, C, Hh, W), B, "fmap")
    return Case("B=%d of %dx%dx%d NCHW" % GAP, dict(f=f), lambda L, p, st: L.isx_gap_l2(p.f, B, C, Hh, W, EPS, p.y, st),
                lambda a: dict(y=dm.gap_l2(a.f, B_launch=B)), outs=dict(y=Out("f32", B, (C,), 3)), crossing=("f",))


@case("isx_gap_l2_nhwc")
def _():
    B, C, Hh, W = GAP
    f = LG.Periodic(_normal(_rng(B, C, 1), 3, Hh * W, C), B, "fmap")
    return Case("B=%d of %dx%dx%d NHWC" % (B, Hh, W, C), dict(f=f), lambda L, p, st: L.isx_gap_l2_nhwc(p.f, B, C, Hh, W, EPS, p.y, st),
                lambda a: dict(y=dm.gap_l2_nhwc(a.f)), outs=dict(y=Out("f32", B, (C,), 3)), crossing=("f",))


def _bias_act(C, inner, period, tag):
    """y: rows of C * inner elements (inner = 1: one channels-last pixel; inner = H W: one NCHW image)."""
    row = C * inner
    rows = _rows_past_line(row, 8)
    rows += 1 - rows % 2 if tag == "scalar" else 0                             # an odd row count of an odd row: n % 4 != 0
    n = rows * row
    assert (n % 4 != 0) == (tag == "scalar")
    rng = _rng(C, inner)
    y, res, b = LG.Periodic(_normal(rng, period, row), rows, "y"), LG.Periodic(_normal(rng, period, row), rows, "residual"), _normal(rng, C)
    ch = (np.arange(row) // inner) % C
    return Case("n=%d C=%d inner=%d (%s)" % (n, C, inner, tag), dict(y=y, b=b, r=res), lambda L, p, st: L.isx_bias_act_inplace(p.y, p.b, p.r, n, C, inner, 1, st),
                lambda a: dict(y=np.maximum((a.y + a.b[ch][None, :]) + a.r, F(0))), io=("y",), crossing=("y", "r"))


case("isx_bias_act_inplace", "inner_1")(lambda: _bias_act(64, 1, 131, "float4, channels last"))
case("isx_bias_act_inplace", "inner_hw")(lambda: _bias_act(8, 16, 131, "float4, NCHW"))
case("isx_bias_act_inplace", "scalar")(lambda: _bias_act(3, 49, 131, "scalar"))

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
IMAGES = (14270, 224, 224)                         # 14 270 x 150 528 = 2 148 034 560 bytes in, as many floats out


def _u8_to_f32(cl):
    B, Hh, W = IMAGES
    img = LG.Periodic(_rng(B, cl).integers(0, 256, (3, Hh, W, 3), dtype=np.uint8), B, "img")

    def ref(a):
        out = O.images_u8_to_f32(a.img, MEAN, STD)
        return dict(out=_nhwc(out) if cl else out)
    return Case("B=%d of %dx%d, %s" % (B, Hh, W, "channels last" if cl else "NCHW"), dict(img=img),
                lambda L, p, st: L.isx_images_u8_to_f32(p.img, B, Hh, W, *MEAN, *STD, cl, p.out, st), ref,
                outs=dict(out=Out("f32", B, (Hh, W, 3) if cl else (3, Hh, W), 3)), crossing=("img", "out"))


case("isx_images_u8_to_f32", "nchw")(lambda: _u8_to_f32(0))
case("isx_images_u8_to_f32", "channels_last")(lambda: _u8_to_f32(1))


# ==== inference trunk ===============================================================================================================================
def _conv1x1(Cin, Cout, res, cfg):
    M, period = 8388800, 131
    rng = _rng(Cin, Cout)
    x = LG.Periodic(_normal(rng, period, Cin), M, "x", guard=128 * Cin)
    w, b = _normal(rng, Cout, Cin) * F(Cin ** -0.5), _normal(rng, Cout)
    r = LG.Periodic(_normal(rng, period, Cout), M, "residual", guard=128 * Cout) if res else None
    assert G.stream_applicable(M, Cin, Cout, 0) == (Cin == 64)
    return Case("M=%d Cin=%d Cout=%d%s, %s" % (M, Cin, Cout, " + residual" if res else "", "conv cfg 9" if cfg == 9 else "automatic dispatch"),
                dict(x=x, w=w, b=b, r=r), lambda L, p, st: L.isx_conv1x1_nhwc(p.x, M, Cin, p.w, Cout, p.b, p.r, 1, p.y, st),
                lambda a: dict(y=O.conv1x1_nhwc(a.x, a.w, a.b, a.r, True)), outs=dict(y=Out("f32", M, (Cout,), period, guard=128 * Cout)),
                hooks=(-1, cfg), crossing=("y", "r") if res else ("x",), guard=dict(w=128 * Cin))


for _cfg in (-1, 9):
    case("isx_conv1x1_nhwc", "y_crosses" + ("_cfg9" if _cfg == 9 else ""))(lambda _cfg=_cfg: _conv1x1(64, 256, True, _cfg))
    case("isx_conv1x1_nhwc", "x_crosses" + ("_cfg9" if _cfg == 9 else ""))(lambda _cfg=_cfg: _conv1x1(256, 64, False, _cfg))


def _conv3x3(B, Hh, Cin, Cout, stride, period, posmaj):
    Ho = (Hh - 1) // stride + 1
    rng = _rng(B, Hh, Cin, stride)
    x = LG.Periodic(_normal(rng, period, Hh, Hh, Cin), B, "x", guard=128 * Cin * min(Hh * Hh, 64))
    w, b = _normal(rng, Cout, 3, 3, Cin) * F((9 * Cin) ** -0.5), _normal(rng, Cout)
    assert (G.pos_major_rows(B, Hh, Hh, Cin, Ho, Ho, Cout, Cout // 64) > 0) == posmaj
    og = max(128 * Cout, 127 * Ho * Ho * Cout if posmaj else 0)
    return Case("B=%d of %dx%d Cin=%d Cout=%d stride %d (%s)" % (B, Hh, Hh, Cin, Cout, stride, "position-major" if posmaj else "pixel-major"),
                dict(x=x, w=w, b=b), lambda L, p, st: L.isx_conv3x3_nhwc(p.x, B, Hh, Hh, Cin, p.w, Cout, stride, p.b, None, 1, p.y, st),
                lambda a: dict(y=O.conv3x3_nhwc(a.x, a.w, a.b, stride, None, True)), outs=dict(y=Out("f32", B, (Ho, Ho, Cout), period, guard=og)),
                crossing=("y",), guard=dict(w=128 * 9 * Cin))


case("isx_conv3x3_nhwc", "pixel_major")(lambda: _conv3x3(2675, 56, 32, 256, 1, 3, False))
case("isx_conv3x3_nhwc", "position_major")(lambda: _conv3x3(171199, 7, 64, 256, 1, 7, True))
case("isx_conv3x3_nhwc", "stride_2")(lambda: _conv3x3(10700, 56, 32, 256, 2, 3, False))


# ==== retrieval =====================================================================================================================================
def _unit(rng, n, d):
    return O.l2norm_rows(_normal(rng, n, d))


@case("isx_cosine_sim")
def _():
    M = N = 46400
    D, period = 8, 131
    rng = _rng(M, D)
    q, g = LG.Periodic(_unit(rng, period, D), M, "Q", guard=128 * D), _unit(rng, N, D)
    return Case("M=N=%d D=%d" % (M, D), dict(q=q, g=g), lambda L, p, st: L.isx_cosine_sim(p.q, M, p.g, N, D, p.sim, st),
                lambda a: dict(sim=O.cosine_sim(a.q, a.g)), outs=dict(sim=Out("f32", M, (N,), period, guard=128 * N)), crossing=("sim",), guard=dict(g=128 * D))


SIM = (524309, 4099, 131)                          # (M, N, period): 2 149 142 591 scores, rows of an odd length


def _sim_block(seed):
    M, N, period = SIM
    sim = _normal(_rng(N, seed), period, N)
    sim[:, N // 3] = sim[:, 1]                                                # a tie per row: broken by index
    return LG.Periodic(sim, M, "sim")


@case("isx_topk_rows")
def _():
    M, N, period = SIM
    k = 10

    def ref(a):
        s, i = O.topk_rows(a.sim, k, idx_base=3)
        return dict(ts=s, ti=np.ascontiguousarray(i, np.int64))
    return Case("M=%d N=%d k=%d" % (M, N, k), dict(sim=_sim_block(0)), lambda L, p, st: L.isx_topk_rows(p.sim, M, N, k, 3, p.ts, p.ti, st), ref,
                outs=dict(ts=Out("f32", M, (k,), period), ti=Out("i64", M, (k,), period)), crossing=("sim",))


def _rank_full(M, N, period, what, ws_past):
    rng = _rng(M, N)
    sim = (np.round(_normal(rng, period, N) * 8) / 8).astype(F)                # many ties: broken by index
    sim = LG.Periodic(sim, M, "sim")
    return Case("M=%d N=%d (%s)" % (M, N, what), dict(sim=sim), lambda L, p, st: L.isx_rank_full(p.sim, M, N, p.ranked, p.ws, L.isx_rank_full_workspace(M, N), st),
                lambda a: dict(ranked=np.ascontiguousarray(O.rank_full(a.sim), np.int64)), outs=dict(ranked=Out("i64", M, (N,), period)),
                ws=dict(ws=lambda L: L.isx_rank_full_workspace(M, N)), crossing_ws=("ws", ws_past))


case("isx_rank_full", "second_slab")(lambda: _rank_full(32771, 4097, 7, "rows in slabs of 32 768: the second slab", 1 << 31))
case("isx_rank_full", "workspace_4gib")(lambda: _rank_full(65543, 4097, 7, "the key workspace past 4 GiB", 1 << 32))


def _tiled_rows(a, rows):
    """Host: row r of the result is row r % len(a) of a."""
    return np.asarray(a)[np.arange(rows) % len(a)]


def _search(fast):
    """The repeated gallery rows make every score an R-fold tie (R = 8005 or 8004) that the index breaks."""
    M, N, D, k, period, base = 4, 1048640, 2048, 10, 131, 11
    rng = _rng(N, D, fast)
    q, g = _unit(rng, M, D), LG.Periodic(_unit(rng, period, D), N, "G", guard=256 * D)

    def ref(a):
        s, i = O.topk_rows(np.ascontiguousarray(_tiled_rows(O.cosine_sim(a.q, a.g).T, N).T), k, idx_base=base)
        return dict(ts=s, ti=np.ascontiguousarray(i, np.int64))
    if fast:
        ws = lambda L: L.isx_cosine_topk_fast_workspace(M, N, D, k, 0)
        call = lambda L, p, st: L.isx_cosine_topk_fast(p.q, M, p.g, N, D, k, base, None, None, p.ts, p.ti, p.ws, ws(L), st)
    else:
        ws = lambda L: L.isx_cosine_topk_workspace(M, N, D, k)
        call = lambda L, p, st: L.isx_cosine_topk(p.q, M, p.g, N, D, k, base, p.ts, p.ti, p.ws, ws(L), st)
    return Case("M=%d N=%d D=%d k=%d" % (M, N, D, k), dict(q=q, g=g), call, ref, outs=dict(ts=Out("f32", M, (k,)), ti=Out("i64", M, (k,))), ws=dict(ws=ws),
                crossing=("g",), guard=dict(q=256 * D))


case("isx_cosine_topk")(lambda: _search(False))
case("isx_cosine_topk_fast")(lambda: _search(True))

ROWS_F16 = (1048585, 2048, 131)                    # (B, D, period)


@case("isx_rows_to_f16")
def _():
    B, D, period = ROWS_F16
    x = _normal(_rng(B, D, 16), period, D)
    x[1, :8] = [65504.0, -65504.0, 6.1e-5, 5.96e-8, 2.9e-8, 0.0, -0.0, 1.0009765625]

    def norm2(got, block):                                                   # tests/test_gpu_fast_guards.py norm2_within, on every row
        exact = _tiled_rows((block.astype(np.float64) ** 2).sum(1), B)
        got = got.astype(np.float64)
        assert (got >= exact * (1 - 1e-6)).all() and (got <= exact * (1 + 2e-6 + (D + 2) * 2.0 ** -23)).all()
    return Case("B=%d D=%d" % (B, D), dict(x=LG.Periodic(x, B, "x")), lambda L, p, st: L.isx_rows_to_f16(p.x, B, D, p.h, p.n2, p.am, st),
                lambda a: dict(h=a.x.astype(np.float16), am=np.abs(a.x).max(1), n2=a.x), outs=dict(h=Out("f16", B, (D,), period), n2=Out("f32", B, ()), am=Out("f32", B, (), period)),
                check=dict(n2=norm2), crossing=("x", "h"))


@case("isx_gallery_to_f16")
def _():
    import test_gpu_fast_guards as TF
    N, D, period = ROWS_F16
    g = _unit(_rng(N, D, 17), period, D) * F(0.3)

    def ref(a):
        want, n2max, amax, lost = TF.gallery_f16_model(a.g)                   # one power-of-two scale for the gallery: the period's, since the maximum is
        return dict(gh=want, gs=np.array([n2max, amax, lost, 0.0]))
    return Case("N=%d D=%d" % (N, D), dict(g=LG.Periodic(g, N, "G")), lambda L, p, st: L.isx_gallery_to_f16(p.g, N, D, p.gh, p.gs, st), ref,
                outs=dict(gh=Out("f16", N, (D,), period), gs=Out("f32", 4, ())), check=dict(gs=lambda s_, want: TF.gstats_within(s_, want[0], want[1], want[2], D)),
                crossing=("g", "gh"))


@case("isx_cosine_sim_f16")
def _():
    import test_gpu_fast_guards as TF
    M = N = 46400
    D, period = 64, 131
    rng = _rng(M, D, 18)
    q, g = rng.standard_normal((period, D)).astype(np.float16), rng.standard_normal((N, D)).astype(np.float16)

    def within(first, want):                                                 # the bound of test_cosine_sim_f16
        exact, bound = want
        assert not np.isnan(first).any() and (np.abs(first - exact) <= bound).all()
    return Case("M=N=%d D=%d" % (M, D), dict(q=LG.Periodic(q, M, "Q", guard=256 * D), g=g), lambda L, p, st: L.isx_cosine_sim_f16(p.q, M, p.g, N, D, p.sim, st),
                lambda a: dict(sim=TF.sim_f16_bound(a.q, a.g)), outs=dict(sim=Out("f32", M, (N,), period, guard=256 * N, own_period=within)), crossing=("sim",),
                guard=dict(g=256 * D))


def _labels(M, N, period):
    Lb = max(1, N // 10)
    gl, ql = (np.arange(N) % Lb).astype(np.int32), (np.arange(period) % (Lb + 1)).astype(np.int32)
    ql[period - 1] = Lb                                                      # absent from the gallery: NaN
    return LG.Periodic(ql, M, "query labels"), gl


def _same_ap(M):
    def check(got, want):
        want = _tiled_rows(want, M)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        G.assert_bits(got[ok], want[ok])
    return check


@case("isx_average_precision_sim")
def _():
    M, N, period = SIM
    ql, gl = _labels(M, N, period)
    return Case("M=%d N=%d" % (M, N), dict(sim=_sim_block(1), ql=ql, gl=gl), lambda L, p, st: L.isx_average_precision_sim(p.sim, M, N, p.ql, p.gl, 1, p.ap, st),
                lambda a: dict(ap=O.average_precision(O.rank_full(a.sim), a.ql, a.gl, 1)), outs=dict(ap=Out("f64", M, ())), check=dict(ap=_same_ap(M)), crossing=("sim",))


@case("isx_average_precision")
def _():
    """ranked: 65 543 x 4097 int64 indices, 2.1 GB -- past 4 GiB?  No: 268 M elements of 8 bytes = 2.15e9 bytes; M = 131 101 gives 4.297e9 bytes."""
    M, N, period = 131101, 4097, 7
    sim = (np.round(_normal(_rng(M, N, 19), period, N) * 8) / 8).astype(F)
    ranked = np.ascontiguousarray(O.rank_full(sim), np.int64)
    ql, gl = _labels(M, N, period)
    assert M * N * 8 > 1 << 32
    c = Case("M=%d N=%d: %d bytes of ranked" % (M, N, M * N * 8), dict(ranked=LG.Periodic(ranked, M, "ranked"), ql=ql, gl=gl),
             lambda L, p, st: L.isx_average_precision(p.ranked, M, N, p.ql, p.gl, 2, p.ap, st), lambda a: dict(ap=O.average_precision(a.ranked, a.ql, a.gl, 2)),
             outs=dict(ap=Out("f64", M, ())), check=dict(ap=_same_ap(M)), crossing_ws=("ranked", 1 << 32))
    return c


@case("isx_masked_sums")
def _():
    import math
    M, N, period = SIM
    nlab = 5
    gl, ql = (np.arange(N) % nlab).astype(np.int32), (np.arange(period) % nlab).astype(np.int32)
    ql[period - 1] = nlab

    def ref(a):
        rows = [[float(v) for v in r] for r in a.sim]
        return dict(out=(np.array([[math.fsum(v for v, l in zip(row, a.gl) if l == a.ql[i]), math.fsum(row)] for i, row in enumerate(rows)]), a.sim))

    def within(got, want):                                                   # tests/test_gpu_retrieval_guards.py: N float64 adds in any order
        exact, sim = want
        bound = _tiled_rows(N * 2.0 ** -52 * np.abs(sim.astype(np.float64)).sum(1), M)
        assert (np.abs(got - _tiled_rows(exact, M)) <= bound[:, None]).all() and (got[period - 1::period, 0] == 0.0).all()
    return Case("M=%d N=%d" % (M, N), dict(sim=_sim_block(2), ql=LG.Periodic(ql, M, "query labels"), gl=gl),
                lambda L, p, st: L.isx_masked_sums(p.sim, M, N, p.ql, p.gl, p.out, st), ref, outs=dict(out=Out("f64", M, (2,))), check=dict(out=within), crossing=("sim",))


def _mine(rows_entry):
    """The N x N matrix with periodic rows; 300 couples whose anchors spread over all rows, a third of them in the rows past 2^31 elements."""
    N, period = 46400, 131
    r0 = 5 if rows_entry else 0
    rng = _rng(N, rows_entry, 20)
    sim = LG.Periodic(O.l2norm_rows(_normal(rng, period, N)), N - r0, "sim")
    labels = rng.integers(0, 50, N).astype(np.int32)
    i1 = np.r_[rng.integers(r0, N, 200), rng.integers(LG.LINE // N + 1, N, 100)].astype(np.int64)
    i2 = np.array([rng.choice(np.flatnonzero(labels == labels[a])) for a in i1], np.int64)
    n = len(i1)
    ref = lambda a: dict(neg=np.concatenate([tm.mine(a.sim[(a_ - r0) % period][None], N, a_, a.labels, [a_], [p_], 1) for a_, p_ in zip(a.i1.tolist(), a.i2.tolist())]))
    if rows_entry:
        call = lambda L, p, st: L.isx_mine_negatives_rows(p.sim, N, r0, N - r0, p.labels, p.i1, p.i2, n, 1, p.neg, st)
    else:
        call = lambda L, p, st: L.isx_mine_negatives(p.sim, N, p.labels, p.i1, p.i2, n, 1, p.neg, st)
    return Case("N=%d, %d couples%s" % (N, n, ", rows %d.." % r0 if rows_entry else ""), dict(sim=sim, labels=labels, i1=i1, i2=i2), call, ref,
                outs=dict(neg=Out("i64", n, ())), crossing=("sim",))


case("isx_mine_negatives")(lambda: _mine(False))
case("isx_mine_negatives_rows")(lambda: _mine(True))


# ==== training ======================================================================================================================================
XENT = (2147500, 1000, 131)                        # (B, C, period)


def _xent_fns():
    import test_gpu_xent_chains as XC                                         # EXP / LOG: the device's expf and logf, read through isx_debug_expf_logf
    return XC.EXP, XC.LOG


def _xent_block(seed):
    B, C, period = XENT
    rng = _rng(C, seed)
    return LG.Periodic(_normal(rng, period, C) * F(3), B, "logits"), LG.Periodic(rng.integers(0, C, (period,), dtype=np.int32), B, "labels")


@case("isx_softmax_xent_fwd")
def _():
    B, C, period = XENT
    z, y = _xent_block(0)

    def ref(a):
        EXP, LOG = _xent_fns()
        return dict(rows=np.asarray(xm.forward(a.z, a.y, EXP, LOG), F))
    return Case("B=%d C=%d" % (B, C), dict(z=z, y=y), lambda L, p, st: L.isx_softmax_xent_fwd(p.z, p.y, B, C, p.rows, st), ref,
                outs=dict(rows=Out("f32", B, (), period)), crossing=("z",))


@case("isx_softmax_xent_bwd")
def _():
    B, C, period = XENT
    z, y = _xent_block(1)

    def ref(a):
        EXP, LOG = _xent_fns()
        return dict(dz=np.asarray(xm.backward(a.z, a.y, xm.scale_of(0.2, float(a.sd[0])), EXP), F))
    return Case("B=%d C=%d" % (B, C), dict(z=z, y=y, sd=np.array([xm.SCALE_DEV], F)), lambda L, p, st: L.isx_softmax_xent_bwd(p.z, p.y, B, C, 0.2, p.sd, p.dz, st), ref,
                outs=dict(dz=Out("f32", B, (C,), period)), crossing=("z", "dz"))


TRIPLET = (1048649, 2048, 131)                     # (B, D, period)


def _triplet_blocks():
    B, D, period = TRIPLET
    a_, p_, n_ = tm.row_case(period, D)
    return LG.Periodic(np.array(a_), B, "anchor"), LG.Periodic(np.array(p_), B, "positive"), LG.Periodic(np.array(n_), B, "negative")


@case("isx_triplet_loss_fwd")
def _():
    B, D, period = TRIPLET
    a_, p_, n_ = _triplet_blocks()
    return Case("B=%d D=%d" % (B, D), dict(a=a_, p=p_, n=n_), lambda L, p, st: L.isx_triplet_loss_fwd(p.a, p.p, p.n, B, D, tm.MARGIN, 1, p.rows, st),
                lambda a: dict(rows=tm.loss_rows(a.a, a.p, a.n, tm.MARGIN, True)), outs=dict(rows=Out("f32", B, (), period)), crossing=("a", "p", "n"))


def _triplet_bwd(dev):
    """Six operands of 2^31 elements would be 51.5 GB: the positive rows ARE the anchor rows here (the one read-only buffer passed twice, which the
    entry allows), five buffers, 43 GB.  The three gradients stay distinct: g_a = n - a, g_p = -a, g_n = a on the active rows."""
    B, D, period = TRIPLET
    a_, _, n_ = _triplet_blocks()
    rows = tm.loss_rows(a_.block, a_.block, n_.block, tm.MARGIN, True)
    assert (rows > 0).any() and (rows == 0).any()

    def ref(a):
        scale = tm.scale_dev(1.0 / B, float(a.sd[0])) if dev else tm.scale_host(1.0 / B)
        return dict(zip(("ga", "gp", "gn"), tm.grads(a.a, a.a, a.n, a.rows, scale, True)))
    # the loss rows (B values, with the zeros of the clamped triplets) stay far below 2^29 elements: no shift of the rule reaches them
    ins = dict(a=a_, n=n_, rows=LG.Periodic(rows, B, "loss rows"))
    if dev:
        ins["sd"] = np.array([tm.SCALE_DEV], F)
        call = lambda L, p, st: L.isx_triplet_loss_bwd_dev(p.a, p.a, p.n, p.rows, B, D, 1.0 / B, p.sd, 1, p.ga, p.gp, p.gn, st)
    else:
        call = lambda L, p, st: L.isx_triplet_loss_bwd(p.a, p.a, p.n, p.rows, B, D, 1.0 / B, 1, p.ga, p.gp, p.gn, st)
    return Case("B=%d D=%d, pos = anchor" % (B, D), ins, call, ref, outs=dict(ga=Out("f32", B, (D,), period), gp=Out("f32", B, (D,), period), gn=Out("f32", B, (D,), period)),
                crossing=("a", "n", "ga", "gp", "gn"))


case("isx_triplet_loss_bwd")(lambda: _triplet_bwd(False))
case("isx_triplet_loss_bwd_dev")(lambda: _triplet_bwd(True))


@case("isx_relu_grad")
def _():
    row, period = 64, 131
    rows = _rows_past_line(row, 8)
    n = rows * row
    rng = _rng(row, period, 2)
    dy, y = LG.Periodic(_normal(rng, period, row), rows, "dy"), LG.Periodic(_normal(rng, period, row), rows, "y")
    return Case("n=%d" % n, dict(dy=dy, y=y), lambda L, p, st: L.isx_relu_grad(p.dy, p.y, n, p.dz, st), lambda a: dict(dz=sm.relu_grad(a.dy, a.y)),
                outs=dict(dz=Out("f32", rows, (row,), period)), crossing=("dy", "y", "dz"))


@case("isx_softmax_xent_leaves")
def _():
    k, C, period = 5, 1000, 7
    Lv = XENT[0] // k
    z, y = xm.leaf_case(period, k, C)

    def ref(a):
        EXP, LOG = _xent_fns()
        loss, dz, _ = xm.leaves(a.z.reshape(period * k, C), a.y.reshape(-1), period, k, 0.2, xm.SCALE_DEV, EXP, LOG)
        return dict(loss=np.asarray(loss, F), dz=np.asarray(dz, F).reshape(period, k, C))
    return Case("leaves=%d k=%d C=%d" % (Lv, k, C), dict(z=LG.Periodic(np.array(z).reshape(period, k, C), Lv, "logits"), y=LG.Periodic(np.ascontiguousarray(y, np.int32).reshape(period, k), Lv, "labels")),
                lambda L, p, st: L.isx_softmax_xent_leaves(p.z, p.y, Lv, k, C, 0.2, xm.SCALE_DEV, p.loss, p.dz, st), ref,
                outs=dict(loss=Out("f32", Lv, (), period), dz=Out("f32", Lv, (k, C), period)), crossing=("z", "dz"))


@case("isx_triplet_leaves")
def _():
    k, D, period = 5, 2048, 7
    Lv = _rows_past_line(3 * k * D, 8)
    d = np.array(tm.leaf_case(period, k, D)).reshape(period, 3 * k, D)
    sa, sb = tm.leaf_scales(period, k, True)

    def ref(a):
        loss, dd, _ = tm.leaves(a.d.reshape(period * 3 * k, D), period, k, tm.MARGIN, True, sa, sb)
        return dict(loss=np.asarray(loss, F), dd=np.asarray(dd, F).reshape(period, 3 * k, D))
    return Case("leaves=%d k=%d D=%d" % (Lv, k, D), dict(d=LG.Periodic(d, Lv, "d")), lambda L, p, st: L.isx_triplet_leaves(p.d, Lv, k, D, tm.MARGIN, 1, sa, sb, p.loss, p.dd, st), ref,
                outs=dict(loss=Out("f32", Lv, (), period), dd=Out("f32", Lv, (3 * k, D), period)), crossing=("d", "dd"))


@case("isx_gap_bwd_nhwc")
def _():
    B, C, Hh, W = GAP
    period = 7
    g = _normal(_rng(B, C, 30), period, C)
    return Case("B=%d of %dx%dx%d" % (B, Hh, W, C), dict(g=LG.Periodic(g, B, "g")), lambda L, p, st: L.isx_gap_bwd_nhwc(p.g, B, Hh, W, C, p.dx, st),
                lambda a: dict(dx=np.ascontiguousarray(np.broadcast_to((a.g / F(Hh * W))[:, None, None, :], (period, Hh, W, C)))),
                outs=dict(dx=Out("f32", B, (Hh, W, C), period)), crossing=("dx",))


@case("isx_boxpool_s1_bwd_nhwc")
def _():
    import _eval_model as em
    B, C, Hh, W = GAP
    kh, kw, period = 3, 2, 3
    g = _normal(_rng(B, C, 31), period, Hh - kh + 1, W - kw + 1, C)
    return Case("B=%d of %dx%dx%d, %dx%d windows" % (B, Hh, W, C, kh, kw), dict(g=LG.Periodic(g, B, "g")),
                lambda L, p, st: L.isx_boxpool_s1_bwd_nhwc(p.g, B, C, Hh, W, kh, kw, p.dx, st), lambda a: dict(dx=em.boxpool_bwd_canonical(a.g, Hh, W, kh, kw)),
                outs=dict(dx=Out("f32", B, (Hh, W, C), period)), crossing=("dx",))


def _dgrad1(Cout, Cin):
    M, period = 8388800, 131
    rng = _rng(Cout, Cin, 32)
    dz, wt = LG.Periodic(_normal(rng, period, Cout), M, "dz", guard=128 * Cout), _normal(rng, Cin, Cout) * F(2.0 ** -4)
    big = Cin == 256
    mask = LG.Periodic(_normal(rng, period, Cin), M, "mask", guard=128 * Cin)      # plain normals: the sign decides, no planted zeros (the 99 % rule)
    return Case("M=%d Cout=%d -> Cin=%d, mask" % (M, Cout, Cin), dict(dz=dz, wt=wt, mask=mask),
                lambda L, p, st: L.isx_conv1x1_dgrad_nhwc(p.dz, M, Cout, p.wt, Cin, None, p.mask, p.dx, st), lambda a: dict(dx=sm.dgrad1x1(a.dz, a.wt, None, a.mask)),
                outs=dict(dx=Out("f32", M, (Cin,), period, guard=128 * Cin)), crossing=("dx", "mask") if big else ("dz",), guard=dict(wt=128 * Cout))


case("isx_conv1x1_dgrad_nhwc", "dx_crosses")(lambda: _dgrad1(64, 256))
case("isx_conv1x1_dgrad_nhwc", "dz_crosses")(lambda: _dgrad1(256, 64))


@case("isx_conv3x3_dgrad_nhwc")
def _():
    B, Hh = SMALL_MAPS
    Cout, Cin, period = 64, 256, 7
    rng = _rng(B, Cout, Cin, 33)
    dz = LG.Periodic(_normal(rng, period, Hh, Hh, Cout), B, "dz", guard=128 * Cout * 64)
    wt = _normal(rng, Cin, 3, 3, Cout) * F(2.0 ** -4)
    mask = LG.Periodic(_normal(rng, period, Hh, Hh, Cin), B, "mask", guard=128 * Cin * 49)
    return Case("B=%d of %dx%d Cout=%d -> Cin=%d, mask" % (B, Hh, Hh, Cout, Cin), dict(dz=dz, wt=wt, mask=mask),
                lambda L, p, st: L.isx_conv3x3_dgrad_nhwc(p.dz, B, Hh, Hh, Cout, p.wt, Cin, p.mask, p.dx, st), lambda a: dict(dx=sm.dgrad3x3(a.dz, a.wt, a.mask)),
                outs=dict(dx=Out("f32", B, (Hh, Hh, Cin), period, guard=128 * Cin * 49)), crossing=("dx", "mask"), guard=dict(wt=128 * 9 * Cout))


@case("isx_conv3x3_s2_col2im_nhwc")
def _():
    B, Hh, Cin, period = 76100, 14, 64, 7                                     # 76 100 x 49 output pixels x 576 = 2 147 846 400 floats of dcol
    Ho = (Hh - 1) // 2 + 1
    rng = _rng(B, Hh, Cin, 34)
    dcol = LG.Periodic(_normal(rng, period, Ho * Ho, 9, Cin), B, "dcol")
    mask = LG.Periodic(_normal(rng, period, Hh, Hh, Cin), B, "mask")
    return Case("B=%d of %dx%d Cin=%d" % (B, Hh, Hh, Cin), dict(dcol=dcol, mask=mask), lambda L, p, st: L.isx_conv3x3_s2_col2im_nhwc(p.dcol, B, Hh, Hh, Cin, p.mask, p.dx, st),
                lambda a: dict(dx=sm.col2im_s2(a.dcol.reshape(period * Ho * Ho, 9, Cin), period, Hh, Hh, Cin, a.mask)), outs=dict(dx=Out("f32", B, (Hh, Hh, Cin), period)),
                crossing=("dcol",))


@case("isx_linear_wgrad_leaves")
def _():
    Lv, R, N, K, period = 61700, 3, 17, 2048, 7                               # dw: 61 700 x 17 x 2048 = 2 148 147 200
    rng = _rng(Lv, N, K)
    dy, x = _normal(rng, period, R, N), _normal(rng, period, R, K)
    ref = lambda a: dict(dw=np.stack([O.cosine_sim(np.ascontiguousarray(a.dy[l].T), np.ascontiguousarray(a.x[l].T)) for l in range(period)]))
    return Case("leaves=%d R=%d N=%d K=%d" % (Lv, R, N, K), dict(dy=LG.Periodic(dy, Lv, "dy"), x=LG.Periodic(x, Lv, "x")),
                lambda L, p, st: L.isx_linear_wgrad_leaves(p.dy, p.x, Lv, R, N, K, p.dw, st), ref, outs=dict(dw=Out("f32", Lv, (N, K), period)), crossing=("dw",))


@case("isx_colsum_leaves")
def _():
    Lv, R, C, period = 7135, 3, 100352, 7                                     # x: 21 405 rows of 100 352
    x = _normal(_rng(Lv, R, C), period, R, C)
    return Case("leaves=%d R=%d C=%d" % (Lv, R, C), dict(x=LG.Periodic(x, Lv, "x")), lambda L, p, st: L.isx_colsum_leaves(p.x, Lv, R, C, p.out, st),
                lambda a: dict(out=hm.colsum_leaves(a.x.reshape(period * R, C), period, R)), outs=dict(out=Out("f32", Lv, (C,), period)), crossing=("x",))


HEAD = (21440, 100352)                             # 21 440 x 100 352 = 2 151 546 880: rows a multiple of 64


@case("isx_head_linear_fwd_rows")
def _():
    M, K, N, period = 21400, HEAD[1], 64, 3
    rng = _rng(M, K, N)
    x, w, bias = _normal(rng, period, K), _normal(rng, N, K) * F(K ** -0.5), _normal(rng, N)
    ws = lambda L: L.isx_head_linear_rows_workspace(M, K, N)
    return Case("M=%d K=%d N=%d" % (M, K, N), dict(x=LG.Periodic(x, M, "x"), w=w, bias=bias),
                lambda L, p, st: L.isx_head_linear_fwd_rows(p.x, M, K, p.w, N, p.bias, p.y, p.ws, ws(L), st), lambda a: dict(y=hm.linear_fwd(a.x, a.w, a.bias)),
                outs=dict(y=Out("f32", M, (N,), period)), ws=dict(ws=ws), crossing=("x",))


@case("isx_head_linear_dgrad")
def _():
    (Mp, K), N, period = HEAD, 256, 3
    rng = _rng(Mp, K, N, 1)
    dy, w = _normal(rng, period, N), _normal(rng, N, K) * F(N ** -0.5)
    dyT = np.ascontiguousarray(_tiled_rows(dy, Mp).T)                        # (N, Mp): column m is row m % 3 of dy
    return Case("Mp=%d N=%d K=%d" % (Mp, N, K), dict(dyT=dyT, w=w), lambda L, p, st: L.isx_head_linear_dgrad(p.dyT, Mp, N, p.w, K, p.dx, st),
                lambda a: dict(dx=hm.dgrad(np.ascontiguousarray(a.dyT[:, :period].T), a.w)), outs=dict(dx=Out("f32", Mp, (K,), period)), crossing=("dx",))


@case("isx_head_sgd_step")
def _():
    """A second step (first = 0): w and mom, 8.6 GB each, read and updated in place.  Their rows and the columns of dy are periodic over N."""
    (N, K), R, period = HEAD, 3, 3
    _, lr, mom, damp, wd, nest = hm.SGD_SETS[3]
    rng = _rng(N, K, R)
    dy, x = _normal(rng, R, period), _normal(rng, R, K)
    w0, m0 = _normal(rng, period, K) * F(K ** -0.5), _normal(rng, period, K) * F(0.01)
    ref = lambda a: dict(zip(("w", "mom"), hm.sgd_step(a.w, a.mom, hm.wgrad_rows(np.ascontiguousarray(a.dy[:, :period]), a.x), False, lr, mom, damp, wd, nest)))
    return Case("N=%d K=%d R=%d, momentum" % (N, K, R), dict(dy=np.ascontiguousarray(_tiled_rows(dy.T, N).T), x=x, w=LG.Periodic(w0, N, "w"), mom=LG.Periodic(m0, N, "mom")),
                lambda L, p, st: L.isx_head_sgd_step(p.dy, p.x, R, N, K, p.w, p.mom, 0, lr, mom, damp, wd, nest, st), ref, io=("w", "mom"), crossing=("w", "mom"))


# ==== inference trunk, the fused kernels ============================================================================================================
SMALL_MAPS = (171199, 7)                           # 171 199 images of 7 x 7: 8 388 751 pixels, x 256 channels = 2 147 520 256 elements; 1338 groups of 128


@case("isx_conv1x1_dual_nhwc", "stride_2")
def _():
    B, Ho = SMALL_MAPS
    Hh, K1, K2, Cout, period = 2 * Ho, 32, 32, 256, 7
    rng = _rng(B, K1, K2)
    t = LG.Periodic(_normal(rng, period, Ho, Ho, K1), B, "t", guard=128 * K1)
    x = LG.Periodic(_normal(rng, period, Hh, Hh, K2), B, "x", guard=128 * K2 * Hh * 2)
    w, b = _normal(rng, Cout, K1 + K2) * F((K1 + K2) ** -0.5), _normal(rng, Cout)
    return Case("B=%d of %dx%d -> %dx%d, K1=K2=32 Cout=%d stride 2" % (B, Hh, Hh, Ho, Ho, Cout), dict(t=t, x=x, w=w, b=b),
                lambda L, p, st: L.isx_conv1x1_dual_nhwc(p.t, K1, p.x, B, Hh, Hh, K2, 2, p.w, Cout, p.b, 1, p.y, st),
                lambda a: dict(y=O.conv1x1_dual_nhwc(a.t, a.x, a.w, a.b, 2, True)), outs=dict(y=Out("f32", B, (Ho, Ho, Cout), period, guard=128 * Cout)),
                crossing=("y",), guard=dict(w=128 * (K1 + K2)))


def _expand_weights(rng, Cin, mid, Cout, k3):
    return _normal(rng, mid, 3, 3, Cin) * F((9 * Cin) ** -0.5), _normal(rng, mid), _normal(rng, Cout, k3) * F(k3 ** -0.5), _normal(rng, Cout)


@case("isx_conv3x3_expand_nhwc")
def _():
    B, Hh = SMALL_MAPS
    Cin, period = 32, 7
    rng = _rng(B, Cin, 2)
    x = LG.Periodic(_normal(rng, period, Hh, Hh, Cin), B, "x", guard=128 * Cin * 64)
    r = LG.Periodic(_normal(rng, period, Hh, Hh, 256), B, "residual", guard=128 * 256 * 49)
    w2, b2, w3, b3 = _expand_weights(rng, Cin, 64, 256, 64)

    def ref(a):
        mid = O.conv3x3_nhwc(a.x, a.w2, a.b2, 1, None, True)
        return dict(y=O.conv1x1_nhwc(mid.reshape(-1, 64), np.ascontiguousarray(a.w3t.T), a.b3, a.r.reshape(-1, 256), True).reshape(period, Hh, Hh, 256))
    return Case("B=%d of %dx%d Cin=%d + residual" % (B, Hh, Hh, Cin), dict(x=x, w2=w2, b2=b2, w3t=np.ascontiguousarray(w3.T), b3=b3, r=r),
                lambda L, p, st: L.isx_conv3x3_expand_nhwc(p.x, B, Hh, Hh, Cin, p.w2, p.b2, 1, p.w3t, 256, p.b3, p.r, 1, p.y, st), ref,
                outs=dict(y=Out("f32", B, (Hh, Hh, 256), period, guard=128 * 256 * 49)), crossing=("y", "r"), guard=dict(w2=64 * 9 * Cin, w3t=64 * 256))


@case("isx_conv3x3_expand_dual_nhwc")
def _():
    B, Hh = SMALL_MAPS
    Cin, period = 32, 7
    rng = _rng(B, Cin, 3)
    t = LG.Periodic(_normal(rng, period, Hh, Hh, Cin), B, "t", guard=128 * Cin * 64)
    x2 = LG.Periodic(_normal(rng, period, Hh, Hh, 64), B, "x2", guard=128 * 64 * 49)
    w2, b2, wc, b = _expand_weights(rng, Cin, 64, 256, 128)
    ref = lambda a: dict(y=O.conv1x1_dual_nhwc(O.conv3x3_nhwc(a.t, a.w2, a.b2, 1, None, True), a.x2, np.ascontiguousarray(a.wct.T), a.b, 1, True))
    return Case("B=%d of %dx%d Cin=%d" % (B, Hh, Hh, Cin), dict(t=t, w2=w2, b2=b2, x2=x2, wct=np.ascontiguousarray(wc.T), b=b),
                lambda L, p, st: L.isx_conv3x3_expand_dual_nhwc(p.t, B, Hh, Hh, Cin, p.w2, p.b2, p.x2, p.wct, 256, p.b, 1, p.y, st), ref,
                outs=dict(y=Out("f32", B, (Hh, Hh, 256), period, guard=128 * 256 * 49)), crossing=("y",), guard=dict(w2=64 * 9 * Cin, wct=64 * 256))


def _expand128(B, Hh, period, posmaj):
    Cin, Cout = 64, 128
    rng = _rng(B, Hh, 128)
    P = Hh * Hh
    assert (G.pos_major_rows(B, Hh, Hh, Cin, Hh, Hh, Cout, 2) > 0) == posmaj
    og = max(128 * Cout, 127 * P * Cout if posmaj else 0)
    x = LG.Periodic(_normal(rng, period, Hh, Hh, Cin), B, "x", guard=128 * Cin * min(P, 64) * 2)
    r = LG.Periodic(_normal(rng, period, Hh, Hh, Cout), B, "residual", guard=og)
    w2, b2, w3, b3 = _expand_weights(rng, Cin, 128, Cout, 128)

    def ref(a):
        mid = O.conv3x3_nhwc(a.x, a.w2, a.b2, 1, None, True)
        return dict(y=O.conv1x1_nhwc(mid.reshape(-1, 128), np.ascontiguousarray(a.w3t.T), a.b3, a.r.reshape(-1, Cout), True).reshape(period, Hh, Hh, Cout))
    return Case("B=%d of %dx%d Cin=%d Cout=%d + residual (%s)" % (B, Hh, Hh, Cin, Cout, "position-major" if posmaj else "pixel-major"),
                dict(x=x, w2=w2, b2=b2, w3t=np.ascontiguousarray(w3.T), b3=b3, r=r),
                lambda L, p, st: L.isx_conv3x3_expand128_nhwc(p.x, B, Hh, Hh, Cin, p.w2, p.b2, p.w3t, Cout, p.b3, p.r, 1, p.y, st), ref,
                outs=dict(y=Out("f32", B, (Hh, Hh, Cout), period, guard=og)), crossing=("y", "r"), guard=dict(w2=128 * 9 * Cin, w3t=128 * Cout))


case("isx_conv3x3_expand128_nhwc", "position_major")(lambda: _expand128(342393, 7, 7, True))
case("isx_conv3x3_expand128_nhwc", "pixel_major")(lambda: _expand128(19951, 29, 3, False))


@case("isx_stem7x7_pool_nhwc")
def _():
    B, Hh, W = IMAGES
    rng = _rng(B, Hh, 7)
    x = LG.Periodic(_normal(rng, 3, Hh, W, 3), B, "x", guard=8 * W * 3 * 4)
    w, b = _normal(rng, 64, 7, 7, 3) * F(147 ** -0.5), _normal(rng, 64)
    Hp = ((Hh - 1) // 2 + 1 - 1) // 2 + 1
    return Case("B=%d of %dx%d" % IMAGES, dict(x=x, w=w, b=b), lambda L, p, st: L.isx_stem7x7_pool_nhwc(p.x, B, Hh, W, p.w, p.b, p.out, st),
                lambda a: dict(out=O.stem7x7_pool_nhwc(a.x, a.w, a.b)), outs=dict(out=Out("f32", B, (Hp, Hp, 64), 3, guard=128 * 64)), crossing=("x", "out"),
                guard=dict(w=64 * 147))


@case("isx_bias_relu_maxpool_nhwc")
def _():
    Hh, W, C, period = 8, 8, 64, 131
    B = _rows_past_line(Hh * W * C, 8)
    rng = _rng(B, C, 4)
    y, b = LG.Periodic(_normal(rng, period, Hh, W, C), B, "y"), _normal(rng, C)
    return Case("B=%d of %dx%dx%d" % (B, Hh, W, C), dict(y=y, b=b), lambda L, p, st: L.isx_bias_relu_maxpool_nhwc(p.y, p.b, B, Hh, W, C, p.out, st),
                lambda a: dict(out=O.bias_relu_maxpool_nhwc(a.y, a.b)), outs=dict(out=Out("f32", B, (4, 4, C), period)), crossing=("y",))


# ==== pooling and the region path ===================================================================================================================
def _boxpool(nhwc):
    B, C, Hh, W = GAP
    kh, kw = 3, 2
    fmap = _normal(_rng(B, C, 5), 3, C, Hh, W)
    fn = "isx_boxpool_s1_nhwc" if nhwc else "isx_boxpool_s1"
    oshape = (Hh - kh + 1, W - kw + 1, C) if nhwc else (C, Hh - kh + 1, W - kw + 1)
    return Case("B=%d of %dx%dx%d, %dx%d windows, %s" % (B, C, Hh, W, kh, kw, "NHWC" if nhwc else "NCHW"), dict(f=LG.Periodic(_nhwc(fmap) if nhwc else fmap, B, "fmap")),
                lambda L, p, st: getattr(L, fn)(p.f, B, C, Hh, W, kh, kw, p.out, st),
                lambda a: dict(out=_nhwc(O.boxpool_s1(_nchw(a.f), kh, kw)) if nhwc else O.boxpool_s1(a.f, kh, kw)), outs=dict(out=Out("f32", B, oshape, 3)),
                crossing=("f",))


case("isx_boxpool_s1")(lambda: _boxpool(False))
case("isx_boxpool_s1_nhwc")(lambda: _boxpool(True))

CLS = (72320, 464, 8, 8, 7)                        # (B, K, Hp, Wp, period): 72 320 x 29 696 = 2 147 614 720 class scores


def _cls_block(nhwc, seed):
    B, K, Hp, Wp, period = CLS
    cls = _normal(_rng(K, seed), period, K, Hp, Wp)
    return LG.Periodic(_nhwc(cls) if nhwc else cls, B, "cls")


def _best(nhwc):
    B, K, Hp, Wp, period = CLS
    fn = "isx_best_location_desc_nhwc" if nhwc else "isx_best_location_desc"

    def ref(a):
        desc, loc = dm.best_location_desc(_nchw(a.cls) if nhwc else a.cls)
        return dict(desc=desc, loc=np.ascontiguousarray(loc, np.int64))
    return Case("B=%d K=%d on %dx%d, %s" % (B, K, Hp, Wp, "NHWC" if nhwc else "NCHW"), dict(cls=_cls_block(nhwc, 0)),
                lambda L, p, st: getattr(L, fn)(p.cls, B, K, Hp, Wp, EPS, p.desc, p.loc, st), ref,
                outs=dict(desc=Out("f32", B, (K,), period), loc=Out("i64", B, (2,), period)), crossing=("cls",))


case("isx_best_location_desc")(lambda: _best(False))
case("isx_best_location_desc_nhwc")(lambda: _best(True))


def _region_topk(nhwc):
    import _eval_model as em
    B, K, Hp, Wp, period = CLS
    k = 6
    fn = "isx_region_topk_nhwc" if nhwc else "isx_region_topk"

    def ref(a):
        idx, sc = em.oracle_region_topk(_nchw(a.cls) if nhwc else a.cls, k)
        return dict(idx=np.ascontiguousarray(idx, np.int64), sc=sc)
    return Case("B=%d K=%d on %dx%d k=%d, %s" % (B, K, Hp, Wp, k, "NHWC" if nhwc else "NCHW"), dict(cls=_cls_block(nhwc, 1)),
                lambda L, p, st: getattr(L, fn)(p.cls, B, K, Hp, Wp, k, p.idx, p.sc, st), ref,
                outs=dict(idx=Out("i64", B, (k,), period), sc=Out("f32", B, (k,), period)), crossing=("cls",))


case("isx_region_topk")(lambda: _region_topk(False))
case("isx_region_topk_nhwc")(lambda: _region_topk(True))


def _gather(nhwc):
    """Two windows per image of an 8 x 8 map (Wp = 2): 21 400 rows of 100 352.  One window of the period is -1 (a zero row), one past the map."""
    B, C, Hf, kh, k, Wp, period = 10700, 2048, 8, 7, 2, 2, 3
    rng = _rng(B, C, 6)
    fmap = _normal(rng, period, C, Hf, Hf)
    idx = np.array([[3, 0], [-1, 2], [1, 4]], np.int64)
    shift = _normal(rng, C * kh * kh) * F(0.01)
    fn = "isx_region_gather_l2_nhwc" if nhwc else "isx_region_gather_l2"
    ref = lambda a: dict(rows=dm.region_gather_l2(_nchw(a.f) if nhwc else a.f, kh, kh, a.idx, Wp, shift=a.shift, order="hwc" if nhwc else "chw"))
    return Case("B=%d of %dx%dx%d, k=%d windows of %dx%d, %s" % (B, C, Hf, Hf, k, kh, kh, "NHWC" if nhwc else "NCHW"),
                dict(f=LG.Periodic(_nhwc(fmap) if nhwc else fmap, B, "fmap"), idx=LG.Periodic(idx, B, "flat_idx"),
                     shift=dm.shift_hwc(shift, C, kh, kh) if nhwc else shift),
                lambda L, p, st: getattr(L, fn)(p.f, B, C, Hf, Hf, kh, kh, p.idx, k, Wp, p.shift, EPS, p.rows, st), ref,
                outs=dict(rows=Out("f32", B, (k, C * kh * kh), period)), crossing=("rows",))


case("isx_region_gather_l2")(lambda: _gather(False))
case("isx_region_gather_l2_nhwc")(lambda: _gather(True))

REGION_SUM = (5350, 14, 14, 2048, 7, 7, 2, 3)      # (B, Hf, Wf, C, kh, kw, k, period): 5350 x 401 408 = 2 147 532 800 elements of fmap


def _region_sum_inputs(seed):
    import _region_train_model as rm
    B, Hf, Wf, C, kh, kw, k, period = REGION_SUM
    rng = _rng(B, C, seed)
    fmap = _normal(rng, period, C, Hf, Wf)
    idx = np.array([[9, 0], [63, -1], [27, 36]], np.int64)                      # Wp = 8: 64 windows; one entry skipped
    return rm, fmap, idx, _normal(rng, C * kh * kw) * F(0.01), _normal(rng, period, C * kh * kw)


@case("isx_region_sum_l2_nhwc")
def _():
    B, Hf, Wf, C, kh, kw, k, period = REGION_SUM
    rm, fmap, idx, shift, _ = _region_sum_inputs(0)
    Wp = Wf - kw + 1

    def ref(a):
        rows, n2 = rm.region_sum_l2(_nchw(a.f), kh, kw, a.idx, Wp, a.shift)
        return dict(rows=rows, n2=n2)
    return Case("B=%d of %dx%dx%d, k=%d windows of %dx%d" % (B, Hf, Wf, C, k, kh, kw), dict(f=LG.Periodic(_nhwc(fmap), B, "fmap"), idx=LG.Periodic(idx, B, "flat_idx"), shift=shift),
                lambda L, p, st: L.isx_region_sum_l2_nhwc(p.f, B, C, Hf, Wf, kh, kw, p.idx, k, Wp, p.shift, EPS, p.rows, p.n2, st), ref,
                outs=dict(rows=Out("f32", B, (C * kh * kw,), period), n2=Out("f32", B, (k,), period)), crossing=("f",))


@case("isx_region_sum_l2_bwd_nhwc")
def _():
    B, Hf, Wf, C, kh, kw, k, period = REGION_SUM
    rm, fmap, idx, shift, g = _region_sum_inputs(1)
    Wp = Wf - kw + 1
    n2 = rm.region_sum_l2(fmap, kh, kw, idx, Wp, shift)[1]

    def ref(a):
        df, cw = rm.region_sum_l2_bwd(_nchw(a.f), a.g, a.n2, kh, kw, a.idx, Wp, None)
        return dict(dfmap=_nhwc(df), cw=cw)
    return Case("B=%d of %dx%dx%d, k=%d windows of %dx%d" % (B, Hf, Wf, C, k, kh, kw),
                dict(f=LG.Periodic(_nhwc(fmap), B, "fmap"), g=LG.Periodic(g, B, "g"), n2=LG.Periodic(n2, B, "n2"), idx=LG.Periodic(idx, B, "flat_idx")),
                lambda L, p, st: L.isx_region_sum_l2_bwd_nhwc(p.f, p.g, p.n2, B, C, Hf, Wf, kh, kw, p.idx, k, Wp, None, 1, p.cw, p.dfmap, st), ref,
                outs=dict(cw=Out("f32", B, (k,), period), dfmap=Out("f32", B, (Hf, Wf, C), period)), crossing=("f", "dfmap"))


# ==== operands made of several periodic parts ========================================================================================================
@case("isx_topk_merge")
def _():
    """P x k = 4096, the documented maximum; the lists (P, M, k) pass 2^31 elements through M.  The top scores of parts 0 and 1 tie: the index decides."""
    P, k, period = 64, 64, 131
    M = _rows_past_line(P * k, 8)
    rng = _rng(P, k, 21)
    sc = -np.sort(-_normal(rng, P, period, k), axis=2)                       # every list in canonical order, scores distinct
    sc[1, :, 0] = sc[0, :, 0] = np.maximum(sc[0, :, 0], sc[1, :, 0]) + F(1)
    idx = np.stack([100000 * p_ + np.argsort(rng.random((period, k)), axis=1) for p_ in range(P)]).astype(np.int64)

    def ref(a):
        s_, i_ = O.topk_merge(a.s, a.i)
        return dict(ts=s_, ti=np.ascontiguousarray(i_, np.int64))
    return Case("P=%d M=%d k=%d" % (P, M, k), dict(s=LG.Periodic(sc, M, "scores", parts=P), i=LG.Periodic(idx, M, "idx", parts=P)),
                lambda L, p, st: L.isx_topk_merge(p.s, p.i, P, M, k, p.ts, p.ti, st), ref, outs=dict(ts=Out("f32", M, (k,), period), ti=Out("i64", M, (k,), period)),
                crossing=("s", "i"))


@case("isx_tree_sum_rows")
def _():
    Lr, c, period = 2, 64, 131
    rows = _rows_past_line(c, 8)
    n = rows * c
    rng = _rng(Lr, c, 40)
    block = (rng.standard_normal((Lr, period, c)) * 10.0 ** rng.integers(-3, 4, (Lr, period, c))).astype(F)

    def ref(a):
        import test_gpu_eval_guards as EG
        return dict(out=EG._tree_ref(a.rows.reshape(Lr, period * c)).reshape(period, c))
    return Case("L=%d n=%d" % (Lr, n), dict(rows=LG.Periodic(block, rows, "rows", parts=Lr)), lambda L, p, st: L.isx_tree_sum_rows(p.rows, Lr, n, n, p.out, st), ref,
                outs=dict(out=Out("f32", rows, (c,), period)), crossing=("rows", "out"))


@case("isx_head_linear_fwd")
def _():
    """xT: (K, Mp), column m the activation row m % 3 -- K parts of Mp elements with a period of 3."""
    (Mp, K), M, N, period = HEAD, 21400, 64, 3
    rng = _rng(Mp, K, N, 2)
    x, w, bias = _normal(rng, period, K), _normal(rng, N, K) * F(K ** -0.5), _normal(rng, N)
    ws = lambda L: L.isx_head_linear_splits(K) * Mp * N * 4
    return Case("M=%d Mp=%d K=%d N=%d" % (M, Mp, K, N), dict(xT=LG.Periodic(np.ascontiguousarray(x.T).reshape(K, period, 1), Mp, "xT", parts=K), w=w, bias=bias),
                lambda L, p, st: L.isx_head_linear_fwd(p.xT, M, Mp, K, p.w, N, p.bias, p.y, p.ws, ws(L), st),
                lambda a: dict(y=hm.linear_fwd(np.ascontiguousarray(a.xT.reshape(K, period).T), a.w, a.bias)), outs=dict(y=Out("f32", M, (N,), period)), ws=dict(ws=ws),
                crossing=("xT",))


@case("isx_head_linear_dgrad_parts")
def _():
    Ng, Gr, K, period = 32, 5, 64, 3
    Mp = 192 * 34953                                                         # a multiple of 64 and of the period: 6 710 976 rows per group
    N = Ng * Gr
    rng = _rng(Mp, Ng, Gr)
    dy, w = _normal(rng, period, N), _normal(rng, N, K) * F(Ng ** -0.5)
    return Case("Mp=%d Ng=%d groups=%d K=%d" % (Mp, Ng, Gr, K), dict(dyT=LG.Periodic(np.ascontiguousarray(dy.T).reshape(N, period, 1), Mp, "dyT", parts=N), w=w),
                lambda L, p, st: L.isx_head_linear_dgrad_parts(p.dyT, Mp, Ng, Gr, p.w, K, p.parts, st),
                lambda a: dict(parts=hm.dgrad_parts(np.ascontiguousarray(a.dyT.reshape(N, period).T), a.w, Ng)), outs=dict(parts=Out("f32", Mp, (K,), period, parts=Gr)),
                crossing=("parts",))


# ==== sharded average precision, DBA, the prep library ================================================================================================
WIDE = (917, 2341889, 7)                           # (M, N, period): 2 147 512 213 scores in rows of 2.3 M


def _wide(seed):
    M, N, period = WIDE
    rng = _rng(N, seed, 50)
    sim = _normal(rng, period, N)
    sim[:, N // 3] = sim[:, 1]                                                # a tie per row, broken by index; the last column ties with column 2
    sim[:, N - 1] = sim[:, 2]
    gl = np.full(N, 3, np.int32)
    gl[rng.choice(N, 9, replace=False)] = 0
    gl[np.r_[rng.choice(N, 4, replace=False), N - 1]] = 1
    return sim, np.array([0, 5, 0, 1, 5, 0, 1], np.int32), gl


@case("isx_ap_shard_positives")
def _():
    import _eval_model as em
    M, N, period = WIDE
    base = 1001
    sim, ql, gl = _wide(0)

    def ref(a):
        keys, count = np.zeros((period, em.AP_MAXP), np.uint64), np.zeros(period, np.int32)
        for r in range(period):
            j = np.flatnonzero(a.gl == a.ql[r])
            keys[r, :len(j)] = em.rank_keys(a.sim[r, j], base + j)
            count[r] = len(j)
        return dict(keys=np.sort(keys, axis=1), count=count)

    def as_sets(got, want):                                                  # "any order" (include/isx.h): the rows as sorted sets
        np.testing.assert_array_equal(np.sort(got.view(np.uint64), axis=1), _tiled_rows(want, M))
    return Case("M=%d N=%d" % (M, N), dict(sim=LG.Periodic(sim, M, "sim"), ql=LG.Periodic(ql, M, "query labels"), gl=gl),
                lambda L, p, st: L.isx_ap_shard_positives(p.sim, M, N, base, p.ql, p.gl, em.AP_MAXP, p.keys, p.count, st), ref,
                outs=dict(keys=Out("i64", M, (em.AP_MAXP,)), count=Out("i32", M, (), period)), check=dict(keys=as_sets), crossing=("sim",))


@case("isx_ap_shard_hist")
def _():
    import _eval_model as em
    M, N, period = WIDE
    W = 64
    sim, _, _ = _wide(1)
    rng = _rng(W, 51)
    keys = np.zeros((period, W), np.uint64)
    for r, npos in enumerate((37, 64, 1, 12, 64, 5, 20)):
        j = np.r_[rng.choice(N - 1, npos - 1, replace=False), N - 1]
        keys[r, rng.choice(W, npos, replace=False)] = em.rank_keys(sim[r, j], j)

    def ref(a):
        import test_gpu_eval_guards as EG
        return dict(hist=np.ascontiguousarray(EG._cpu_hist(a.sim, 0, a.keys), np.int32))
    return Case("M=%d N=%d W=%d" % (M, N, W), dict(sim=LG.Periodic(sim, M, "sim"), keys=LG.Periodic(keys, M, "keys_all")),
                lambda L, p, st: L.isx_ap_shard_hist(p.sim, M, N, 0, p.keys, W, p.hist, st), ref, outs=dict(hist=Out("i32", M, (em.AP_MAXP,), period)), crossing=("sim",))


@case("isx_ap_from_hist")
def _():
    ld, period = 40, 131
    M = _rows_past_line(ld, 8)
    rng = _rng(ld, 52)
    n_lab = rng.integers(38, 46, period).astype(np.int32)                      # nearly every row full: the zeros past n_lab stay under 1 % of the block
    n_lab[:6] = [3, 0, 41, 40, 1, 2]
    hist = np.zeros((period, ld), np.int32)
    for r in range(period):
        n = min(int(n_lab[r]), ld)
        hist[r, :n] = 1 + rng.integers(0, 1 << 20, n)                          # counts of a gallery of millions: no two positions alike
    def ref(a):
        from utils import metrics
        return dict(ap=metrics.ap_from_hist(torch.from_numpy(a.hist), torch.from_numpy(a.n_lab), 2).numpy())
    return Case("M=%d ld=%d" % (M, ld), dict(hist=LG.Periodic(hist, M, "hist"), n_lab=LG.Periodic(n_lab, M, "n_lab")),
                lambda L, p, st: L.isx_ap_from_hist(p.hist, ld, p.n_lab, M, 2, p.ap, st), ref, outs=dict(ap=Out("f64", M, ())), check=dict(ap=_same_ap(M)), crossing=("hist",))


@case("isx_dba_groups")
def _():
    """Instances of 1, 2, 3 and 5 items inside every period of 131 embeddings (the items of an instance interleaved); order / grp_begin / grp_size
    are the period's own plus the period's first item.  N = 8005 periods."""
    import _eval_model as em
    D, period, reps = 2048, 131, 8005
    N = period * reps
    rng = _rng(D, period, 53)
    sizes = [5] * 10 + [3] * 17 + [2] * 12 + [1] * 6
    assert sum(sizes) == period
    labels = np.concatenate([np.full(s_, g, np.int32) for g, s_ in enumerate(sizes)])[rng.permutation(period)]
    E = O.l2norm_rows(_normal(rng, period, D))
    order, begin, size, mg = em.dba_groups_of(labels)
    off = (np.arange(N) // period * period).astype(np.int32)
    tiled = lambda v: np.ascontiguousarray(v[np.arange(N) % period], np.int32)
    return Case("N=%d D=%d" % (N, D), dict(emb=LG.Periodic(E, N, "emb"), order=tiled(order) + off, begin=tiled(begin) + off, size=tiled(size)),
                lambda L, p, st: L.isx_dba_groups(p.emb, N, D, p.order, p.begin, p.size, mg, -1, p.out, st), lambda a: dict(out=em.dba_chain(a.emb, labels, -1)),
                outs=dict(out=Out("f32", N, (D,), period)), crossing=("emb", "out"))


@case("isxp_channel_moments_u8")
def _():
    import _mean_std_model as M_
    B, Hh, W = IMAGES
    img = LG.Periodic(_rng(B, 54).integers(0, 256, (3, Hh, W, 3), dtype=np.uint8), B, "img")

    def call(L, p, st):
        from isx import prep
        rc = prep.lib().isxp_channel_moments_u8(p.img, B, Hh, W, p.moments, st)
        assert rc == 0, prep.lib().isxp_last_error()
        return rc
    return Case("B=%d of %dx%d" % IMAGES, dict(img=img), call, lambda a: dict(moments=np.ascontiguousarray(M_.moments(a.img), np.int64)),
                outs=dict(moments=Out("i64", B, (3, 2), 3)), crossing=("img",))


@case("isx_affine_noisy_u8")
def _():
    """The resident set is the period's three images; image b of the call is row b % 3 with the matrix and the noise id of b % 3.  The fp64
    workspace of the spline coefficients is 17 GB."""
    import _augment_model as am
    B, Hh, W = IMAGES
    period, seed = 3, 20240607
    rng = _rng(B, 55)
    img = rng.integers(0, 256, (period, Hh, W, 3), dtype=np.uint8)
    ang = np.array([0.2, -0.1, 0.05])
    mat = np.stack([np.array([np.cos(t), -np.sin(t), 20.0 * t * 5, np.sin(t), np.cos(t), -8.0 * t * 5]) for t in ang]).astype(np.float64)
    ids = np.array([7, 1, 12], np.int64)
    rows = np.array([2, 0, 1], np.int64)
    mean, std = np.array(MEAN, F), np.array(STD, F)
    ws = lambda L: L.isx_affine_noisy_workspace(B, Hh, W)

    def ref(a):
        u8 = np.stack([am.affine_noisy(a.img[rows[i]], mat[i], seed, int(ids[i]))[0] for i in range(period)])
        return dict(u8=u8, f32=am.normalise(u8, mean, std, True))
    return Case("B=%d of %dx%d" % IMAGES, dict(img=img, rows=_tiled_rows(rows, B), mat=_tiled_rows(mat, B), ids=_tiled_rows(ids, B), mean=mean, std=std),
                lambda L, p, st: L.isx_affine_noisy_u8(p.img, p.rows, B, Hh, W, p.mat, seed, p.ids, p.mean, p.std, 1, p.u8, p.f32, p.ws, ws(L), st), ref,
                outs=dict(u8=Out("u8", B, (Hh, W, 3), period), f32=Out("f32", B, (Hh, W, 3), period)), ws=dict(ws=ws), crossing=("u8", "f32"),
                crossing_ws=("ws", 1 << 34))


# ==== trunk-suffix backward: weight gradients ========================================================================================================
def _wgrad(taps):
    """4093 leaves of one 82 x 100 image: 33 562 600 pixels x 64 channels.  S = 16 splits per leaf, so the grid's z extent is 65 488 of 65 535;
    the period is three distinct leaves."""
    from isx._lib import lib
    leaves, Hh, W, C, period = 4093, 82, 100, 64, 3
    K = Hh * W
    Sp = lib().isx_conv_wgrad_splits(K, C, C, taps)
    assert 1 < Sp and leaves * Sp <= 65535, (Sp, "leaves x splits must stay within the grid's z extent")
    rng = _rng(leaves, taps, 60)
    dz, x = _normal(rng, period, Hh, W, C), _normal(rng, period, Hh, W, C)
    g = sm.Geom(period, Hh, W, taps, 1)
    ref = lambda a: dict(zip(("dw", "db"), sm.wgrad_partials(a.dz.reshape(-1, C), a.x.reshape(-1, C), g, period, Sp)))
    return Case("leaves=%d of %dx%d Cin=Cout=%d taps=%d (S=%d)" % (leaves, Hh, W, C, taps, Sp),
                dict(dz=LG.Periodic(dz, leaves, "dz", guard=128 * C), x=LG.Periodic(x, leaves, "x", guard=128 * C + (W + 2) * C)),
                lambda L, p, st: L.isx_conv_wgrad_nhwc(p.dz, p.x, leaves, leaves, Hh, W, C, C, taps, 1, p.dw, p.db, st), ref,
                outs=dict(dw=Out("f32", leaves, (Sp, C, taps, C), period), db=Out("f32", leaves, (Sp, C), period)), crossing=("x", "dz"))


case("isx_conv_wgrad_nhwc", "taps_1")(lambda: _wgrad(1))
case("isx_conv_wgrad_nhwc", "taps_9")(lambda: _wgrad(9))


class FoldCase(object):
    """isx_bn_fold_backward with leaves x leaf_stride past the line: three leaves whose gradient buffers lie 2^30 + 16 396 floats apart inside ONE
    poisoned buffer of 2.15e9 floats.  Nothing is tiled (no period); the three leaves' gradients are compared with tests/_suffix_model.py bit
    for bit and every other element of the buffer must still be poison."""
    taps, Cin, Sp, leaves, Cout = 9, 64, 2, 3, sm.FOLD_COUT
    stride = (1 << 30) + 4 * 4099
    crossing, crossing_ws, shape = ("gw",), None, "leaves=3 splits=2 Cout=%d Cin=64 taps=9, leaf_stride=%d" % (sm.FOLD_COUT, (1 << 30) + 4 * 4099)

    def periodic(self):
        return {}

    def bytes_needed(self, L=None):
        return 4 * (2 * self.stride + 8192) + 2 * GB

    def table_row(self, cid, entry):
        return "| %s | `%s` | %s | gw / ggamma / gbeta: leaf 2 begins at float %d | no tiled operand |" % (cid, entry, self.shape, 2 * self.stride)

    def run(self):
        from isx._lib import lib
        L = lib()
        taps, Cin, Sp, leaves, Cout, stride = self.taps, self.Cin, self.Sp, self.leaves, self.Cout, self.stride
        assert leaves * stride > LG.LINE
        if torch.cuda.get_device_properties(0).total_memory < self.bytes_needed():
            pytest.skip("the device has less than %.1f GB in all" % (self.bytes_needed() / GB))
        dwp, db = sm.fold_case(taps, Cin, leaves, Sp)[:2]
        w, scale, mean, istd = sm.fold_params(taps, Cin)
        want = sm.fold_backward(dwp, db, w, scale, mean, istd, taps)
        nw = Cout * Cin * taps
        per_leaf = nw + 2 * Cout
        ins = [G.in_f32(np.array(a), 4096) for a in (dwp, db, w, scale, mean, istd)]
        buf = G.out_f32((2 * stride + per_leaf,), 4096)
        try:
            rc = L.isx_bn_fold_backward(ins[0].ptr, ins[1].ptr, leaves, Sp, ins[2].ptr, ins[3].ptr, ins[4].ptr, ins[5].ptr, Cout, Cin, taps, 0, stride,
                                        buf.ptr, buf.ptr + 4 * nw, buf.ptr + 4 * (nw + Cout), torch.cuda.current_stream().cuda_stream)
            assert rc == 0, (rc, L.isx_last_error())
            torch.cuda.synchronize()
            assert buf.guards_intact() and all(r.guards_intact() for r in ins)
            body = buf.body
            for l in range(leaves):
                at = l * stride
                for name, lo, n, wnt in (("gw", 0, nw, want[0][l]), ("ggamma", nw, Cout, want[1][l]), ("gbeta", nw + Cout, Cout, want[2][l])):
                    G.assert_bits(body[at + lo:at + lo + n].cpu().numpy(), np.ascontiguousarray(wnt).reshape(-1), (name, "leaf", l))
            assert buf.unwritten() == buf.n - leaves * per_leaf, "a store between the leaves' gradient buffers"
        finally:
            torch.cuda.synchronize()
            del buf
            torch.cuda.empty_cache()


case("isx_bn_fold_backward")(FoldCase)


@case("isx_debug_expf_logf")
def _():
    """The probe has no CPU reference (it IS the reference of the cross-entropy cases): the expected period is what a call on the period block alone
    returns -- the functions are element-wise, so the large call must repeat those bits."""
    row, period = 64, 131
    rows = _rows_past_line(row, 8)
    n = rows * row
    x = np.abs(_normal(_rng(row, period, 70), period, row)) * F(3) + F(1e-3)

    def ref(a):
        from isx._lib import lib
        t = torch.from_numpy(a.x).cuda()
        e, l = torch.empty_like(t), torch.empty_like(t)
        assert lib().isx_debug_expf_logf(t.data_ptr(), t.numel(), e.data_ptr(), l.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        e, l = e.cpu().numpy(), l.cpu().numpy()
        assert np.allclose(e, np.exp(a.x.astype(np.float64)), rtol=1e-5) and np.allclose(l, np.log(a.x.astype(np.float64)), rtol=1e-5, atol=1e-6)
        return dict(e=e, l=l)
    return Case("n=%d" % n, dict(x=LG.Periodic(x, rows, "x")), lambda L, p, st: L.isx_debug_expf_logf(p.x, n, p.e, p.l, st), ref,
                outs=dict(e=Out("f32", rows, (row,), period), l=Out("f32", rows, (row,), period)), crossing=("x", "e", "l"))


# ==== the tests =====================================================================================================================================
def stream_entries():
    """Every function of include/isx.h whose last parameter is `isx_stream_t stream`, plus the stream-taking entry of include/isx_prep.h."""
    names = []
    for header in ("isx.h", "isx_prep.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        names += re.findall(r"\b(isxp?_\w+)\s*\([^;{}]*?\w+\s+stream\s*\)\s*;", text)
    return sorted(set(names))


_BUILT = {}


def _built(cid):
    """A case is built once per process: its period blocks and the closures of its reference (host memory only)."""
    if cid not in _BUILT:
        _BUILT[cid] = next(b for i, _, b in TABLE if i == cid)()
    return _BUILT[cid]


def test_every_period_holds_the_rules(capsys):
    """Builds every case on the host: LG.Periodic asserts the prime rule and the 99 % rule for every operand that reaches 2^29 elements, Case that
    the operands it names do pass 2^31.  Prints the case table of docs/rounds/r17.md (pytest -s)."""
    ids = [i for i, _, _ in TABLE]
    assert len(ids) == len(set(ids))
    rows = []
    for cid, entry, _ in TABLE:
        c = _built(cid)
        for n, x in c.periodic().items():
            assert x.share is None or x.share >= LG.MIN_DIFFER, (cid, n, x.share)
            assert LG.is_odd_prime(x.period), (cid, n, x.period)
        assert c.bytes_needed() <= PEAK_BYTES, (cid, c.bytes_needed() / GB)
        rows.append(c.table_row(cid, entry))
    with capsys.disabled():
        if os.environ.get("ISX_LARGE_TABLE"):
            print("\n" + "\n".join(rows))


def test_every_stream_taking_entry_is_placed():
    """Every function of include/isx.h whose last parameter is the stream, and the entry of include/isx_prep.h, has a case in TABLE or a quoted
    reason in LIMITED -- never both."""
    names = stream_entries()
    assert len(names) >= 70 and "isx_l2norm_rows" in names and "isx_tree_sum_rows" in names and "isxp_channel_moments_u8" in names and "isx_version" not in names, names
    tabled = {entry for _, entry, _ in TABLE}
    assert not tabled & set(LIMITED), sorted(tabled & set(LIMITED))
    missing = [n for n in names if n not in tabled and n not in LIMITED]
    assert not missing, ("stream-taking entries with neither a case nor a documented limit", missing)
    assert tabled <= set(names) and set(LIMITED) <= set(names), (sorted(tabled - set(names)), sorted(set(LIMITED) - set(names)))
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "isx.h")).read().replace(" * ", " "))
    for n, reason in LIMITED.items():                                        # the quoted condition stands in the header
        quotes = re.findall(r"'([^']+)'", reason)
        assert quotes and len(reason) > 40, n
        for q in quotes:
            assert all(re.sub(r"\s+", " ", part.strip()) in header for part in q.split("...")), (n, q)


@gpu
@pytest.mark.parametrize("cid", [i for i, _, _ in TABLE])
def test_large(cid):
    _built(cid).run()


# ---- limits that an entry states: the first shape past the limit is refused and nothing is written ---------------------------------------------------
def _refused(call, outs, message):
    from isx._lib import lib
    L = lib()
    torch.cuda.synchronize()
    rc = call(L, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == -1 and message in L.isx_last_error().decode(), (rc, L.isx_last_error())
    for r in outs:
        assert r.unwritten() == r.n and r.guards_intact(), "a refused call wrote"


@gpu
def test_wgrad_refuses_past_its_stated_limits():
    """include/isx.h at isx_conv_wgrad_nhwc: leaves <= 4096, leaves x S <= 65535, B H W < 2^31.  The case above runs 4093 leaves x 16 splits = 65 488;
    here 4097 leaves (of one pixel: S = 1), and 4096 leaves whose 16 splits would need a grid z extent of 65 536."""
    C = 64
    dw, db = G.out_f32((4097 * 16 * C * C,), 4096), G.out_f32((4097 * 16 * C,), 4096)
    x = G.in_f32(np.zeros((4097 * C,), F), 4096)
    big = torch.zeros(4096 * 8192 * C, dtype=torch.float32, device="cuda")       # 4096 leaves of 8192 pixels: the operands exist, the call is refused
    try:
        _refused(lambda L, st: L.isx_conv_wgrad_nhwc(x.ptr, x.ptr, 4097, 4097, 1, 1, C, C, 1, 1, dw.ptr, db.ptr, st), (dw, db), "bad shape")
        from isx._lib import lib
        assert lib().isx_conv_wgrad_splits(8192, C, C, 1) == 16
        _refused(lambda L, st: L.isx_conv_wgrad_nhwc(big.data_ptr(), big.data_ptr(), 4096, 4096, 64, 128, C, C, 1, 1, dw.ptr, db.ptr, st), (dw, db), "z extent")
    finally:
        del big
        torch.cuda.empty_cache()


@gpu
def test_region_gather_refuses_past_its_stated_limit():
    """include/isx.h at isx_region_gather_l2: B < 65536 (one image per grid row).  65 536 images of a 1 x 1 x 4 map, one window each."""
    B, C = 65536, 4
    f, idx = G.in_f32(np.zeros((B, C), F), 4096), G.in_i64(np.zeros((B, 1), np.int64), 4096)
    rows = G.out_f32((B, 1, C), 4096)
    _refused(lambda L, st: L.isx_region_gather_l2(f.ptr, B, C, 1, 1, 1, 1, idx.ptr, 1, 1, None, EPS, rows.ptr, st), (rows,), "bad shape")
    _refused(lambda L, st: L.isx_region_gather_l2_nhwc(f.ptr, B, C, 1, 1, 1, 1, idx.ptr, 1, 1, None, EPS, rows.ptr, st), (rows,), "bad shape")


# ---- the whole trunk through the Python layer ------------------------------------------------------------------------------------------------------------
@gpu
def test_folded_trunk_on_2680_images():
    """net.features (the folded channels-last ResNet-50 trunk of bench.py) on 2680 images of 224 x 224 built from a period of 5: the layer-1
    activations are 2680 x 56 x 56 x 256 = 2.15e9 floats, so conv1x1_stream_applicable, the position-major rule and the tail grids see sizes whose
    byte counts change sign in 32 bits.  The output equals 536 repeats of the B = 5 run bit for bit, and the B = 5 run agrees with the unfolded
    torch trunk inside the bound of tests/test_gpu_dropin.py::test_bias_act_and_folded_trunk."""
    from bench_legs.common import build_net
    B, period = 2680, 5
    dev = torch.device("cuda")
    net = build_net("resnet50", "f32", dev, channels_last=True, fold_bn=True)
    plain = build_net("resnet50", "f32", dev, channels_last=False, fold_bn=False)
    x5 = torch.from_numpy(_normal(_rng(B, period, 80), period, 3, 224, 224)).cuda()
    assert LG.check_period(x5.cpu().numpy(), period, "images") >= LG.MIN_DIFFER
    try:
        with torch.no_grad():
            ref = plain.features(x5)
            out5 = net.features(x5.contiguous(memory_format=torch.channels_last))
            assert float((out5 - ref).abs().max()) <= 2e-4 * float(ref.abs().max())
            del plain, ref
            big = x5.repeat(B // period, 1, 1, 1).contiguous(memory_format=torch.channels_last)
            out = net.features(big)
            del big
        torch.cuda.synchronize()
        assert out.shape[0] == B and out.permute(0, 2, 3, 1).is_contiguous() and out5.permute(0, 2, 3, 1).is_contiguous()
        LG.assert_periodic(out.permute(0, 2, 3, 1).reshape(-1).view(torch.int32), out5.permute(0, 2, 3, 1).reshape(-1).view(torch.int32), None, "trunk output")
    finally:
        torch.cuda.synchronize()
        out = out5 = net = None
        torch.cuda.empty_cache()


@gpu
def test_the_comparison_itself_past_the_line():
    """The tiling and the comparison of tests/_large.py on the device at the size of the cases: an int32 tensor of 2^31 + 4099 elements tiled from a
    period of 131 x 67 holds, at six probes around 2^31 and at both ends, the element that the host arithmetic names; it compares clean; and
    one flipped bit just past 2^31 and one in the last element are reported with their exact indices.  (A torch copy or comparison that
    wrapped at 2^31 would otherwise make every case here pass or fail for the wrong reason.)"""
    n, P = LG.LINE + 4099, 131 * 67
    block = torch.from_numpy(np.random.default_rng(1).integers(-1 << 31, 1 << 31, P, dtype=np.int64).astype(np.int32)).cuda()
    t = torch.full((n,), G.POISON_I32, dtype=torch.int32, device="cuda")
    try:
        LG.tile_into(t, block)
        for i in (0, 1, P - 1, P, LG.LINE - 1, LG.LINE, LG.LINE + 1, (1 << 30) + 5, n - 1):
            assert int(t[i]) == int(block[i % P]), i
        assert LG.mismatches(t, block, G.POISON_I32) == (0, None, None, 0)
        t[LG.LINE + 3] ^= 4
        t[n - 1] ^= 1
        assert LG.mismatches(t, block, G.POISON_I32) == (2, LG.LINE + 3, n - 1, 0)
        t[n - 1] = G.POISON_I32
        with pytest.raises(AssertionError, match=r"2 of %d elements wrong, 1 still poison; first wrong flat index %d \(mod 536870912: 3, 1073741824: 3, 2147483648: 3\)" % (n, LG.LINE + 3)):
            LG.assert_periodic(t, block, G.POISON_I32, "probe")
    finally:
        del t
        torch.cuda.empty_cache()
