"""Guarded device buffers for the tests that call the C ABI directly (test_gpu_trunk_guards.py, test_gpu_retrieval_guards.py,
test_gpu_fast_guards.py, test_gpu_eval_guards.py).

A Region is ONE allocation: a leading guard, the body, a trailing guard.  The guards hold a sentinel bit pattern and are compared bit for bit
after every launch; an OUTPUT body starts as a poison pattern (a NaN with a payload no kernel produces, or an integer no kernel produces) and
must not hold it afterwards; an INPUT body holds the data and its guards are NaNs, so that an operand read past either end reaches the output
as a NaN.  Unlike _guarded / _guards_intact of test_gpu_triplet_chains.py the guard size is chosen per call (it has to cover every address a
dead row of the last tile maps to) and the body may start `offset` elements past a 256-byte boundary (offset = 1: a pointer that is only
4-byte aligned).  All comparisons are on integer views: a legitimate NaN is never mistaken for the poison."""
import numpy as np
import torch

POISON_F32 = 0x7FC0DEAD                      # a quiet NaN with a payload
GUARD_OUT_F32 = 0xC640E400                   # -12345.0f
GUARD_IN_F32 = 0x7FC0BEEF                    # NaN around the operands
POISON_I64 = -(1 << 62)
POISON_I32 = -(1 << 30)
GUARD_I64 = -12345
POISON_F64 = 0x7FF8DEAD0000DEAD              # a quiet NaN with a payload, as int64 bits
GUARD_U8 = 0xA5
POISON_U8 = 0xCD
POISON_F16 = 0x7EAD                          # a quiet half NaN with a payload (a conversion of a NaN gives 0x7E00 | top payload bits of the source)
GUARD_OUT_F16 = 0xF1E2                       # -12048.0 as a half
GUARD_IN_F16 = 0x7EEF                        # half NaN around the fp16 operands

_KIND = {  # kind -> (storage dtype, view dtype, guard, poison)
    "f32": (torch.int32, torch.float32, GUARD_OUT_F32, POISON_F32),
    "i32": (torch.int32, torch.int32, GUARD_I64, POISON_I32),
    "i64": (torch.int64, torch.int64, GUARD_I64, POISON_I64),
    "f64": (torch.int64, torch.float64, GUARD_I64, POISON_F64),
    "u8": (torch.uint8, torch.uint8, GUARD_U8, POISON_U8),
    "f16": (torch.int16, torch.float16, GUARD_OUT_F16, POISON_F16),
}


def _signed(v, dtype):
    bits = {torch.int16: 16, torch.int32: 32, torch.int64: 64}.get(dtype)
    return v - (1 << bits) if bits and v >= 1 << (bits - 1) else v


class Region:
    def __init__(self, kind, shape, guard, offset=0, data=None, guard_value=None):
        store, view, g, poison = _KIND[kind]
        self.kind, self.shape, self.view_dtype = kind, tuple(int(s) for s in np.atleast_1d(shape)), view
        self.n = int(np.prod(self.shape))
        item = torch.empty((), dtype=store).element_size()
        per256 = 256 // item
        lead = -(-int(guard) // per256) * per256              # the body at offset 0 sits on a 256-byte boundary of the allocation
        self.start = lead + int(offset)
        self.guard_value = _signed(g if guard_value is None else guard_value, store)
        self.poison = _signed(poison, store)
        self.buf = torch.full((self.start + self.n + int(guard),), self.guard_value, dtype=store, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        body = self.buf[self.start:self.start + self.n]
        if data is None:
            body.fill_(self.poison)
        else:
            a = np.ascontiguousarray(data)
            assert a.size == self.n and a.dtype.itemsize == item, (a.shape, a.dtype, self.shape)
            body.copy_(torch.from_numpy(a.reshape(-1).view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[item])))
        self.ptr = self.buf.data_ptr() + self.start * item
        assert self.ptr % item == 0 and (offset or self.ptr % 256 == 0)

    @property
    def body(self):
        """The body as a tensor of the element type (a view: no copy)."""
        b = self.buf[self.start:self.start + self.n]
        return (b if b.dtype == self.view_dtype else b.view(self.view_dtype)).view(*self.shape)

    def raw(self):
        """The body as the integer storage type, flat: what bit comparisons use."""
        return self.buf[self.start:self.start + self.n]

    def guards_intact(self):
        return bool((self.buf[:self.start] == self.guard_value).all()) and bool((self.buf[self.start + self.n:] == self.guard_value).all())

    def unwritten(self):
        return int((self.raw() == self.poison).sum())

    def host(self):
        return self.body.cpu().numpy()


def out_f32(shape, guard, offset=0):
    return Region("f32", shape, guard, offset)


def out_i64(shape, guard, offset=0):
    return Region("i64", shape, guard, offset)


def out_f64(shape, guard, offset=0):
    return Region("f64", shape, guard, offset)


def out_f16(shape, guard, offset=0):
    """An fp16 output (int16 storage): poisoned with a half NaN no conversion produces, between sentinel guards."""
    return Region("f16", shape, guard, offset)


def in_f16(a, guard, offset=0):
    """An fp16 operand between half-NaN guards.  offset counts halfs: the fp16 GEMM needs 16-byte aligned operands (offset % 8 == 0)."""
    a = np.ascontiguousarray(a, np.float16)
    return Region("f16", a.shape, guard, offset, data=a, guard_value=GUARD_IN_F16)


def in_f32(a, guard=1024, offset=0):
    """An fp32 operand between NaN guards."""
    a = np.ascontiguousarray(a, np.float32)
    return Region("f32", a.shape, guard, offset, data=a, guard_value=GUARD_IN_F32)


def in_i32(a, guard=1024, offset=0):
    """int32 labels between guards of a label no case uses."""
    a = np.ascontiguousarray(a, np.int32)
    return Region("i32", a.shape, guard, offset, data=a)


def in_i64(a, guard=1024, offset=0):
    a = np.ascontiguousarray(a, np.int64)
    return Region("i64", a.shape, guard, offset, data=a)


def in_f32_io(a, guard, offset=0):
    """An fp32 buffer a kernel updates in place: the data between SENTINEL guards."""
    a = np.ascontiguousarray(a, np.float32)
    return Region("f32", a.shape, guard, offset, data=a)


def workspace(nbytes, guard=4096):
    """A byte workspace of exactly nbytes on a 256-byte boundary, at least 4 KiB of a byte pattern on both sides."""
    assert guard >= 4096
    return Region("u8", (max(int(nbytes), 1),), guard)


def ptr(r):
    return None if r is None else r.ptr


def assert_clean(outs, ins=(), what=""):
    """After a launch: every guard intact, no output element still poison.  Synchronises (the reductions read the buffers)."""
    for i, r in enumerate(ins):
        assert r is None or r.guards_intact(), ("guard of input %d overwritten" % i, what)
    for i, r in enumerate(outs):
        assert r.guards_intact(), ("store outside output %d" % i, what)
        left = r.unwritten()
        assert left == 0, ("output %d: %d of %d elements never written" % (i, left, r.n), what)


def bits(a):
    """Host array -> its unsigned bit pattern (fp16 -> uint16, fp32 -> uint32, fp64 -> uint64)."""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_bits(got, want, what=""):
    got = got.host() if isinstance(got, Region) else (got.cpu().numpy() if isinstance(got, torch.Tensor) else got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = bits(got) != bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


def assert_special(got, want, what="", fold_zero_sign=False):
    """assert_bits for operands with NaN, infinities and subnormals (tests/test_gpu_special_values.py): the NaN positions are the same set, every
    other element is equal bit for bit; the sign and payload of a NaN are free.  fold_zero_sign: -0 counts as +0 (max(-0, +0) of the bias and
    pool kernels under ReLU only: the one sign IEEE leaves open)."""
    from _special_values import compare
    got = got.host() if isinstance(got, Region) else (got.cpu().numpy() if isinstance(got, torch.Tensor) else got)
    compare(got, np.asarray(want), what, fold_zero_sign)


def assert_same_special(a, b, what=""):
    """Two device results of one call under assert_special's rule, compared on the device (large bodies)."""
    a, b = (r.body if isinstance(r, Region) else r for r in (a, b))
    na, nb = torch.isnan(a), torch.isnan(b)
    assert torch.equal(na, nb), ("NaN positions differ between the two runs", what, int((na != nb).sum()))
    bad = (a.contiguous().view(torch.int32) != b.contiguous().view(torch.int32)) & ~na
    assert not bool(bad.any()), ("bits differ between the two runs", what, int(bad.sum()))


# ---- host arithmetic of the launchers (csrc/gemm.hip, csrc/conv.hip), restated so that a case can assert the path it means to take ----------
def tail_split_rows(M, N, slots=512):
    """gemm_tail_split_rows: rows covered by whole rounds of 128x128 tiles when the last round is partial (0: no split)."""
    tn = (N + 127) // 128
    tiles = ((M + 127) // 128) * tn
    if tn > slots or slots % tn:
        return 0
    rounds = tiles // slots
    rem = tiles - rounds * slots
    if rounds < 1 or rem == 0 or rem > slots * 4 // 5:
        return 0
    return rounds * (slots // tn) * 128


def pos_major_rows(B, H, W, Cin, Ho, Wo, Cout, tiles_n64):
    """conv3x3_pos_major_rows: virtual rows of a position-major launch, 0 = pixel-major."""
    P = Ho * Wo
    ok = Cin % 64 == 0 and B >= 128 and P <= 28 * 28 and (128 * H * W + 2 * W + 4) * Cin * 4 < (1 << 32) and 128 * P * Cout * 4 < (1 << 31)
    groups = (B + 127) // 128
    return groups * P * 128 if ok and groups * P * 2 * tiles_n64 < (1 << 31) else 0


def stream_applicable(M, Cin, Cout, x_ptr):
    """conv1x1_stream_applicable"""
    return Cin == 64 and Cout in (64, 256) and M >= 16384 and x_ptr % 16 == 0


# ---- host arithmetic of the fp16 search (csrc/fast.hip, csrc/cosine.hip), restated for tests/test_gpu_fast_guards.py ---------------------------
HBK = 64                                      # csrc/fast.hip:164  constexpr int HBK = 64  (halfs per k-tile)
GBM = GBN = 256                               # csrc/fast.hip:290  constexpr int GBM = 256, GBN = 256
F16_GEMMS = ("cosine_gemm_f16_kernel<false>", "cosine_gemm_f16_kernel<true>",
             "cosine_gemm_f16_big_kernel<false,false>", "cosine_gemm_f16_big_kernel<false,true>",
             "cosine_gemm_f16_big_kernel<true,false>", "cosine_gemm_f16_big_kernel<true,true>",
             "gemm_f16_pp_kernel<false>", "gemm_f16_pp_kernel<true>")     # <FILTER> / <FILTER,FULLK>: the eight instantiations of csrc/fast.hip


def f16_gemm_kernel(tile, M, N, D, filt):
    """launch_gemm_f16 (csrc/fast.hip:671-698): the instantiation ONE launch of M x N x D runs under isx_debug_set_f16_tile(tile);
    filt = the launch has group flags (a filtered chunk of the search).  None: an empty launch."""
    if M == 0 or N == 0:
        return None
    btm, btn = (M + GBM - 1) // GBM, (N + GBN - 1) // GBN
    big = tile >= 1 if tile >= 0 else btm * btn >= 512                        # :679
    f = "true" if filt else "false"
    if not big:
        return "cosine_gemm_f16_kernel<%s>" % f                                # :694-695
    fullk = D % HBK == 0                                                      # :682
    if fullk and tile != 2:                                                   # :683-685
        return "gemm_f16_pp_kernel<%s>" % f
    return "cosine_gemm_f16_big_kernel<%s,%s>" % (f, "true" if fullk else "false")    # :686-689


def a256(v):
    return (v + 255) // 256 * 256


def topk_fixed_bytes(M, k):
    """csrc/cosine.hip:26"""
    return a256(M * k * 8) + a256(M * 4)


def topk_chunk_bytes(M, nc):
    """csrc/cosine.hip:27"""
    return a256(M * ((nc + 31) // 32)) + M * nc * 4


def fast_kl(k):
    """csrc/fast.hip:857-863: candidates kept per query by the approximate pass."""
    return min(max((200 * k // 100 + 32 + 31) // 32 * 32, 64), 256)


def topk_chunks(M, N, k, avail, f16):
    """run_topk_chunks (csrc/cosine.hip:41-116) for k <= 256: the column chunks [(c0, width, filtered)] of a search whose workspace holds `avail`
    bytes (everything of the job's workspace, the fixed part included).  The first chunk is always plain (and short only from N = 32768 on),
    every later one runs the filter epilogue with ngrp = ceil(width / 32)."""
    assert k <= 256
    fixed, min_nc = topk_fixed_bytes(M, k), min(N, 128)
    assert avail >= fixed + topk_chunk_bytes(M, min_nc)
    nc = min((avail - fixed) // (M * 4), N)
    while nc > min_nc and topk_chunk_bytes(M, nc) > avail - fixed:
        nc = max(nc - (1024 if nc > 4096 else 128), min_nc)
    if nc < N and nc >= 128:
        nc = nc // 128 * 128
    if nc < N and nc >= 4096:
        tile, slots = (256, 256) if f16 else (128, 512)
        tm, tn, tries = (M + tile - 1) // tile, nc // tile, 0
        while tries < 16 and tn > 16:
            rem = tm * tn % slots
            if rem == 0 or rem >= slots * 9 // 10:
                nc = tn * tile
                break
            tn, tries = tn - 1, tries + 1
    out, c0 = [], 0
    while c0 < N:
        w = min(N - c0, nc)
        if c0 == 0 and w > 8192 and N >= 4 * 8192:
            w = 8192
        out.append((c0, w, c0 != 0))
        c0 += w
    return out


def fast_layout(M, N, D, k, own_gallery):
    """fast_layout (csrc/fast.hip:866-891): (offset of the chunk area shared by the two pipelines, bytes of isx_cosine_topk_fast_workspace)."""
    o = a256(M * D * 2) + a256(M * 4) + 256 + (a256(N * D * 2) if own_gallery else 0) + 256 + 2 * a256(M * 4) + 256 + a256(M * D * 4)
    nc = N if M * N * 4 <= 1 << 30 else min(max((1 << 30) // (M * 4) // 2048 * 2048, 2048), N)
    return o, o + topk_fixed_bytes(M, fast_kl(k)) + topk_chunk_bytes(M, nc)
