"""Periodic operands past 2^31 elements and a full-coverage bit comparison (tests/test_gpu_large_tensors.py; tests/test_large_model.py proves
the detecting power on the CPU).

A host reference for 8 GB of output is out of reach, and every entry of include/isx.h documents that a row, image or leaf of its result
depends on that row, image or leaf alone.  So an operand that crosses the 2^31-element line is a small PERIOD BLOCK of random rows tiled on
the device, the reference is computed for one period on the CPU, and EVERY element of the device's output is compared, as integers, with that
block broadcast over the repeats (mismatches / assert_periodic).

The period must not hide a wrap.  A kernel that reads x[i - 2^k] for x[i] is invisible when the period divides 2^k, so a period is an odd prime
number of rows: check_period asserts, for every shift of 2^k elements with k in SHIFTS, that the shift is no multiple of the period and that
the block's values at two positions that far apart differ for at least MIN_DIFFER of the positions (a constant or low-entropy block fails).
A prime number of rows also walks every tile phase: neither 64, 128 nor 256 divides it."""
import numpy as np
import torch

import _guards as G

SHIFTS = tuple(range(29, 35))                  # 2^29 .. 2^34 elements; the same shifts in BYTES of 1..8-byte elements lie in this range too
MODS = (1 << 29, 1 << 30, 1 << 31)
MIN_DIFFER = 0.99
LINE = 1 << 31                                 # elements; x 4 bytes = 8 GiB, so the 2 GiB and 4 GiB byte lines are passed with it
CHUNK = 1 << 27                                # elements compared at once: the boolean temporary and its reductions stay far below 2 GB
_INT = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}
_KIND = {np.dtype(np.float32): "f32", np.dtype(np.int32): "i32", np.dtype(np.int64): "i64", np.dtype(np.uint8): "u8", np.dtype(np.float16): "f16",
         np.dtype(np.float64): "f64", np.dtype(np.uint64): "i64"}
_IN_GUARD = {"f32": G.GUARD_IN_F32, "f16": G.GUARD_IN_F16}


def is_odd_prime(p):
    return p >= 3 and p % 2 == 1 and all(p % d for d in range(3, int(p ** 0.5) + 1, 2))


def as_ints(a):
    """Host array -> flat array of its bit patterns (a copy; the signed integer type of the element size)."""
    a = np.array(a, order="C")
    return a.reshape(-1).view(_INT[a.dtype.itemsize])


def check_period(block, rows, what, shifts=SHIFTS, min_differ=MIN_DIFFER):
    """block: the period of an operand, `rows` rows (images, leaves) of block.size / rows elements.  Asserts the rules above and returns the
    smallest share of differing positions over the shifts."""
    bits = as_ints(block)
    P = bits.size
    assert is_odd_prime(rows), (what, "the period is %d rows: not an odd prime" % rows)
    assert P % rows == 0, (what, P, rows)
    worst = 1.0
    for k in shifts:
        s = (1 << k) % P
        assert s != 0, (what, "a shift of 2^%d elements is a multiple of the period of %d elements: a wrap by it would be invisible" % (k, P))
        share = float(np.count_nonzero(bits != np.roll(bits, -s))) / P
        worst = min(worst, share)
        assert share >= min_differ, (what, "only %.4f of the positions differ from the one 2^%d elements on: the block would hide a wrap" % (share, k))
    return worst


# ---- the comparison (host or device tensors) -----------------------------------------------------------------------------------------------------
def mismatches(got, want, poison=None, chunk=CHUNK):
    """got: flat integer tensor of n elements; want: flat integer tensor of the period's P elements (same dtype and device).  Element i of got
    must equal want[i % P].  Returns (number of wrong elements, first wrong flat index, last wrong flat index, elements still `poison`)."""
    assert got.dim() == 1 and want.dim() == 1 and got.dtype == want.dtype and got.device == want.device and not got.dtype.is_floating_point
    n, P = got.numel(), want.numel()
    step = max(1, chunk // P) * P
    count, first, last, left = 0, None, None, 0
    for pos in range(0, n, step):
        seg = got[pos:pos + step]
        m = seg.numel()
        whole = m // P
        bad = torch.empty(m, dtype=torch.bool, device=got.device)
        if whole:
            torch.ne(seg[:whole * P].view(whole, P), want, out=bad[:whole * P].view(whole, P))
        if m > whole * P:
            torch.ne(seg[whole * P:], want[:m - whole * P], out=bad[whole * P:])
        if poison is not None:
            left += int((seg == poison).sum())
        c = int(bad.sum())
        if c:
            b8 = bad.view(torch.uint8)
            if first is None:
                first = pos + int(b8.argmax())
            last = pos + m - 1 - int(b8.flip(0).argmax())
            count += c
        del bad
    return count, first, last, left


def describe(count, first, last, left, n, what, mods=MODS):
    at = lambda i: "%d (mod %s)" % (i, ", ".join("%d: %d" % (m, i % m) for m in mods))
    return "%s: %d of %d elements wrong, %d still poison; first wrong flat index %s; last %s" % (what, count, n, left, at(first), at(last))


def assert_periodic(got, want, poison=None, what="", chunk=CHUNK, mods=MODS):
    """Every element of the flat integer tensor `got` equals the period `want` broadcast over the repeats, and none is still poison."""
    count, first, last, left = mismatches(got, want, poison, chunk)
    if count or left:
        if first is None:                       # poison that the period itself holds: a broken case, not a broken kernel
            raise AssertionError("%s: %d elements equal the poison although they match the expected period" % (what, left))
        P = want.numel()
        raise AssertionError(describe(count, first, last, left, got.numel(), what, mods) +
                             "; there got 0x%x, want 0x%x" % (int(got[first]) & (1 << 8 * got.element_size()) - 1,
                                                              int(want[first % P]) & (1 << 8 * got.element_size()) - 1))


def tile_into(body, block):
    """body: flat tensor of n elements; block: flat tensor of P.  body[i] = block[i % P], written on body's device without a temporary."""
    n, P = body.numel(), block.numel()
    whole = n // P
    if whole:
        body[:whole * P].view(whole, P).copy_(block.view(1, P).expand(whole, P))
    if n > whole * P:
        body[whole * P:].copy_(block[:n - whole * P])
    return body


# ---- device side ---------------------------------------------------------------------------------------------------------------------------------
class Periodic(object):
    """An operand of `rows` rows, row r a copy of row r % period of `block` ((period, ...) host array).  The host rules are checked here,
    for every operand that reaches the smallest shift (a smaller one cannot be wrapped by it), and `share` keeps the smallest share of
    differing positions.
    parts > 1: the operand is `parts` such matrices one after the other ((P, M, k) lists, the L rows of a tree sum, the K rows of a transposed
    activation), block (parts, period, ...), part q tiled from block[q].  The flat operand then has no single period; the rule itself is checked
    instead, on SAMPLES positions per shift: the element a shift of 2^k before position i differs from the one at i."""
    SAMPLES = 1 << 18

    def __init__(self, block, rows, what="", guard=4096, must_cross=False, parts=1):
        self.block, self.rows, self.parts, self.guard = np.ascontiguousarray(block), int(rows), int(parts), guard
        self.period = int(self.block.shape[0] if parts == 1 else self.block.shape[1])
        self.row_elems = self.block.size // (self.period * self.parts)
        self.part_n = self.rows * self.row_elems
        self.n = self.parts * self.part_n
        self.crosses = self.n > LINE
        assert self.crosses or not must_cross, (what, "%d elements: below the line" % self.n)
        assert parts == 1 or self.block.shape[0] == parts
        if self.n <= 1 << SHIFTS[0]:
            self.share = None
        elif parts == 1:
            self.share = check_period(self.block, self.period, what)
        else:
            self.share = self._check_sampled(what)

    def _check_sampled(self, what):
        assert is_odd_prime(self.period), (what, "the period is %d rows: not an odd prime" % self.period)
        bits = as_ints(self.block).reshape(self.parts, -1)
        P = bits.shape[1]
        value = lambda i: bits[i // self.part_n, (i % self.part_n) % P]
        rng, worst = np.random.default_rng(P), 1.0
        for k in SHIFTS:
            if 1 << k >= self.n:
                break
            i = rng.integers(1 << k, self.n, self.SAMPLES)
            share = float(np.count_nonzero(value(i) != value(i - (1 << k)))) / self.SAMPLES
            worst = min(worst, share)
            assert share >= MIN_DIFFER, (what, "only %.4f of the sampled positions differ from the one 2^%d elements before" % (share, k))
        return worst

    @property
    def shape(self):
        return ((self.parts,) if self.parts > 1 else ()) + (self.rows,) + self.block.shape[(1 if self.parts == 1 else 2):]

    def region(self, io=False):
        """A guarded Region whose body holds the tiled operand: NaN guards around an fp operand, sentinel guards around an in-place one."""
        kind = _KIND[self.block.dtype]
        r = G.Region(kind, self.shape, self.guard, guard_value=None if io else _IN_GUARD.get(kind))
        block = torch.from_numpy(as_ints(self.block)).to(r.buf.dtype).cuda()
        if self.parts == 1:
            tile_into(r.raw(), block)
            return r
        body, block = r.raw().view(self.parts, self.part_n), block.view(self.parts, -1)
        P = block.shape[1]
        whole = self.part_n // P
        if whole:
            body[:, :whole * P].view(self.parts, whole, P).copy_(block.view(self.parts, 1, P).expand(self.parts, whole, P))
        if self.part_n > whole * P:
            body[:, whole * P:].copy_(block[:, :self.part_n - whole * P])
        return r


def assert_region_periodic(region, want_block, what, parts=1):
    """The whole body of an output Region against the expected period (host array), bit for bit; nothing poisoned, guards intact.  parts > 1:
    the output is `parts` matrices one after the other, want_block (parts, period, ...)."""
    want = np.ascontiguousarray(want_block)
    if parts > 1:
        assert region.guards_intact(), ("store outside", what)
        raw, w = region.raw().view(parts, -1), torch.from_numpy(as_ints(want)).to(region.buf.dtype).cuda().view(parts, -1)
        for q in range(parts):
            assert_periodic(raw[q], w[q], None if region.kind == "u8" else region.poison, "%s, part %d" % (what, q))
        return
    assert _KIND[want.dtype] == region.kind or (want.dtype == np.uint64 and region.kind == "i64"), (what, want.dtype, region.kind)
    assert region.guards_intact(), ("store outside", what)
    assert_periodic(region.raw(), torch.from_numpy(as_ints(want)).to(region.buf.dtype).cuda(), None if region.kind == "u8" else region.poison, what)
