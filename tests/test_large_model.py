"""The detecting power of tests/_large.py, proved on the CPU at a scaled-down modulus: 2^12 elements stand for the 2^30 (or 2^31, 2^32) at which
a 32-bit offset of a kernel would wrap.  The "kernel" is y[i] = 2 x[i] + 1 on int32 bit patterns, over an operand tiled from a period block as
tests/test_gpu_large_tensors.py tiles its operands; each simulated fault is what one wrong offset does to such a kernel's output.  No broken
kernel is ever run on a GPU to show this."""
import numpy as np
import pytest
import torch

import _large as LG

MOD = 1 << 12
ROW = 24                                       # elements per row
N_ROWS = 3 * MOD // ROW + 5                    # 12 k elements: the modulus is passed twice
POISON = LG.G.POISON_I32
SMALL_SHIFTS = (12, 13)
SMALL_MODS = (1 << 11, 1 << 12, 1 << 13)


def _block(rows, seed=0):
    return np.random.default_rng([rows, seed]).integers(-1 << 30, 1 << 30, (rows, ROW), dtype=np.int32)


def _tiled(block, n):
    return LG.tile_into(torch.empty(n, dtype=torch.int32), torch.from_numpy(block.reshape(-1)))


def _f(x):
    return x * 2 + 1                           # int32 arithmetic wraps: still a bijection of the bit patterns


def _setup(period_rows):
    block = _block(period_rows)
    n = N_ROWS * ROW
    x = _tiled(block, n)
    return block, n, x, torch.from_numpy(_f(block.reshape(-1)))


def _detects(got, want, chunk):
    with pytest.raises(AssertionError) as e:
        LG.assert_periodic(got, want, POISON, "simulated", chunk=chunk, mods=SMALL_MODS)
    return str(e.value)


CHUNKS = (1 << 27, 1000, 7 * ROW + 1)            # one chunk; chunks of several periods; chunks of a single period with a ragged end


@pytest.mark.parametrize("chunk", CHUNKS)
def test_correct_output_passes(chunk):
    block, n, x, want = _setup(7)
    LG.check_period(block, 7, "x", shifts=SMALL_SHIFTS)
    LG.assert_periodic(_f(x), want, POISON, "correct", chunk=chunk, mods=SMALL_MODS)
    assert LG.mismatches(_f(x), want, POISON, chunk) == (0, None, None, 0)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_wrapped_loads_are_flagged(chunk):
    """(a) y[i] = f(x[i mod 2^12]): right below the modulus, wrong for nearly every element from it on."""
    block, n, x, want = _setup(7)
    got = _f(x[torch.arange(n) % MOD])
    count, first, last, left = LG.mismatches(got, want, POISON, chunk)
    assert first >= MOD and first < MOD + 8 and last >= n - 8 and left == 0 and count >= 0.99 * (n - MOD)
    msg = _detects(got, want, chunk)
    assert "first wrong flat index %d (mod 2048: %d, 4096: %d, 8192: %d)" % (first, first % 2048, first % 4096, first % 8192) in msg


@pytest.mark.parametrize("chunk", CHUNKS)
def test_wrapped_stores_are_flagged(chunk):
    """(b) the store of element i lands at i mod 2^12: poison from the modulus on, the last writer's value below it."""
    block, n, x, want = _setup(7)
    got = torch.full((n,), POISON, dtype=torch.int32)
    for lo in range(0, n, MOD):                # in order: the last writer wins, as for blocks that run in order
        seg = _f(x[lo:lo + MOD])
        got[:seg.numel()] = seg
    count, first, last, left = LG.mismatches(got, want, POISON, chunk)
    assert left == n - MOD and last == n - 1 and first < 8 and count >= left + 0.99 * MOD         # every near-end element holds a later slab's value
    assert "%d still poison" % left in _detects(got, want, chunk)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_unwritten_tail_is_flagged(chunk):
    """(c) nothing written from the modulus on."""
    block, n, x, want = _setup(7)
    got = _f(x)
    got[MOD:] = POISON
    assert LG.mismatches(got, want, POISON, chunk) == (n - MOD, MOD, n - 1, n - MOD)
    _detects(got, want, chunk)


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("back", (1, 2 * ROW + 3, 7 * ROW))
def test_one_wrong_element_in_the_last_period_is_flagged(chunk, back):
    """(d) one element, one bit."""
    block, n, x, want = _setup(7)
    got = _f(x)
    got[n - back] ^= 1
    assert LG.mismatches(got, want, POISON, chunk) == (1, n - back, n - back, 0)
    assert "1 of %d elements wrong" % n in _detects(got, want, chunk)


def test_a_period_that_divides_the_modulus_hides_wrapped_loads():
    """Why the period is an odd prime number of rows: with a period of 2^7 elements the wrapped loads of (a) give the CORRECT output, the
    comparison passes, and only check_period refuses the case."""
    rows = 16                                   # 16 rows of 8 elements: 2^7
    block = np.random.default_rng(5).integers(-1 << 30, 1 << 30, (rows, 8), dtype=np.int32)
    n = 3 * MOD + 40
    x = _tiled(block, n)
    got = _f(x[torch.arange(n) % MOD])
    LG.assert_periodic(got, torch.from_numpy(_f(block.reshape(-1))), POISON, "hidden", mods=SMALL_MODS)        # passes: nothing seen
    with pytest.raises(AssertionError, match="not an odd prime"):
        LG.check_period(block, rows, "x", shifts=SMALL_SHIFTS)
    assert all((1 << k) % block.size == 0 for k in SMALL_SHIFTS)                                               # the rule behind the prime


def test_low_entropy_blocks_are_refused():
    for block in (np.zeros((7, ROW), np.float32), np.tile(np.arange(2, dtype=np.int32), (7, ROW // 2)),
                  np.maximum(np.random.default_rng(1).standard_normal((7, ROW), dtype=np.float32), 0)):      # half zeros: a quarter of the pairs equal
        with pytest.raises(AssertionError, match="would hide a wrap"):
            LG.check_period(block, 7, "x", shifts=SMALL_SHIFTS)
    assert LG.check_period(np.random.default_rng(2).standard_normal((7, ROW), dtype=np.float32), 7, "x", shifts=SMALL_SHIFTS) >= 0.99


def test_prime_rule():
    assert [p for p in range(1, 30) if LG.is_odd_prime(p)] == [3, 5, 7, 11, 13, 17, 19, 23, 29]
    for p in (131, 997, 4099):
        assert LG.is_odd_prime(p)
