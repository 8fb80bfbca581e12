"""CPU model of the canonical sums of the descriptor head's training kernels (csrc/head.hip, the FOLD path of csrc/wgrad_kernel.hpp), shared by
tests/test_head_model.py (the model against float64, and against the wrong orders it has to tell apart) and tests/test_gpu_head_chains.py (the
kernels against the model, bit for bit).

Every dot product is oracle.cosine_sim: a k-ordered fp32 fmaf chain from +0, the chain the fp32 MFMA computes (tests/test_gpu_parity.py).  Every
other add and multiply is a numpy float32 operation: one rounding each, never fused -- libisx is built with -ffp-contract=off.  No torch, no matmul."""
import functools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import oracle as O

F = np.float32
BK = 32                                           # k-tile of the head kernels


def chains(a, b):
    """(M, D), (N, D) -> (M, N): out[m][n] = the fmaf chain over d = 0 .. D-1 of a[m][d] * b[n][d], from +0.  Rows are independent: a large
    problem is cut by rows over a few threads (the C call releases the GIL)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    M = a.shape[0]
    n = min(8, os.cpu_count() or 1, M)
    if n <= 1 or M * b.shape[0] * a.shape[1] < (1 << 24):
        return O.cosine_sim(a, b)
    cuts = [M * i // n for i in range(n + 1)]
    with ThreadPoolExecutor(n) as pool:
        return np.concatenate(list(pool.map(lambda i: O.cosine_sim(a[cuts[i]:cuts[i + 1]], b), range(n))), 0)


def inputs(rows, cols, seed, special_rows=True):
    """Seeded standard normals, column c scaled by logspace(-2, 2)[c]: partial sums of different lengths round differently.  special_rows: row 2
    is all zero and row 3 is zero past column 0 (when there are that many rows)."""
    a = np.random.default_rng(seed).standard_normal((rows, cols)).astype(F) * np.logspace(-2, 2, cols).astype(F)
    if special_rows and rows > 3:
        a[2] = 0
        a[3, 1:] = 0
    return np.ascontiguousarray(a, F)


# ---- isx_head_linear_fwd / isx_head_linear_fwd_rows ---------------------------------------------------------------------------------------
def splits(K):
    """(S, kt_per, [(k_lo, k_hi) of split 0 .. S-1]): S = clamp(K // 2048, 1, 32) from K alone, kt_per = ceil((K / 32) / S) k-tiles per split."""
    S = min(max(K // (BK * 64), 1), 32)
    nk = K // BK
    kt_per = (nk + S - 1) // S
    return S, kt_per, [(BK * s * kt_per, min(K, BK * (s + 1) * kt_per)) for s in range(S)]


def linear_partials(x, w, ranges):
    """One chain per (output, k range)."""
    return [chains(x[:, lo:hi], w[:, lo:hi]) for lo, hi in ranges]


def add_in_order(parts):
    """((p_0 + p_1) + p_2) + ..."""
    y = parts[0].copy()
    for p in parts[1:]:
        y = y + p
    return y


def linear_fwd(x, w, bias=None):
    y = add_in_order(linear_partials(x, w, splits(x.shape[1])[2]))
    return y if bias is None else y + np.asarray(bias, F)[None, :]


# ---- isx_head_linear_dgrad / isx_head_linear_dgrad_parts ------------------------------------------------------------------------------------
def groups(N):
    return 8 if N % 256 == 0 else 1


def dgrad_parts(dy, w, Ng):
    """(groups, M, K): parts[g][m][k] = the chain over the n of group g (Ng consecutive output features) of dy[m][n] * w[n][k]."""
    G = dy.shape[1] // Ng
    assert G * Ng == dy.shape[1] == w.shape[0]
    wT = np.ascontiguousarray(w.T)
    return np.stack([chains(dy[:, g * Ng:(g + 1) * Ng], wT[:, g * Ng:(g + 1) * Ng]) for g in range(G)], 0)


def fold(parts):
    """((0 + c_0) + c_1) + ...: the second accumulator of the FOLD path."""
    tot = np.zeros(parts[0].shape, F)
    for c in parts:
        tot = tot + c
    return tot


def dgrad(dy, w):
    N = dy.shape[1]
    return fold(dgrad_parts(dy, w, N // groups(N)))


# ---- isx_head_sgd_step -------------------------------------------------------------------------------------------------------------------
def wgrad_rows(dy, x):
    """(N, K): g[n][k] = the chain over the rows r = 0 .. R-1 of dy[r][n] * x[r][k]."""
    return chains(np.ascontiguousarray(dy.T), np.ascontiguousarray(x.T))


def sgd_step(w, buf, g, first, lr, momentum, dampening, weight_decay, nesterov):
    """head_sgd_kernel's epilogue, operation by operation.  Returns (w, buf); buf passes through untouched (None allowed) without momentum."""
    lr, momentum, dampening, weight_decay = F(lr), F(momentum), F(dampening), F(weight_decay)
    if weight_decay != 0:
        g = g + weight_decay * w
    upd = g
    if momentum != 0:
        buf = g.copy() if first else momentum * buf + (F(1) - dampening) * g
        upd = g + momentum * buf if nesterov else buf
    return w - lr * upd, buf


# ---- isx_colsum_leaves -------------------------------------------------------------------------------------------------------------------
def colsum_leaves(x, leaves, R):
    """(leaves, C): s = 0; s += row_r for the R rows of the leaf in row order."""
    out = np.zeros((leaves, x.shape[1]), F)
    for l in range(leaves):
        for r in range(R):
            out[l] = out[l] + x[l * R + r]
    return out


# ---- the shapes both test files walk: the smallest that reach each launch variant and each boundary ------------------------------------------
FWD_K = (32, 2016, 4256, 6144)                    # one k-tile; S = 1, 63 tiles; S = 2, 67 + 66 tiles; S = 3, even
FWD_N = (64, 192, 256)                            # 192: not a multiple of 128
FWD_M = (1, 64, 65, 128, 129, 192, 193, 320)      # Mp = 64, 128, 192; two 192-row tiles, the second with one row; TM = 1 with 5 row tiles
FWD_CAP = (7, 64, 67744)                          # (M, N, K) at the cap: S = 32, kt_per = 67, the last split 40 tiles
# (N, K, rows) of the input gradient: G = 8 with fold_kt = 1, 3, 2; G = 1, the second with a zero-filled k-tile tail.  rows 24: Mp = 64; 128 with
# K = 128: the 2x2 tile; 192: the 3x1 tile; 256 with K = 192: the 1x1 tile over several row tiles
DGRAD_NK = ((256, 64), (768, 192), (512, 128), (192, 128), (100, 64))
DGRAD_CASES = tuple((N, K, M) for N, K in DGRAD_NK for M in (24, 128, 192, 256) if M in (24, 192) or (M == 128 and K == 128) or (M == 256 and K == 192))
PARTS_EXTRA = (96, 5, 64, 24)                     # (Ng, groups, K, rows): groups that are not the canonical eight
SGD_NK = ((64, 128), (192, 384), (256, 256))      # 64-row tile (N % 128 != 0) twice, 128-row tile
SGD_R = (0, 1, 24, 33, 77)
SGD_SETS = (                                      # lr, momentum, dampening, weight_decay, nesterov
    ("plain", 1e-2, 0.0, 0.0, 0.0, 0),
    ("decay", 1e-2, 0.0, 0.0, 5e-4, 0),
    ("momentum_dampening", 1e-2, 0.9, 0.1, 0.0, 0),
    ("momentum_decay", 1e-2, 0.9, 0.0, 5e-4, 0),
    ("nesterov_decay", 1e-2, 0.9, 0.0, 5e-4, 1),
)
SGD_UPDATE_NKR = ((192, 384, 33), (256, 256, 33))  # head_sgd_kernel<1> and <2>, the second k-tile of rows mostly zero fill
COLSUM_CASES = ((3, 5, 7), (2, 1, 300), (1, 24, 2048), (2, 0, 9))        # (leaves, R, C)


# ---- shared, read-only cases ----------------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def fwd_case(K):
    """(x, w, bias, partials, y without bias) of the forward pass at K for the LARGEST M and N of the list, computed once.  Output (m, n) is a
    function of row m of x and row n of w alone, so the model of a smaller case is the corner [:M, :N] of this one; the kernels are run at the
    smaller case's own M and N on the corner of the inputs."""
    M, N = FWD_CAP[:2] if K == FWD_CAP[2] else (max(FWD_M), max(FWD_N))
    x, w = inputs(M, K, K), inputs(N, K, K + 1, special_rows=False)
    bias = np.random.default_rng(K + 2).standard_normal(N).astype(F)
    parts = linear_partials(x, w, splits(K)[2])
    return _frozen(x, w, bias, np.stack(parts, 0), add_in_order(parts))


@functools.lru_cache(maxsize=None)
def dgrad_case(N, K, M):
    """(dy, w, parts of N / groups(N) features each, dx)."""
    dy, w = inputs(M, N, 7 * N + K + M), inputs(N, K, 7 * N + K + M + 1, special_rows=False)
    parts = dgrad_parts(dy, w, N // groups(N))
    return _frozen(dy, w, parts, fold(parts))


@functools.lru_cache(maxsize=None)
def parts_extra_case():
    """(dy, w, parts) of PARTS_EXTRA."""
    Ng, G, K, M = PARTS_EXTRA
    dy, w = inputs(M, Ng * G, 480), inputs(Ng * G, K, 481, special_rows=False)
    return _frozen(dy, w, dgrad_parts(dy, w, Ng))


@functools.lru_cache(maxsize=None)
def rows_case(N, K, R, seed=0):
    """(dy, x, g) of the weight gradient over R rows."""
    dy, x = inputs(R, N, 11 * N + K + R + 1000 * seed), inputs(R, K, 11 * N + K + R + 1000 * seed + 1)
    return _frozen(dy, x, wgrad_rows(dy, x))


def sgd_w0(N, K):
    """The weight the update tests start from: small against the first gradients, as a freshly initialised layer is."""
    return inputs(N, K, 5, special_rows=False) * F(0.01)


@functools.lru_cache(maxsize=None)
def colsum_case(leaves, R, C):
    x = inputs(leaves * R, C, 13 * C + R)
    return _frozen(x, colsum_leaves(x, leaves, R))
