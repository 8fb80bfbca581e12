"""Integer model of isxs_resize_cubic_u8 (include/isx_scale.h, csrc/scale.hip), written from the definition and independent of isx/scale.py:
the tables come from Python integers (unbounded, // is floor division), one output index at a time; the pixels are the 16-tap double sum in
int64 numpy.  Imports nothing from the library.  tests/test_resize_model.py pins the host twin to it and it to float64 torch bicubic;
tests/test_gpu_resize.py pins the kernel to it.  Also the case table both files share."""
import functools

import numpy as np

import _augment_model as A

# (Hs, Ws, Hd, Wd)
CASES = [(1, 1, 4, 4), (5, 7, 3, 4), (7, 5, 7, 9), (2, 3, 9, 1), (64, 64, 65, 63), (37, 53, 224, 299), (300, 200, 448, 299),
         (448, 448, 224, 224), (448, 597, 224, 299), (1000, 30, 10, 90)]
KINDS = ("random", "bw", "ramp")
# (Hs, Ws, max_ar, (top, left, Hp, Wp), (Hd, Wd)): the pad cases of the issue, each resized to a short side of 8
PAD_CASES = [(10, 30, 2.0, (3, 0, 15, 30), (8, 16)), (30, 10, 2.0, (0, 3, 30, 15), (16, 8)), (9, 30, 2.0, (3, 0, 15, 30), (8, 16))]
WIDE = (2, 8, 4100, 8, 2050)                       # (B, Hs, Ws, Hd, Wd): several column tiles, rows of 6150 bytes (not a multiple of 16)


def case_id(c):
    return "%dx%d-%dx%d" % tuple(c)


def tables(S, T):
    """(taps, coefficients): two lists of T rows of 4 Python integers."""
    D = 2 * T
    D3 = D ** 3

    def nearest(n):                                 # n / D^3 to the nearest integer, ties toward +infinity
        return (2 * n + D3) // (2 * D3)

    def n1(q):
        return 2560 * q ** 3 - 4608 * q * q * D + 2048 * D3
    taps, coef = [], []
    for j in range(T):
        num = (2 * j + 1) * S - T
        s = num // D
        r = num - s * D
        assert 0 <= r < D
        c0, c1, c2 = nearest(-1536 * r * (D - r) ** 2), nearest(n1(r)), nearest(n1(D - r))
        coef.append([c0, c1, c2, 2048 - c0 - c1 - c2])
        taps.append([min(max(s - 1 + k, 0), S - 1) for k in range(4)])
    return taps, coef


def padded(img, top, left, Hp, Wp, seed, noise_id):
    """The virtual padded image P as an array (Hp,Wp,3): tests/_augment_model.noise outside, `img` inside."""
    img = np.asarray(img)
    Hs, Ws = img.shape[:2]
    if (top, left, Hp, Wp) == (0, 0, Hs, Ws):
        return img
    P = A.noise(seed, noise_id, Hp, Wp).copy()
    P[top:top + Hs, left:left + Ws] = img
    return P


def resize_padded(P, Hd, Wd):
    """(Hp,Wp,3) uint8 -> (Hd,Wd,3) uint8."""
    Hp, Wp = P.shape[:2]
    ty, cy = (np.array(v, np.int64) for v in tables(Hp, Hd))
    tx, cx = (np.array(v, np.int64) for v in tables(Wp, Wd))
    P = P.astype(np.int64)
    acc = np.zeros((Hd, Wd, 3), np.int64)
    for i in range(4):
        for j in range(4):
            acc += (cy[:, i, None] * cx[None, :, j])[:, :, None] * P[ty[:, i, None], tx[None, :, j]]
    return np.clip((acc + 2 ** 21) >> 22, 0, 255).astype(np.uint8)


def resize(img, size, pad=None, seed=0, noise_ids=None):
    """(B,Hs,Ws,3) uint8 -> (B,Hd,Wd,3) uint8: the arguments of isx.scale.resize_cubic_u8 on numpy arrays."""
    img = np.asarray(img)
    B, Hs, Ws = img.shape[:3]
    top, left, Hp, Wp = pad if pad is not None else (0, 0, Hs, Ws)
    ids = [0] * B if noise_ids is None else [int(v) for v in noise_ids]
    return np.stack([resize_padded(padded(img[b], top, left, Hp, Wp, seed, ids[b]), size[0], size[1]) for b in range(B)])


def image(kind, H, W, B=1, salt=0):
    """(B,H,W,3) uint8: random bytes, random 0 / 255, or a diagonal ramp that wraps every 256 steps (a different step per channel)."""
    rng = np.random.default_rng(1000003 * H + 1009 * W + 17 * B + salt)
    if kind == "random":
        return rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    if kind == "bw":
        return (rng.integers(0, 2, (B, H, W, 3), dtype=np.uint8) * 255).astype(np.uint8)
    y, x, c, b = np.ogrid[0:H, 0:W, 0:3, 0:B]
    return np.ascontiguousarray(np.moveaxis((3 * y + (5 + 2 * c) * x + 40 * c + 11 * b) % 256, -1, 0).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def case(c, kind):
    """(image (1,Hs,Ws,3), its model result (1,Hd,Wd,3)) of a case of CASES: computed once per process, read-only."""
    Hs, Ws, Hd, Wd = c
    img = image(kind, Hs, Ws)
    want = resize(img, (Hd, Wd))
    img.setflags(write=False)
    want.setflags(write=False)
    return img, want


def float_bicubic(img, size):
    """float64 torch bicubic (a = -3/4, half-pixel centres, replicated border, no antialiasing) of a (B,H,W,3) uint8 array -> (B,Hd,Wd,3) float64."""
    import torch
    x = torch.from_numpy(np.array(img)).permute(0, 3, 1, 2).double()
    y = torch.nn.functional.interpolate(x, size=tuple(size), mode="bicubic", align_corners=False)
    return y.permute(0, 2, 3, 1).contiguous().numpy()
