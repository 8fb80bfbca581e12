"""Training-time augmentation of the reference (utils/image.py:128-187): affine_cv and random_affine_noisy_cv -- a random rotation / shift /
scale / flip through a cubic-spline warp (scipy.ndimage.affine_transform, order 3, mode 'constant') whose uncovered pixels are filled with random
bytes.  The arithmetic here is numpy only (scipy may be absent) and is the arithmetic of csrc/augment.hip (isx_affine_noisy_u8), float64, one
rounding per operation:

  prefilter   cubic B-spline coefficients, pole z = sqrt(3) - 2, mirror boundaries, axis 0 then axis 1
  warp        (yi, xi) = (t0 + m00 y + m01 x, t1 + m10 y + m11 x); outside iff yi < 0, yi > H - 1, xi < 0 or xi > W - 1; otherwise 4 x 4 taps
  cast        truncate toward zero, then modulo 256 (the reference's astype(np.uint8): cubic overshoot wraps, it is not clamped)
  noise       outside pixels get noise_byte(seed, noise_id, y, x, c), a counter-based generator (include/isx.h): NOT the reference's np.random
              stream, which would need the number of outside pixels of one image before the parameters of the next are drawn

The object random_affine_noisy_cv returns is callable on one (H,W,3) uint8 array, as in the reference (the --device=-1 path); the training
mains recognise it as P.train_trans and run the same operation per batch on the GPU (train/_common.py)."""
import random

import numpy as np

__all__ = ['RandomAffineNoisy', 'affine_cv', 'random_affine_noisy_cv']

POLE = np.sqrt(3.0) - 2.0
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1, _M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def _mix64(z):
    """The output function of splitmix64 on uint64 arrays (wrapping arithmetic)."""
    with np.errstate(over='ignore'):
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def noise_bytes(seed, noise_id, H, W):
    """(H,W,3) uint8: byte (y,x,c) = top byte of mix64(seed + GOLDEN * (noise_id * 3HW + 3 (y W + x) + c)), all modulo 2**64."""
    with np.errstate(over='ignore'):
        idx = np.uint64(int(noise_id) & (2 ** 64 - 1)) * np.uint64(3 * H * W) + np.arange(3 * H * W, dtype=np.uint64)
        z = _mix64(np.uint64(int(seed) & (2 ** 64 - 1)) + _GOLDEN * idx)
    return (z >> np.uint64(56)).astype(np.uint8).reshape(H, W, 3)


def _filter_lines(c):
    """In place along axis 0 of a float64 array (n, ...): the recursive cubic B-spline filter with mirror initialisation."""
    n = c.shape[0]
    if n == 1:
        return c
    z = POLE
    c *= (1.0 - z) * (1.0 - 1.0 / z)
    zn1 = 1.0
    for _ in range(n - 1):
        zn1 = zn1 * z
    c0 = c[0] + zn1 * c[n - 1]
    zi = z
    for i in range(1, n - 1):
        if abs(zi) < 1e-30:
            break
        c0 = c0 + zi * (c[i] + zn1 * c[n - 1 - i])
        zi = zi * z
    c[0] = c0 / (1.0 - zn1 * zn1)
    for i in range(1, n):
        c[i] = c[i] + z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * (z / (z * z - 1.0))
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return c


def spline_coefficients(img):
    """(H,W,C) -> float64 cubic B-spline coefficients of every channel (scipy.ndimage.spline_filter, order 3, mode 'mirror')."""
    c = np.array(img, dtype=np.float64)
    _filter_lines(c)
    _filter_lines(c.transpose(1, 0, 2))
    return c


def _mirror(i, n):
    if n == 1:
        return np.zeros_like(i)
    m = 2 * (n - 1)
    i = np.mod(i, m)
    return np.where(i > n - 1, m - i, i)


def _weights(t):
    u = 1.0 - t
    w1 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0
    w0 = u * u * u / 6.0
    return [w0, w1, w2, 1.0 - w0 - w1 - w2]


def warp(coeff, mat6):
    """coeff: (H,W,C) spline coefficients; mat6 = (m00, m01, t0, m10, m11, t1).  Returns (values (H,W,C) float64, outside (H,W) bool)."""
    H, W, _ = coeff.shape
    m00, m01, t0, m10, m11, t1 = [float(v) for v in mat6]
    y = np.arange(H, dtype=np.float64)[:, None]
    x = np.arange(W, dtype=np.float64)[None, :]
    yi = t0 + m00 * y + m01 * x
    xi = t1 + m10 * y + m11 * x
    outside = (yi < 0) | (yi > H - 1) | (xi < 0) | (xi > W - 1)
    yi, xi = np.where(outside, 0.0, yi), np.where(outside, 0.0, xi)
    fy, fx = np.floor(yi), np.floor(xi)
    wy, wx = _weights(yi - fy), _weights(xi - fx)
    iy = [_mirror(fy.astype(np.int64) + k - 1, H) for k in range(4)]
    ix = [_mirror(fx.astype(np.int64) + k - 1, W) for k in range(4)]
    out = np.zeros(coeff.shape, dtype=np.float64)
    for j in range(4):
        for k in range(4):
            out = out + coeff[iy[j], ix[k]] * wy[j][:, :, None] * wx[k][:, :, None]
    return out, outside


def cast_u8(v):
    """float64 -> uint8 as the reference's astype(np.uint8) does on x86-64: truncate toward zero, then modulo 256."""
    return (np.asarray(v).astype(np.int64) & 255).astype(np.uint8)


def matrix(H, W, angle, v_shift, h_shift, sx, sy):
    """The reference's 3 x 3 matrix (utils/image.py:131-148): output (y, x, 1) -> input (y, x, 1), about the centre (H/2 + .5, W/2 + .5)."""
    mat = np.array([[sy * np.cos(angle), -sy * np.sin(angle), v_shift],
                    [sx * np.sin(angle), sx * np.cos(angle), h_shift],
                    [0., 0., 1.]])
    off = (H / 2.0 + 0.5, W / 2.0 + 0.5)
    return np.dot(np.dot(np.array([[1., 0., off[0]], [0., 1., off[1]], [0., 0., 1.]]), mat),
                  np.array([[1., 0., -off[0]], [0., 1., -off[1]], [0., 0., 1.]]))


def mat6(m):
    """3 x 3 matrix -> the (m00, m01, t0, m10, m11, t1) row isx_affine_noisy_u8 takes."""
    return np.array([m[0, 0], m[0, 1], m[0, 2], m[1, 0], m[1, 1], m[1, 2]], dtype=np.float64)


def affine_cv(img, angle, v_shift, h_shift, sx, sy, cval=0.):
    """The reference's affine_cv: the warped image as float64, `cval` where the warp leaves the input."""
    img = np.asarray(img)
    v, outside = warp(spline_coefficients(img), mat6(matrix(img.shape[0], img.shape[1], angle, v_shift, h_shift, sx, sy)))
    v[outside] = cval
    return v


def affine_noisy(img_u8, m6, seed, noise_id):
    """One image through prefilter, warp, cast and noise fill: the host twin of isx_affine_noisy_u8."""
    img_u8 = np.asarray(img_u8)
    v, outside = warp(spline_coefficients(img_u8), m6)
    out = cast_u8(v)
    out[outside] = noise_bytes(seed, noise_id, img_u8.shape[0], img_u8.shape[1])[outside]
    return out


def _key_hash(keys, lanes):
    """(lanes, B) uint64: a hash per lane number and row of an int64 key array (B,K) -- chained splitmix64 over the key's columns, then one
    more round per lane."""
    keys = np.atleast_2d(np.asarray(keys, dtype=np.int64)).astype(np.uint64)
    h = np.full(keys.shape[0], 0x243F6A8885A308D3, dtype=np.uint64)
    with np.errstate(over='ignore'):
        for k in range(keys.shape[1]):
            h = _mix64(h + _GOLDEN + keys[:, k])
        return _mix64(h[None, :] + _GOLDEN * np.arange(1, lanes + 1, dtype=np.uint64)[:, None])


class RandomAffineNoisy(object):
    """What random_affine_noisy_cv returns.  Called on a host image it behaves as the reference's closure (parameters from np.random / random,
    in the reference's order); the training mains use `plan` instead, which derives parameters and noise ids from keys, not from a stream."""

    def __init__(self, rotation=0, h_range=0, v_range=0, hs_range=0, vs_range=0, h_flip=False):
        self.rotation = rotation * (np.pi / 180)
        self.h_range, self.v_range, self.hs_range, self.vs_range, self.h_flip = h_range, v_range, hs_range, vs_range, bool(h_flip)

    matrix = staticmethod(matrix)

    def draw(self, rng_np=np.random, rng_py=random, shape=None):
        """(angle, v_shift, h_shift, sx, sy) drawn in the reference's order (utils/image.py:176-183); the shifts are fractions of the image
        size unless `shape` = (H, W, ...) is given."""
        angle = rng_np.uniform(-self.rotation, self.rotation)
        v = rng_np.uniform(-self.v_range, self.v_range)
        h = rng_np.uniform(-self.h_range, self.h_range)
        sx = 1 + rng_py.uniform(-self.hs_range, self.hs_range)
        sy = 1 + rng_py.uniform(-self.vs_range, self.vs_range)
        if self.h_flip and rng_py.random() < 0.5:
            sx = -sx
        if shape is not None:
            v, h = v * shape[0], h * shape[1]
        return angle, v, h, sx, sy

    def plan(self, keys, H, W):
        """keys: (B,K) integers, one row per image (seed, epoch, item index, role ...).  Returns (mats (B,6) float64, noise_ids (B,) int64): the
        same five uniforms and flip as `draw`, each a function of the image's key alone -- so a batch is the same whatever slice of it a
        data-parallel rank builds."""
        hashed = _key_hash(keys, 7)
        unit = (hashed >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)         # 53 bits -> [0, 1)

        def u(lane, lo, hi):
            return lo + (hi - lo) * unit[lane]
        angle = u(0, -self.rotation, self.rotation)
        v = u(1, -self.v_range, self.v_range) * H
        h = u(2, -self.h_range, self.h_range) * W
        sx = 1 + u(3, -self.hs_range, self.hs_range)
        sy = 1 + u(4, -self.vs_range, self.vs_range)
        if self.h_flip:
            sx = np.where(u(5, 0.0, 1.0) < 0.5, -sx, sx)
        # the reference's np.dot chain (matrix above), written out per element in its order of operations: T(o) . M . T(-o)
        o0, o1 = H / 2.0 + 0.5, W / 2.0 + 0.5
        m00, m01, m10, m11 = sy * np.cos(angle), -sy * np.sin(angle), sx * np.sin(angle), sx * np.cos(angle)
        t0 = m00 * -o0 + m01 * -o1 + (v + o0)
        t1 = m10 * -o0 + m11 * -o1 + (h + o1)
        mats = np.stack([m00, m01, t0, m10, m11, t1], 1)
        return mats, (hashed[6] >> np.uint64(1)).astype(np.int64)

    def __call__(self, img):
        img = np.asarray(img)
        m6 = mat6(matrix(img.shape[0], img.shape[1], *self.draw(shape=img.shape)))
        return affine_noisy(img, m6, int(np.random.randint(0, 2 ** 31 - 1)), 0)


def random_affine_noisy_cv(rotation=0, h_range=0, v_range=0, hs_range=0, vs_range=0, h_flip=False):
    return RandomAffineNoisy(rotation, h_range, v_range, hs_range, vs_range, h_flip)
