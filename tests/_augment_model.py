"""numpy-only model of isx_affine_noisy_u8 (csrc/augment.hip): cubic B-spline prefilter, affine warp, wrap-around uint8 cast and counter-based
noise fill, float64 with one rounding per operation.  Imports nothing from the library: tests/test_augment_model.py pins it to the reference's
own output (tests/golden/augment.npz, tools/gen_augment_golden.py), tests/test_gpu_augment.py pins the kernels to it."""
import numpy as np

Z = np.sqrt(3.0) - 2.0
GOLDEN = 0x9E3779B97F4A7C15
U64 = np.uint64


def mix64(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def noise(seed, noise_id, H, W):
    """(H,W,3) uint8: the byte of (y, x, c) is the top byte of mix64(seed + GOLDEN * (noise_id * 3HW + 3 (y W + x) + c)) modulo 2**64."""
    with np.errstate(over="ignore"):
        counter = U64(int(noise_id) % 2 ** 64) * U64(3 * H * W) + np.arange(3 * H * W, dtype=U64)
        return (mix64(U64(int(seed) % 2 ** 64) + U64(GOLDEN) * counter) >> U64(56)).astype(np.uint8).reshape(H, W, 3)


def filter_axis0(c):
    """Lines along axis 0 of a float64 array, in place."""
    n = len(c)
    if n == 1:
        return
    c *= (1.0 - Z) * (1.0 - 1.0 / Z)
    zn = 1.0
    for _ in range(n - 1):
        zn = zn * Z
    acc, zi, i = c[0] + zn * c[n - 1], Z, 1
    while i <= n - 2 and abs(zi) >= 1e-30:
        acc = acc + zi * (c[i] + zn * c[n - 1 - i])
        zi, i = zi * Z, i + 1
    c[0] = acc / (1.0 - zn * zn)
    for i in range(1, n):
        c[i] = c[i] + Z * c[i - 1]
    c[n - 1] = (Z * c[n - 2] + c[n - 1]) * (Z / (Z * Z - 1.0))
    for i in range(n - 2, -1, -1):
        c[i] = Z * (c[i + 1] - c[i])


def prefilter(img):
    c = np.array(img, dtype=np.float64)          # (H,W,3)
    filter_axis0(c)
    filter_axis0(np.swapaxes(c, 0, 1))
    return c


def mirror(i, n):
    if n == 1:
        return i * 0
    p = 2 * (n - 1)
    i = i % p
    return np.where(i >= n, p - i, i)


def weights(t):
    u = 1.0 - t
    w0 = u * u * u / 6.0
    w1 = (t * t * (t - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0
    return w0, w1, w2, 1.0 - w0 - w1 - w2


def warp_f64(img, m):
    """img (H,W,3), m = (m00, m01, t0, m10, m11, t1) -> (float64 values (H,W,3), outside mask (H,W))."""
    H, W = img.shape[:2]
    c = prefilter(img)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    yi = m[2] + m[0] * y + m[1] * x
    xi = m[5] + m[3] * y + m[4] * x
    out = (yi < 0) | (yi > H - 1) | (xi < 0) | (xi > W - 1)
    yi[out] = 0.0
    xi[out] = 0.0
    fy, fx = np.floor(yi), np.floor(xi)
    wy, wx = weights(yi - fy), weights(xi - fx)
    fy, fx = fy.astype(np.int64), fx.astype(np.int64)
    v = np.zeros((H, W, 3))
    for a in range(4):
        ya = mirror(fy + (a - 1), H)
        for b in range(4):
            v = v + c[ya, mirror(fx + (b - 1), W)] * wy[a][..., None] * wx[b][..., None]
    return v, out


def matrix6(H, W, angle, v_shift, h_shift, sx, sy):
    """(m00, m01, t0, m10, m11, t1) of the reference's affine_cv (utils/image.py:131-148): T(o) . M . T(-o) as two np.dot, o = (H/2 + .5, W/2 + .5)."""
    m = np.array([[sy * np.cos(angle), -sy * np.sin(angle), v_shift], [sx * np.sin(angle), sx * np.cos(angle), h_shift], [0., 0., 1.]])
    o = (H / 2.0 + 0.5, W / 2.0 + 0.5)
    m = np.dot(np.dot(np.array([[1., 0., o[0]], [0., 1., o[1]], [0., 0., 1.]]), m), np.array([[1., 0., -o[0]], [0., 1., -o[1]], [0., 0., 1.]]))
    return np.array([m[0, 0], m[0, 1], m[0, 2], m[1, 0], m[1, 1], m[1, 2]])


def cast_u8(v):
    """Truncate toward zero, then modulo 256."""
    return (v.astype(np.int64) & 255).astype(np.uint8)


def affine_noisy(img, m, seed, noise_id):
    """-> (uint8 (H,W,3), outside mask (H,W), float64 values): what isx_affine_noisy_u8 writes to out_u8 for one image."""
    v, out = warp_f64(img, m)
    u8 = cast_u8(v)
    u8[out] = noise(seed, noise_id, img.shape[0], img.shape[1])[out]
    return u8, out, v


def normalise(u8, mean, std, channels_last):
    """out_f32 of the entry: ((float)u8 / 255.0f - mean[c]) / std[c] in fp32; (B,H,W,3) -> (B,3,H,W) memory unless channels_last."""
    f = (u8.astype(np.float32) / np.float32(255.0) - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    return f if channels_last else np.ascontiguousarray(np.moveaxis(f, -1, -3))


def chi_square_256(bytes_):
    """Pearson statistic of a byte sample against the uniform distribution over 256 values (255 degrees of freedom)."""
    n = bytes_.size
    h = np.bincount(bytes_.reshape(-1), minlength=256).astype(np.float64)
    return float(((h - n / 256.0) ** 2 / (n / 256.0)).sum())
