"""Independent model of the dataset statistics (isx/prep.py, csrc/prep.hip) for tests/test_mean_std_model.py and tests/test_gpu_prep.py.

The two conventions are the two branches of the reference's create_mean_std_file.py:25-46, restated in float64 numpy (the script itself cannot
be imported: it runs at import, on hard-coded paths, through cv2): pooled() is the branch with a constant image size, per_image() the one
without.  moments() is what the kernel is compared with bit for bit, and KERNEL_CASES the shapes at which it can go wrong."""
import numpy as np


def moments(img):
    """(B,H,W,3) uint8 -> (B,3,2) int64: per image and channel the sum and the sum of squares."""
    v = np.asarray(img).astype(np.int64).reshape(img.shape[0], -1, 3)
    return np.stack([v.sum(axis=1), (v * v).sum(axis=1)], axis=2)


def pooled(images):
    """Mean and unbiased standard deviation of v / 255 over all values of a channel (the pixels of every image in one column: for images of one
    shape, the reference's stacked tensor)."""
    t = np.concatenate([np.asarray(im).reshape(-1, 3) for im in images]).astype(np.float64) / 255.0
    cols = [np.ascontiguousarray(t[:, c]) for c in range(3)]          # contiguous: numpy's pairwise sum
    return [float(np.mean(v)) for v in cols], [float(np.std(v, ddof=1)) for v in cols]


def per_image(images):
    """Images of any shapes, two passes: the mean of the images' means, then the root of the mean over images of each image's mean squared
    deviation from it."""
    count = len(images)
    scaled = [np.asarray(im).astype(np.float64) / 255.0 for im in images]
    mean = [0.0, 0.0, 0.0]
    for s in scaled:
        area = s.shape[0] * s.shape[1]
        for c in range(3):
            mean[c] += np.sum(s[:, :, c]) / (area * count)
    var = [0.0, 0.0, 0.0]
    for s in scaled:
        area = s.shape[0] * s.shape[1]
        for c in range(3):
            var[c] += np.sum(np.square(s[:, :, c] - mean[c])) / (area * count)
    return [float(m) for m in mean], [float(np.sqrt(v)) for v in var]


def random_images(rng, n, h, w):
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(n)]


def ragged_images(rng, n=9, lo=5, hi=40):
    return [rng.integers(0, 256, (int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1)), 3), dtype=np.uint8) for _ in range(n)]


# (id, (B, H, W), byte offset of the image region past a 256-byte boundary, fill: "random", "ones" (all 255) or "mixed" (image 0 all 255))
KERNEL_CASES = [
    ("1x1x1", (1, 1, 1), 0, "random"),
    ("1x1x5_under_one_load", (1, 1, 5), 0, "random"),                 # 15 bytes
    ("1x1x6", (1, 1, 6), 0, "random"),                                # 18 bytes
    ("3x5x7_misaligned_images", (3, 5, 7), 0, "random"),              # 105 bytes per image: images 1 and 2 start off every boundary, another phase each
    ("2x16x16_whole_groups", (2, 16, 16), 0, "random"),               # 768 bytes = 16 x 48
    ("1x37x53", (1, 37, 53), 0, "random"),
    ("4x64x64_off0", (4, 64, 64), 0, "random"),
    ("4x64x64_off1", (4, 64, 64), 1, "random"),
    ("4x64x64_off2", (4, 64, 64), 2, "random"),
    ("4x64x64_off3", (4, 64, 64), 3, "random"),
    ("4x64x64_off13", (4, 64, 64), 13, "random"),
    ("2x224x224_workload", (2, 224, 224), 0, "mixed"),
    ("1x258x257_past_2^32", (1, 258, 257), 0, "ones"),                # sum of squares 4 311 547 650 > 2^32
]


def kernel_image(cid):
    """The image of a case: seeded by its position in KERNEL_CASES."""
    k = [c[0] for c in KERNEL_CASES].index(cid)
    _, (B, H, W), _, fill = KERNEL_CASES[k]
    if fill == "ones":
        return np.full((B, H, W, 3), 255, np.uint8)
    img = np.random.default_rng([2024, k]).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    if fill == "mixed":
        img[0] = 255
    return img
