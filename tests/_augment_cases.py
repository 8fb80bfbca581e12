"""The inputs of the augmentation tests and what the reference made of them.

make_inputs() rebuilds the test images and warp parameters from a seed (numpy's legacy RandomState: the same stream on every version); nothing
of the reference is stored as a file.  REFERENCE holds what the reference's own utils/image.py (scipy.ndimage.affine_transform underneath)
produced for them, as recorded by tools/gen_augment_golden.py: SHA-256 digests of its matrices, of its outside masks and of its uint8 output
at the pixels the warp covers, plus the five parameters of one seeded call of its random closure.  A digest is compared for equality -- the
uint8 comparison of the tests allows no mismatch on these inputs.  tests/test_augment_model.py recomputes the whole table from the reference
where the reference tree is present, and there also compares float64 values (within 1e-10), which no digest can carry."""
import hashlib

import numpy as np

SEED = 20261019
SHAPES = ((5, 24, 20), (3, 37, 53), (1, 224, 224))


def make_inputs():
    """{'img<s>': (n,H,W,3) uint8, 'params<s>': (n,5) float64 = angle, v_shift, h_shift, sx, sy} for the three shapes."""
    rs = np.random.RandomState(SEED)
    out = {}
    for s, (n, H, W) in enumerate(SHAPES):
        out["img%d" % s] = rs.randint(0, 256, size=(n, H, W, 3)).astype(np.uint8)
        params = np.zeros((n, 5))
        for i in range(n):
            angle = rs.uniform(-np.pi / 4, np.pi / 4)
            sx, sy = 1 + rs.uniform(-.25, .25), 1 + rs.uniform(-.25, .25)
            v, h = rs.uniform(-.1, .1) * H, rs.uniform(-.1, .1) * W
            params[i] = (angle, v, h, -sx if i % 2 else sx, sy)
        out["params%d" % s] = params
    return out


def digest_arrays(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def digest_masks(masks):
    """Outside masks (n,H,W) bool -> digest of their packed bits, image by image."""
    return digest_arrays([np.packbits(np.asarray(m, bool)) for m in masks])


def digest_inside(u8, masks):
    """uint8 images (n,H,W,3) -> digest of the bytes at the pixels the warp covers (outside mask False), image by image in raster order."""
    return digest_arrays([np.asarray(u)[~np.asarray(m, bool)] for u, m in zip(u8, masks)])


def table(mats, outside, u8, draw_params, draw_outside, draw_u8):
    """The REFERENCE table of a set of results (lists indexed by shape)."""
    t = {}
    for s in range(len(SHAPES)):
        t["mat%d" % s] = digest_arrays([np.asarray(mats[s], np.float64)])
        t["outside%d" % s] = digest_masks(outside[s])
        t["inside_u8_%d" % s] = digest_inside(u8[s], outside[s])
        t["outside_count%d" % s] = [int(np.asarray(m).sum()) for m in outside[s]]
    t["draw_params"] = [float(v).hex() for v in draw_params]
    t["draw_outside"] = digest_masks([draw_outside])
    t["draw_inside_u8"] = digest_inside([draw_u8], [draw_outside])
    return t


REFERENCE = {'draw_inside_u8': 'f260b52a5d7b0ced8f3c976fbfb0c629e8ab94def37617afa41d9320cbe1ba3d',
 'draw_outside': 'e9159970b9d37176f501e7e73cbfb93768635455663a7a91676c4436b1c7ae0d',
 'draw_params': ['0x1.50283be8fa528p-2', '0x1.1ef65bee72e02p+1', '-0x1.4be46278e6229p-1', '0x1.0b60ca5529ed2p+0', '0x1.3b646c9b92f5ep+0'],
 'inside_u8_0': 'a9c424664cd43854dda2b40d0161ea2ddfd2d7c74b8ff145c53bec9b3043911b',
 'inside_u8_1': 'c75f48115b9c31f2571bd153ff33094b609464acb79196f071fc23dff184c104',
 'inside_u8_2': 'd3ba6f1ce2ae6b1ed89f07d69452561d4c0396b43d158189fee6d6c6dff6e671',
 'mat0': '7037988d439281fc70a604cadae4b1983ffa52e93f01f20a7828df1c4262c64c',
 'mat1': '3cdf6849851988c576d53aaf13ae23d23189995b6f6804ff7b43875af4e0369f',
 'mat2': 'fa5dfaac52cbfa2486ae895c5a8a3cdbf221a7bff480b00c45f8d316a48ff0f5',
 'outside0': '7a6a2e86581f94ff9b225e89ba1b6d600eec634f588625823604ed2ad5665eb2',
 'outside1': '53447c9e425bd69c864245778b383acbd260668d1b723c093046250cdda407c0',
 'outside2': '0d1240549801767803e92aa043841ee8d9aab0a9bc66772f3a4baee9ef0ff742',
 'outside_count0': [69, 84, 139, 135, 47],
 'outside_count1': [197, 218, 171],
 'outside_count2': [10772]}
