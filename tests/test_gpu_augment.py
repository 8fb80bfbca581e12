"""isx_affine_noisy_u8 (csrc/augment.hip) through the C ABI with buffers the test owns (tests/_guards.py: poisoned outputs between sentinel
guards, operands between guards), against the reference's own output for the inputs of tests/_augment_cases.py (recorded there as digests
of its outside masks and of its uint8 values at every covered pixel) and the numpy model (tests/_augment_model.py, pinned to the reference on
the CPU by tests/test_augment_model.py); then one augmented optimizer step of
train.siamese_descriptor on the engine route."""
import copy
import functools
import os
import random

import numpy as np
import pytest
import torch

import _augment_cases as C
import _augment_model as M
import _guards as G

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SEED = 0x1234567890ABCDEF


@functools.lru_cache(maxsize=None)
def fixture():
    """The test inputs: img<s>, params<s>, and mat<s> = the reference's matrix chain for those parameters (digest-checked in the parity test)."""
    d = dict(C.make_inputs())
    for s in range(len(C.SHAPES)):
        H, W = d["img%d" % s].shape[1:3]
        d["mat%d" % s] = np.stack([M.matrix6(H, W, *p) for p in d["params%d" % s]])
    return d


def noise_ids(n, salt=0):
    return (np.arange(n, dtype=np.int64) * 1000003 + 12345678901 + salt) % (1 << 62)


@functools.lru_cache(maxsize=None)
def model_case(s):
    """The model's output for every image of fixture shape s (seed and noise ids as `run` passes them): (uint8, outside mask), computed once."""
    fx = fixture()
    ids = noise_ids(len(fx["img%d" % s]))
    res = [M.affine_noisy(fx["img%d" % s][i], fx["mat%d" % s][i], SEED, ids[i]) for i in range(len(ids))]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


def _lib():
    from isx._lib import lib
    return lib(), torch.cuda.current_stream().cuda_stream


def run(imgs, rows, mats, seed, ids, cl=True, want_u8=True, want_f32=True, mean=MEAN, std=STD, ws_short=0, expect=0):
    """One guarded call.  Returns (out_u8 host or None, out_f32 host or None, the out_u8 Region)."""
    L, st = _lib()
    imgs = np.ascontiguousarray(imgs, np.uint8)
    N, H, W, _ = imgs.shape
    B = len(mats)
    gi = G.Region("u8", imgs.shape, 4096, data=imgs)
    gm = G.Region("f64", (B, 6), 64, data=np.ascontiguousarray(mats, np.float64))
    gid = G.in_i64(ids, 64)
    gr = G.in_i64(rows, 64) if rows is not None else None
    gmean, gstd = (G.in_f32(np.array(mean, np.float32), 64) if mean is not None else None), (G.in_f32(np.array(std, np.float32), 64) if std is not None else None)
    ou = G.Region("u8", (B, H, W, 3), 4096) if want_u8 else None
    of = G.out_f32((B, H, W, 3) if cl else (B, 3, H, W), 4096) if want_f32 else None
    need = L.isx_affine_noisy_workspace(B, H, W)
    assert need >= B * H * W * 24 and need % 256 == 0
    ws = G.workspace(need - ws_short)
    rc = L.isx_affine_noisy_u8(gi.ptr, G.ptr(gr), B, H, W, gm.ptr, seed, gid.ptr, G.ptr(gmean), G.ptr(gstd), int(cl), G.ptr(ou), G.ptr(of), ws.ptr,
                               need - ws_short, st)
    assert rc == expect, (rc, L.isx_last_error())
    torch.cuda.synchronize()
    ins = [gi, gm, gid, gr, gmean, gstd]
    if expect != 0:
        assert all(r is None or r.guards_intact() for r in ins + [ou, of, ws])
        assert all(r is None or r.unwritten() == r.n for r in (ou, of))            # a refused call launches nothing
        return None, None, ou
    G.assert_clean([of] if of is not None else [], ins, (B, H, W, cl))
    assert ws.guards_intact()
    if ou is not None:
        # a byte output may legitimately hold the poison value: the call is repeated into a body poisoned with another byte, and an element
        # counts as never written only if it shows the poison of BOTH bodies
        ou2 = G.Region("u8", (B, H, W, 3), 4096)
        ou2.raw().fill_(0x32)
        assert L.isx_affine_noisy_u8(gi.ptr, G.ptr(gr), B, H, W, gm.ptr, seed, gid.ptr, G.ptr(gmean), G.ptr(gstd), int(cl), ou2.ptr, None, ws.ptr, need, st) == 0
        torch.cuda.synchronize()
        assert ou.guards_intact() and ou2.guards_intact() and ws.guards_intact(), ("store outside out_u8", (B, H, W))
        left = int(((ou.raw() == ou.poison) & (ou2.raw() == 0x32)).sum())
        assert left == 0, ("out_u8: %d of %d bytes never written" % (left, ou.n), (B, H, W))
        assert torch.equal(ou.raw()[ou2.raw() != 0x32], ou2.raw()[ou2.raw() != 0x32])
    return (ou.host() if ou is not None else None), (of.host() if of is not None else None), ou


@pytest.mark.parametrize("s", [0, 1, 2])
def test_uint8_parity_with_the_reference(s):
    """out_u8 equals the reference's uint8 wherever the warp covers the input, at (5,24,20), (3,37,53) -- H W no multiple of 4, a ragged last
    block -- and (1,224,224); the outside pixels, read off where the output carries the model's noise bytes, are exactly the reference's.
    The rule allows one step of the wrap where the reference's float64 value lies within 1e-9 of an integer (at most 1e-4 of the inside
    pixels); these inputs have no such value (tests/test_augment_model.py counts them against the reference), so ZERO mismatches are asserted
    -- which is what equal digests say.  The byte-for-byte comparison with the model names the pixels if a digest ever differs."""
    fx = fixture()
    imgs, mats = fx["img%d" % s], fx["mat%d" % s]
    assert C.digest_arrays([mats]) == C.REFERENCE["mat%d" % s]
    ids = noise_ids(len(imgs))
    got, _, _ = run(imgs, None, mats, SEED, ids, want_f32=False)
    model_u8, model_out = model_case(s)
    masks = [(got[i] == M.noise(SEED, ids[i], imgs.shape[1], imgs.shape[2])).all(-1) for i in range(len(imgs))]
    bad = [int((got[i] != model_u8[i])[~model_out[i]].sum()) for i in range(len(imgs))]
    print("shape %d: outside pixels per image %s (reference %s); inside bytes that differ from the model %s"
          % (s, [int(m.sum()) for m in masks], C.REFERENCE["outside_count%d" % s], bad))
    assert [int(m.sum()) for m in masks] == C.REFERENCE["outside_count%d" % s]
    assert C.digest_masks(masks) == C.REFERENCE["outside%d" % s]
    assert C.digest_inside(got, masks) == C.REFERENCE["inside_u8_%d" % s]
    assert np.array_equal(got, model_u8)                                    # noise bytes included: the generator of include/isx.h bit for bit


def test_noise_is_a_function_of_seed_id_and_position():
    fx = fixture()
    imgs, mats = fx["img0"], fx["mat0"]
    ids = noise_ids(5)
    alone, _, _ = run(imgs, np.array([3]), mats[3:4], SEED, ids[3:4], want_f32=False)
    rows = np.array([1, 4, 0, 3, 2])
    batch, _, _ = run(imgs, rows, mats[rows], SEED, ids[rows], want_f32=False)
    assert np.array_equal(batch[3], alone[0])                               # B = 1 and row 3 of B = 5: the same bytes
    assert np.array_equal(batch, model_case(0)[0][rows])
    other, _, _ = run(imgs, np.array([3]), mats[3:4], SEED + 1, ids[3:4], want_f32=False)
    out3 = model_case(0)[1][3]
    assert np.array_equal(other[0][~out3], alone[0][~out3]) and not np.array_equal(other[0][out3], alone[0][out3])
    # 256 bins over the outside bytes of the 224 x 224 case: 255 degrees of freedom, mean 255, sigma sqrt(510); bound 255 + 5 sigma = 368.
    # The model passes it first (and is compared with the kernel byte for byte above and here)
    got, _, _ = run(fx["img2"], None, fx["mat2"], SEED, noise_ids(1), want_f32=False)
    out = model_case(2)[1][0]
    n_out = int(out.sum()) * 3
    assert n_out > 20000
    assert M.chi_square_256(model_case(2)[0][0][out]) < 368.0
    chi = M.chi_square_256(got[0][out])
    print("chi-square of %d outside bytes: %.1f" % (n_out, chi))
    assert chi < 368.0


@pytest.mark.parametrize("cl", [True, False])
@pytest.mark.parametrize("s", [0, 1])
def test_f32_output_is_images_u8_to_f32_of_the_u8_output(s, cl):
    L, st = _lib()
    fx = fixture()
    imgs, mats = fx["img%d" % s], fx["mat%d" % s]
    B, H, W, _ = imgs.shape
    u8, f32, region = run(imgs, None, mats, SEED, noise_ids(B), cl=cl)
    want = G.out_f32(f32.shape, 4096)
    assert L.isx_images_u8_to_f32(region.ptr, B, H, W, *MEAN, *STD, int(cl), want.ptr, st) == 0
    G.assert_clean([want])
    G.assert_bits(f32, want.host(), (s, cl))
    G.assert_bits(f32, M.normalise(u8, MEAN, STD, cl), (s, cl, "model"))
    # the float output alone (no out_u8), and without mean / std (0 and 1)
    _, only, _ = run(imgs, None, mats, SEED, noise_ids(B), cl=cl, want_u8=False)
    G.assert_bits(only, f32)
    _, raw, _ = run(imgs, None, mats, SEED, noise_ids(B), cl=cl, mean=None, std=None)
    G.assert_bits(raw, M.normalise(u8, (0, 0, 0), (1, 1, 1), cl))


def test_rows_select_images_of_the_resident_set():
    rng = np.random.RandomState(7)
    imgs = rng.randint(0, 256, (7, 13, 11, 3)).astype(np.uint8)
    fx = fixture()
    rows = np.array([5, 0, 6, 2, 2, 4, 1, 3])
    mats = np.concatenate([fx["mat0"], fx["mat1"]])[:8].copy()
    mats[:, 2] *= 13 / 24.0
    mats[:, 5] *= 11 / 20.0
    ids = noise_ids(8, salt=5)
    a, fa, _ = run(imgs, rows, mats, 99, ids)
    b, fb, _ = run(imgs[rows], None, mats, 99, ids)
    assert np.array_equal(a, b)
    G.assert_bits(fa, fb)
    want = np.stack([M.affine_noisy(imgs[r], mats[i], 99, ids[i])[0] for i, r in enumerate(rows)])
    assert np.array_equal(a, want)


def test_edge_matrices_and_shapes():
    fx = fixture()
    imgs = fx["img1"]                                                        # 37 x 53: H W not a multiple of 4
    B, H, W, _ = imgs.shape
    ident = np.tile(np.array([1., 0., 0., 0., 1., 0.]), (B, 1))
    got, _, _ = run(imgs, None, ident, SEED, noise_ids(B), want_f32=False)
    # interpolating the spline at the grid points returns the samples up to rounding: the values sit ON integers, so the cast may land one below
    assert int(np.abs(got.astype(np.int64) - imgs.astype(np.int64)).max()) <= 1
    away = np.tile(np.array([1., 0., -1000., 0., 1., 0.]), (B, 1))
    got, _, _ = run(imgs, None, away, SEED, noise_ids(B), want_f32=False)
    assert np.array_equal(got, np.stack([M.noise(SEED, i, H, W) for i in noise_ids(B)]))
    nan = away.copy()
    nan[:, 2] = np.nan
    got_nan, _, _ = run(imgs, None, nan, SEED, noise_ids(B), want_f32=False)
    assert np.array_equal(got_nan, got)                                      # a NaN coordinate is outside
    # lines of length 1 and 2, a single pixel, a one-row image
    rng = np.random.RandomState(3)
    for shape in ((2, 1, 1), (2, 1, 9), (2, 9, 1), (2, 2, 2), (1, 3, 70)):
        im = rng.randint(0, 256, shape + (3,)).astype(np.uint8)
        m = np.tile(np.array([.9, .1, .05, -.1, .95, .1]), (shape[0], 1))
        got, _, _ = run(im, None, m, 5, noise_ids(shape[0]), want_f32=False)
        want = np.stack([M.affine_noisy(im[i], m[i], 5, noise_ids(shape[0])[i])[0] for i in range(shape[0])])
        assert np.array_equal(got, want), shape


def test_short_workspace_is_refused():
    fx = fixture()
    L, _ = _lib()
    run(fx["img0"], None, fx["mat0"], SEED, noise_ids(5), ws_short=256, expect=-2)
    assert b"workspace too small" in L.isx_last_error()


def test_ops_affine_noisy_chunks_by_workspace_budget():
    from isx import ops
    fx = fixture()
    imgs, mats = fx["img0"], fx["mat0"]
    ids = noise_ids(5)
    x = torch.from_numpy(imgs).cuda()
    whole, u8 = ops.affine_noisy(x, None, mats, SEED, ids, MEAN, STD, channels_last=True, want_u8=True)
    assert whole.is_contiguous(memory_format=torch.channels_last) and np.array_equal(u8.cpu().numpy(), model_case(0)[0])
    old = ops.AFFINE_WORKSPACE_BUDGET
    try:
        ops.AFFINE_WORKSPACE_BUDGET = 2 * 24 * 20 * 24 + 512                # two images per launch: chunks of 2, 2, 1
        rows = torch.tensor([4, 3, 2, 1, 0])
        parts, u8p = ops.affine_noisy(x, rows, mats[::-1].copy(), SEED, ids[::-1].copy(), MEAN, STD, channels_last=False, want_u8=True)
    finally:
        ops.AFFINE_WORKSPACE_BUDGET = old
    assert np.array_equal(u8p.cpu().numpy(), model_case(0)[0][::-1])
    assert torch.equal(parts.flip(0), whole.contiguous())


def _one_augmented_step(calls):
    import model.siamese as ms
    from train import _common as TC
    from train import siamese_descriptor as sd
    from isx import ops
    from utils.image import random_affine_noisy_cv
    saved, saved_raw = copy.copy(sd.P.__dict__), dict(TC.RAW_INGEST)
    g = torch.Generator().manual_seed(11)
    pat = torch.randint(0, 256, (4, 64, 64, 3), generator=g)
    tr = [(((pat[i % 4] + torch.randint(0, 256, (64, 64, 3), generator=g)) // 2).to(torch.uint8), "c%d" % (i % 4), "tr%d" % i) for i in range(16)]
    te = [(((pat[i % 4] + torch.randint(0, 256, (64, 64, 3), generator=g)) // 2).to(torch.uint8), "c%d" % (i % 4), "te%d" % i) for i in range(8)]
    real = ops.affine_noisy
    try:
        ops.affine_noisy = lambda img, rows, mats, *a, **k: (calls.append((tuple(img.shape), None if rows is None else int(rows.numel()), len(mats))) or real(img, rows, mats, *a, **k))
        TC.RAW_INGEST["mean"], TC.RAW_INGEST["std"] = list(MEAN), list(STD)
        TC.drop_resident()
        P = sd.P
        P.cuda_device, P.cnn_model, P.feature_size2d, P.feature_dim = 0, "resnet50", (2, 2), 32
        P.train_epochs, P.train_batch_size, P.train_micro_batch, P.test_batch_size = 1, 40, 8, 16
        P.train_loss_int, P.train_epoch_switch, P.train_lr, P.train_seed = 1000, 1, 1e-3, 7
        P.untrained_blocks = None
        P.train_pre_proc, P.train_trans = False, random_affine_noisy_cv(rotation=45, hs_range=.25, vs_range=.25, h_flip=True)
        torch.manual_seed(0); random.seed(0)
        init = {k: v.detach().clone() for k, v in sd.get_siamese_net().state_dict().items()}
        torch.manual_seed(0); random.seed(0)
        net, _ = sd.main(tr, tr, te)
        assert ms.SPLIT_TRUNK and ms.SUFFIX_ENGINE and net.trunk_precomputable() and net.suffix_engine() is not None      # the engine route
        return init, {k: v.detach().clone() for k, v in net.state_dict().items()}
    finally:
        ops.affine_noisy = real
        TC.drop_resident()
        TC.RAW_INGEST.update(saved_raw)
        sd.P.__dict__.clear(); sd.P.__dict__.update(saved)


def test_one_augmented_training_step_on_the_engine_route():
    """ResNet-50 (stem + layers 1-3 frozen, layer4 + head trained), 16 raw 64 x 64 images, one mini-batch of 40 triplets: the three branches'
    batches come from ONE isx_affine_noisy_u8 call that reads the resident uint8 set through its row numbers; the step moves layer4 and the
    head; repeated with the same seed it ends on the same weights, bit for bit."""
    calls = []
    init, a = _one_augmented_step(calls)
    assert calls == [((16, 64, 64, 3), 120, 120)], calls
    _, b = _one_augmented_step([])
    moved = 0.0
    for k in a:
        assert torch.equal(a[k], b[k]), k
        if a[k].dtype.is_floating_point:
            moved = max(moved, float((a[k] - init[k].to(a[k].device)).abs().max()))
    assert moved > 0
