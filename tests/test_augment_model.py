"""Training-time augmentation, CPU side: the numpy model of isx_affine_noisy_u8 (tests/_augment_model.py) and the package's host twin
(utils/image.py) against what the reference's own utils/image.py produced for the inputs of tests/_augment_cases.py -- by digest everywhere
(matrices, outside masks, uint8 at every covered pixel), and value by value (float64 within 1e-10) where the reference tree is present and
tools/gen_augment_golden.py can run it --, the parameter draw order, the documented noise generator, the training mains' acceptance of the
augmenter, the --augment flag, and a data-parallel CPU training run whose weights must not depend on the number of ranks."""
import os
import random
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

import _augment_cases as C
import _augment_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"
N_SHAPES = len(C.SHAPES)


@pytest.fixture(scope="module")
def fx():
    """The test inputs, and the matrices the model builds for their parameters."""
    d = dict(C.make_inputs())
    for s in range(N_SHAPES):
        H, W = d["img%d" % s].shape[1:3]
        d["mat%d" % s] = np.stack([M.matrix6(H, W, *p) for p in d["params%d" % s]])
    return d


@pytest.fixture(scope="module")
def modelled(fx):
    """The model's (float64 values, outside mask) of every input image, computed once."""
    return {(s, i): M.warp_f64(fx["img%d" % s][i], fx["mat%d" % s][i]) for s in range(N_SHAPES) for i in range(len(fx["img%d" % s]))}


@pytest.fixture(scope="module")
def ref():
    """What the reference itself computes for the inputs, run here and now (arrays, tools/gen_augment_golden.generate)."""
    if not os.path.isdir(REFERENCE):
        pytest.skip("the reference tree is not present on this machine")
    pytest.importorskip("scipy")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import warnings
    import gen_augment_golden as gen
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return gen, gen.generate(REFERENCE)


def _per_shape(modelled, s, n):
    return [modelled[(s, i)][0] for i in range(n)], [modelled[(s, i)][1] for i in range(n)]


def test_model_matches_the_reference_digests(fx, modelled):
    """Everywhere, the GPU machine included: the model's matrices, outside masks and uint8 values at every covered pixel ARE the reference's
    (equal digests: not one byte differs)."""
    for s in range(N_SHAPES):
        n = len(fx["img%d" % s])
        vals, outs = _per_shape(modelled, s, n)
        assert C.digest_arrays([fx["mat%d" % s]]) == C.REFERENCE["mat%d" % s], s
        assert [int(o.sum()) for o in outs] == C.REFERENCE["outside_count%d" % s]
        assert C.digest_masks(outs) == C.REFERENCE["outside%d" % s], s
        assert C.digest_inside([M.cast_u8(v) for v in vals], outs) == C.REFERENCE["inside_u8_%d" % s], s
        assert all(0.05 < o.mean() < 0.5 for o in outs)                         # every case has both kinds of pixels


def test_recorded_digests_are_what_the_reference_computes(ref):
    gen, data = ref
    assert gen.digest_table(data) == C.REFERENCE


def test_model_matches_the_reference_values(fx, modelled, ref):
    """float64 within 1e-10 of scipy's at every covered pixel of every shape, masks and uint8 equal; and the condition under which the GPU's
    uint8 comparison may assert zero mismatches: no reference value within 1e-9 of an integer on these inputs."""
    _, data = ref
    worst, overshoot = 0.0, []
    for (s, i), (v, out) in modelled.items():
        ro = data["outside%d" % s][i]
        assert np.array_equal(out, ro) and np.array_equal(fx["mat%d" % s][i], data["mat%d" % s][i]), (s, i)
        r = data["f64_%d" % s][i][~ro]
        worst = max(worst, float(np.abs(v[~ro] - r).max()))
        assert np.array_equal(M.cast_u8(v)[~ro], data["u8_%d" % s][i][~ro]), (s, i)
        assert int((np.abs(r - np.round(r)) < 1e-9).sum()) == 0, (s, i)
        overshoot.append(r.ravel())
    print("model against the reference: max |difference| = %.3g" % worst)
    assert worst <= 1e-10
    overshoot = np.concatenate(overshoot)
    assert ((overshoot < 0) | (overshoot >= 256)).mean() > 0.005               # the wrap of the cast is exercised


def test_cast_wraps_like_the_reference():
    assert M.cast_u8(np.array([-34.37, 273.2, -300.2, 255.99, -0.5])).tolist() == [222, 17, 212, 255, 0]
    from utils import image
    assert image.cast_u8(np.array([-34.37, 273.2, -300.2])).tolist() == [222, 17, 212]


def test_package_affine_cv_and_matrix_match_the_reference(fx, modelled):
    from utils import image
    import utils
    assert utils.random_affine_noisy_cv is image.random_affine_noisy_cv and utils.affine_cv is image.affine_cv
    aug = image.random_affine_noisy_cv()
    for s in range(N_SHAPES - 1):
        got_u8, got_out, mats = [], [], []
        for i in range(len(fx["img%d" % s])):
            img, prm = fx["img%d" % s][i], fx["params%d" % s][i]
            m = aug.matrix(img.shape[0], img.shape[1], *prm)
            assert m.dtype == np.float64 and m.shape == (3, 3)
            mats.append(image.mat6(m))
            got = image.affine_cv(img.astype(float), *prm, cval=.1)
            out = (got == .1).all(-1)
            assert np.array_equal(out, modelled[(s, i)][1])
            assert np.array_equal(got[~out], modelled[(s, i)][0][~out])       # the package and the model are the same arithmetic, bit for bit
            got_u8.append(image.cast_u8(got)), got_out.append(out)
        assert C.digest_arrays([np.stack(mats)]) == C.REFERENCE["mat%d" % s]
        assert C.digest_masks(got_out) == C.REFERENCE["outside%d" % s] and C.digest_inside(got_u8, got_out) == C.REFERENCE["inside_u8_%d" % s]


def test_package_affine_cv_matches_the_reference_values(fx, ref):
    from utils import image
    _, data = ref
    for s in range(N_SHAPES - 1):
        for i in range(len(fx["img%d" % s])):
            got = image.affine_cv(fx["img%d" % s][i].astype(float), *fx["params%d" % s][i], cval=.1)
            assert float(np.abs(got - data["f64_%d" % s][i]).max()) <= 1e-10


def test_draw_follows_the_reference_order(fx):
    from utils import image
    aug = image.random_affine_noisy_cv(rotation=45, hs_range=.25, vs_range=.25, h_flip=True, h_range=.05, v_range=.1)
    img = fx["img0"][0]
    got = aug.draw(np.random.RandomState(C.SEED), random.Random(C.SEED), shape=img.shape)
    assert [float(v).hex() for v in got] == C.REFERENCE["draw_params"]
    # the callable itself, seeded like the reference's call: same parameters, same pixels wherever the warp covers the input
    np.random.seed(C.SEED)
    random.seed(C.SEED)
    out = aug(img)
    _, outside = M.warp_f64(img, M.matrix6(img.shape[0], img.shape[1], *got))
    assert out.dtype == np.uint8 and C.digest_masks([outside]) == C.REFERENCE["draw_outside"]
    assert C.digest_inside([out], [outside]) == C.REFERENCE["draw_inside_u8"]


def test_outside_pixels_carry_the_documented_generator(fx):
    from utils import image
    img, m = fx["img1"][1], fx["mat1"][1]
    H, W = img.shape[:2]
    out = image.affine_noisy(img, m, 77, 123456789)
    ref_v, ro = M.warp_f64(img, m)                                          # (pinned to the reference by the digest tests above)
    # the generator of include/isx.h, scalar form, at a few outside pixels
    def byte(seed, counter):
        z = (seed + 0x9E3779B97F4A7C15 * counter) % 2 ** 64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
        return (z ^ (z >> 31)) >> 56
    for y, x in np.argwhere(ro)[::37]:
        for c in range(3):
            assert out[y, x, c] == byte(77, 123456789 * 3 * H * W + 3 * (int(y) * W + int(x)) + c)
    assert np.array_equal(out[ro], M.noise(77, 123456789, H, W)[ro]) and np.array_equal(out[~ro], M.cast_u8(ref_v)[~ro])
    got, mask, _ = M.affine_noisy(img, m, 77, 123456789)
    assert np.array_equal(got, out) and np.array_equal(mask, ro)
    # another noise id, another seed: other bytes; the same pair: the same bytes
    assert not np.array_equal(M.noise(77, 1, H, W), M.noise(77, 2, H, W)) and not np.array_equal(M.noise(1, 5, H, W), M.noise(2, 5, H, W))


def test_noise_histogram_is_flat():
    """256 bins, 255 degrees of freedom: mean 255, standard deviation sqrt(510) = 22.6; 255 + 5 sigma = 368 is the bound the GPU test uses too."""
    b = M.noise(20261019, 9, 224, 224)
    assert M.chi_square_256(b) < 368.0
    assert M.chi_square_256(b[::2]) < 368.0 and M.chi_square_256(np.zeros(1000, np.uint8)) > 368.0


def test_plan_is_a_function_of_the_keys_alone():
    from train._common import augment_keys
    from utils import image
    aug = image.random_affine_noisy_cv(rotation=45, hs_range=.25, vs_range=.25, h_flip=True)
    keys = augment_keys(5, 1, range(8, 16), 2)
    mats, ids = aug.plan(keys, 24, 20)
    m2, i2 = aug.plan(keys[3:5], 24, 20)
    assert np.array_equal(mats[3:5], m2) and np.array_equal(ids[3:5], i2)     # a slice of the batch draws what the whole batch draws
    assert len(set(ids.tolist())) == 8 and ids.min() >= 0
    # plan writes the reference's matrix chain out per element: the rows are matrices `matrix` builds (rotation within 45 degrees, scales
    # within .25 of 1, no shift: the centre (H/2 + .5, W/2 + .5) maps to itself)
    for m in mats:
        sy, sx = np.hypot(m[0], m[1]), np.hypot(m[3], m[4])
        ang = np.arctan2(-m[1], m[0])
        rebuilt = image.mat6(aug.matrix(24, 20, ang, 0.0, 0.0, sx if m[0] * m[4] - m[1] * m[3] > 0 else -sx, sy))
        assert np.abs(rebuilt - m).max() < 1e-12
    other = aug.plan(augment_keys(5, 1, range(8, 16), 1), 24, 20)[0]
    assert not np.array_equal(other, mats)
    det = mats[:, 0] * mats[:, 4] - mats[:, 1] * mats[:, 3]
    assert (np.abs(det) >= .75 ** 2 - 1e-12).all() and (np.abs(det) <= 1.25 ** 2 + 1e-12).all()
    many = aug.plan(augment_keys(0, 0, range(4000), 0), 8, 8)[0]
    flips = (many[:, 0] * many[:, 4] - many[:, 1] * many[:, 3]) < 0
    assert 0.45 < flips.mean() < 0.55                                       # the flip is a fair coin
    ang = np.arctan2(-many[:, 1], many[:, 0])
    assert ang.min() >= -np.pi / 4 - 1e-9 and ang.max() <= np.pi / 4 + 1e-9 and ang.std() > 0.3


def test_abi_refuses_bad_arguments_without_a_gpu():
    from isx import _lib
    lib = _lib.lib()
    assert lib.isx_affine_noisy_workspace(192, 224, 224) == 192 * 3 * 224 * 224 * 8
    assert lib.isx_affine_noisy_workspace(1, 37, 53) == -(-37 * 53 * 24 // 256) * 256 and lib.isx_affine_noisy_workspace(0, 8, 8) == 0
    assert lib.isx_affine_noisy_workspace(70000, 8, 8) == 0 and lib.isx_affine_noisy_workspace(1, 8, 4000) == 0 and lib.isx_affine_noisy_workspace(1, 40000, 40000) == 0
    a = [4096, None, 2, 8, 8, 8192, 1, 12288, None, None, 1, 16384, 20480, 24576, 1 << 20, None]
    call = lambda *pairs: lib.isx_affine_noisy_u8(*[dict(pairs).get(i, v) for i, v in enumerate(a)])
    assert call((2, 0)) == 0                                                 # B == 0: nothing to do
    assert call((3, 0)) == -1 and b"bad shape" in lib.isx_last_error()
    assert call((2, 70000)) == -1 and b"bad shape" in lib.isx_last_error()
    assert call((4, 4000)) == -1 and b"too wide" in lib.isx_last_error()
    for i in (0, 5, 7, 13):
        assert call((i, None)) == -1 and b"null pointer" in lib.isx_last_error(), i
    assert call((11, None), (12, None)) == -1 and b"null pointer" in lib.isx_last_error()
    assert call((13, 24584)) == -1 and b"16-B aligned" in lib.isx_last_error()
    assert call((12, 20488)) == -1 and b"16-B aligned" in lib.isx_last_error()
    for i in (1, 5, 7):
        assert call((i, 8196)) == -1 and b"8-B aligned" in lib.isx_last_error(), i
    assert call((14, 2 * 8 * 8 * 24 - 1)) == -2 and b"workspace too small" in lib.isx_last_error()


def test_augment_flag_parsing():
    from train import _common as TC
    from train.params import Params
    from utils.image import RandomAffineNoisy
    ref = TC.parse_augment("reference")
    assert isinstance(ref, RandomAffineNoisy) and TC.is_augmenter(ref) and not TC.is_augmenter(None) and not TC.is_augmenter(lambda im: im)
    assert (round(ref.rotation * 180 / np.pi, 9), ref.h_range, ref.v_range, ref.hs_range, ref.vs_range, ref.h_flip) == (45, 0, 0, .25, .25, True)
    got = TC.parse_augment("30,0.1,0.2,0.3,0.4,0")
    assert (round(got.rotation * 180 / np.pi, 9), got.h_range, got.v_range, got.hs_range, got.vs_range, got.h_flip) == (30, .1, .2, .3, .4, False)
    assert TC.parse_augment("off") is None
    for bad in ("1,2,3", "45,0,0,.25,.25,yes", "45,0,0,1.5,.25,1", "-1,0,0,0,0,0", "a,b,c,d,e,1"):
        with pytest.raises(ValueError):
            TC.parse_augment(bad)
    P = Params()
    assert P.train_pre_proc is True and P.train_trans is None               # the default stays off
    assert (P.train_aug_rot, P.train_aug_hrange, P.train_aug_vrange, P.train_aug_hsrange, P.train_aug_vsrange, P.train_aug_hflip) == (45, 0, 0, .25, .25, True)
    seen = []
    TC.training_cli(["--dataset=synthetic:CLICIDE_video_224sq:n=4:q=2:labels=2:size=16", "--device=-1", "--augment=reference"], P,
                    lambda: seen.append((P.train_pre_proc, P.train_trans)), "train.siamese_descriptor")
    assert seen[0][0] is False and isinstance(seen[0][1], RandomAffineNoisy)
    with pytest.raises(SystemExit):
        TC.training_cli(["--dataset=synthetic:x", "--augment=1,2"], Params(), lambda: None, "train.siamese_descriptor")


def test_load_training_sets_accepts_the_augmenter():
    from train import _common as TC
    from train import classif_regions as cr
    from train.params import Params
    from utils.image import random_affine_noisy_cv
    spec = "synthetic:CLICIDE_video_224sq:n=12:q=4:labels=3:size=32"
    P = Params(cuda_device=-1, cnn_model="alexnet", train_pre_proc=False, train_trans=random_affine_noisy_cv(rotation=45, h_flip=True))
    labels = []
    saved = dict(TC.RAW_INGEST)
    try:
        train_set, gallery, queries = TC.load_training_sets(P, spec, labels)
        assert train_set is gallery and len(train_set) == 12 and len(queries) == 4 and len(labels) == 3
        im = train_set[0][0]
        assert im.dtype == torch.uint8 and tuple(im.shape) == (32, 32, 3) and TC.RAW_INGEST["mean"] is not None
        # a batch through the augmenter on the CPU: normalised fp32, no provenance, and a function of the keys
        keys = TC.augment_keys(3, 0, range(4), 0)
        x = TC.stage_images([t[0] for t in train_set[:4]], -1, augment=(P.train_trans, keys, 3))
        assert x.dtype == torch.float32 and tuple(x.shape) == (4, 3, 32, 32) and not hasattr(x, "_isx_rows")
        again = TC.stage_images([t[0] for t in train_set[2:4]], -1, augment=(P.train_trans, keys[2:], 3))
        assert torch.equal(again, x[2:])
        plain = TC.stage_images([t[0] for t in train_set[:4]], -1)
        assert not torch.equal(plain, x)
    finally:
        TC.RAW_INGEST.update(saved)
    # every other transformed configuration is still refused, and so is the augmenter on the sub-region classifier
    for kw in (dict(train_pre_proc=False, train_trans=None), dict(train_pre_proc=True, train_trans=lambda im: im), dict(train_pre_proc=False, train_trans=lambda im: im)):
        with pytest.raises(NotImplementedError):
            TC.load_training_sets(Params(cuda_device=-1, cnn_model="alexnet", **kw), spec, [])
    saved_p = dict(cr.P.__dict__)
    try:
        cr.P.train_pre_proc, cr.P.train_trans, cr.P.cuda_device = False, random_affine_noisy_cv(rotation=45), -1
        with pytest.raises(NotImplementedError, match="resize after the warp"):
            cr.run(spec)
    finally:
        cr.P.__dict__.clear(); cr.P.__dict__.update(saved_p)


class _TinyNet(nn.Module):
    def __init__(self, head_out=8):
        super().__init__()
        from model.custom_modules import RowDeferredLinear
        self.features = nn.Sequential(nn.Conv2d(3, 4, 3, stride=2), nn.BatchNorm2d(4), nn.ReLU())
        self.head = RowDeferredLinear(4 * 3 * 3, head_out)
        self.feature_size = head_out

    def one(self, x):
        y = self.head(self.features(x).flatten(1))
        return y / (y.pow(2).sum(1, keepdim=True) + 1e-10).sqrt()

    def forward(self, a, p=None, n=None):
        return (self.one(a), self.one(p), self.one(n)) if self.training and n is not None else self.one(a)


def _run_augmented_training(rank, world, port, out, augment):
    """The pattern of tests/test_training.py::_run_training, on raw uint8 images with the augmenter as P.train_trans."""
    sys.path.insert(0, os.path.join(ROOT, "instance-search_amd"))
    torch.set_num_threads(1)
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from model.custom_modules import TripletLoss
    from train import _common as TC
    from train import siamese_descriptor as sd
    from utils.image import random_affine_noisy_cv
    import torch.optim as optim
    torch.manual_seed(1000 * rank)
    random.seed(0)
    np.random.seed(rank)                    # the global streams differ per rank: the augmentation must not read them
    net = _TinyNet()
    P = sd.P
    P.cuda_device, P.train_epochs, P.train_batch_size, P.train_micro_batch = -1, 2, 8, 2
    P.train_grad_exchange = "tree"
    P.train_loss_int, P.train_test_int, P.test_batch_size, P.feature_dim, P.train_seed = 1000, 1000, 8, 8, 5
    P.train_epoch_switch, P.train_loss_avg, P.train_bn = 1, False, False
    P.train_pre_proc = not augment
    P.train_trans = random_affine_noisy_cv(rotation=45, hs_range=.25, vs_range=.25, h_flip=True) if augment else None
    TC.RAW_INGEST["mean"], TC.RAW_INGEST["std"] = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    g = torch.Generator().manual_seed(1)
    ds = [(torch.randint(0, 256, (8, 8, 3), generator=g, dtype=torch.uint8), "l%d" % (i % 4), "p%d" % i) for i in range(16)]
    del sd.labels[:]
    sd.labels.extend(sorted(set(l for _, l, _ in ds)))
    opt = optim.SGD(net.parameters(), lr=0.05, momentum=0.9, weight_decay=5e-4)
    sd.test_print_descriptor = lambda *a, **k: 0
    sd.train_siam_triplets_pos_couples(net, ds, (ds[:4], ds), TripletLoss(P.triplet_margin, False), opt)
    torch.save({k: v.clone() for k, v in net.state_dict().items()}, out + ".%d" % rank)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def test_augmented_training_does_not_depend_on_the_number_of_ranks(tmp_path):
    """--device=-1, augmentation on: one process and two ranks (gloo) end on the same weights, bit for bit -- the parameters and the noise of an
    image come from its key, not from a stream a rank would advance differently.  And the augmentation is really in the loop: the same run
    without it ends elsewhere."""
    single, dp, plain = str(tmp_path / "single"), str(tmp_path / "dp"), str(tmp_path / "plain")
    mp.spawn(_run_augmented_training, args=(1, 0, single, True), nprocs=1, join=True)
    mp.spawn(_run_augmented_training, args=(2, _free_port(), dp, True), nprocs=2, join=True)
    mp.spawn(_run_augmented_training, args=(1, 0, plain, False), nprocs=1, join=True)
    a, b0, b1, c = torch.load(single + ".0"), torch.load(dp + ".0"), torch.load(dp + ".1"), torch.load(plain + ".0")
    torch.manual_seed(0)
    init = _TinyNet().state_dict()
    assert sum(float((a[k].float() - init[k].float()).abs().sum()) for k in a) > 1e-3
    for k in a:
        assert torch.equal(a[k], b0[k]) and torch.equal(a[k], b1[k]), k
    assert any(not torch.equal(a[k], c[k]) for k in a)


def _captured_batch_builders(mod, train_set, monkeypatch, extra=()):
    """(create_epoch, create_batch) of a training main, captured where it hands them to train_gen; mining is replaced by 'negative = item 0'."""
    got = {}
    monkeypatch.setattr(mod, "train_gen", lambda *a, **k: got.update(create_epoch=a[8], create_batch=a[9]) or 0)
    if hasattr(mod, "get_similarities"):
        monkeypatch.setattr(mod, "get_similarities", lambda *a, **k: (None, -1))
        monkeypatch.setattr(mod, "mine_epoch_negatives", lambda sim, ds, couples, semi: torch.zeros(len(couples), dtype=torch.int64))
    mod.train_siam_triplets_pos_couples(None, train_set, (train_set[:2], train_set), *extra) if hasattr(mod, "get_similarities") else \
        mod.train_classif(type("Net", (), {"feature_size": 8})(), train_set, (train_set[:2], train_set), None, None)
    return got["create_epoch"], got["create_batch"]


@pytest.mark.parametrize("main", ["siamese_descriptor", "siamese_regions", "classif_finetune"])
def test_training_mains_build_augmented_batches_from_keys(main, monkeypatch):
    """create_epoch / create_batch of the three mains that take the augmenter, on the CPU: the items carry their place in the epoch, a batch is
    normalised fp32 without provenance, a slice of the items builds the slice of the batch (what a data-parallel rank does), another epoch draws
    other parameters, and the batch construction is not declared deterministic."""
    import importlib
    from train import _common as TC
    from utils.image import random_affine_noisy_cv
    mod = importlib.import_module("train." + main)
    saved, saved_raw = dict(mod.P.__dict__), dict(TC.RAW_INGEST)
    g = torch.Generator().manual_seed(3)
    ds = [(torch.randint(0, 256, (10, 12, 3), generator=g, dtype=torch.uint8), "l%d" % (i % 3), "p%d" % i) for i in range(9)]
    try:
        TC.RAW_INGEST["mean"], TC.RAW_INGEST["std"] = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
        P = mod.P
        P.cuda_device, P.train_seed, P.train_pre_proc, P.train_epoch_switch = -1, 4, False, 1
        P.train_trans = random_affine_noisy_cv(rotation=45, hs_range=.25, vs_range=.25, h_flip=True)
        del mod.labels[:]
        mod.labels.extend(sorted(set(l for _, l, _ in ds)))
        extra = {"siamese_descriptor": (None, None), "siamese_regions": (None, None, None, 0, True)}.get(main, ())
        create_epoch, create_batch = _captured_batch_builders(mod, ds, monkeypatch, extra)
        assert not getattr(create_batch, "deterministic", False)
        random.seed(1)
        from utils.dataset import get_pos_couples
        items, args = create_epoch(0, get_pos_couples(ds) if main != "classif_finetune" else ds, (ds[:2], ds))
        assert args == {"epoch": 0} and [it[-1] for it in items] == list(range(len(items)))
        inputs, targets = create_batch(items[:6], 6, **args)
        assert len(inputs) == (1 if main == "classif_finetune" else 3) and tuple(targets[0].shape) == (6,)
        for x in inputs:
            assert x.dtype == torch.float32 and tuple(x.shape) == (6, 3, 10, 12) and not hasattr(x, "_isx_rows")
        part, _ = create_batch(items[2:5], 3, **args)
        for x, y in zip(inputs, part):
            assert torch.equal(x[2:5], y)
        later, _ = create_batch(items[:6], 6, epoch=1)
        assert not torch.equal(later[0], inputs[0])
        if main != "classif_finetune":
            assert not torch.equal(inputs[0], inputs[1]) or items[0][2][0] is not items[0][2][1]
    finally:
        TC.RAW_INGEST.update(saved_raw)
        mod.P.__dict__.clear(); mod.P.__dict__.update(saved)
