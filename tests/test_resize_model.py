"""The cubic resize of 8-bit images without a GPU: the host twin isx.scale.resize_cubic_u8_host bit for bit against the integer model
(tests/_resize_model.py), the model against float64 torch bicubic, the reference's two size rules by hand, the boundary of libisxscale.so
(header == exports == binding, every refusal, no symbol shared with the other two libraries: the style of tests/test_mean_std_model.py), the
wrapper's argument contract on CPU tensors, the tool on the host route and the opt-in 8-bit second scale of train.classif_regions.

Against float64 bicubic every value is within 1 level: the 11-bit coefficients move the real-valued result by a fraction of a level (their
rounding errors, at most 3 / 2048 per axis, times 255) and the final rounding by at most half a level more; the largest distance on the case
table is 0.71.  The share of values that differ from rint() of the float result is printed, not asserted."""
import ast
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _augment_model as A
import _resize_model as M
from isx import prep, scale
from isx._lib import IsxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_KINDS = [(c, k) for c in M.CASES for k in M.KINDS]


def _host(img, size, **kw):
    return scale.resize_cubic_u8_host(torch.from_numpy(np.array(img)), size, **kw).numpy()


@pytest.mark.parametrize("c,kind", CASE_KINDS, ids=["%s-%s" % (M.case_id(c), k) for c, k in CASE_KINDS])
def test_host_twin_is_the_model_and_near_float_bicubic(c, kind):
    img, want = M.case(c, kind)
    got = _host(img, c[2:])
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    real = np.clip(M.float_bicubic(img, c[2:]), 0.0, 255.0)
    dist = float(np.abs(want.astype(np.float64) - real).max())
    share = float((want != np.rint(real)).mean())
    print("%s %s: at most %.3f levels from float64 bicubic, %.2f %% of the values differ from its rint" % (M.case_id(c), kind, dist, 100 * share))
    assert dist <= 1.0


def test_coefficient_tables():
    axes = set()
    for Hs, Ws, Hd, Wd in M.CASES:
        axes |= {(Hs, Hd), (Ws, Wd)}
    for _, _, _, (_, _, Hp, Wp), (Hd, Wd) in M.PAD_CASES:
        axes |= {(Hp, Hd), (Wp, Wd)}
    axes |= {(32768, 16384), (1, 16384), (32768, 1), (16383, 16384)}
    for S, T in sorted(axes):
        taps, coef = M.tables(S, T)
        assert all(sum(r) == 2048 for r in coef), (S, T)
        assert max(sum(abs(v) for v in r) for r in coef) <= 2818, (S, T)
        assert all(0 <= t <= S - 1 for r in taps for t in r), (S, T)
        got_t, got_c = scale.axis_table(S, T)
        assert got_t.tolist() == taps and got_c.tolist() == coef, (S, T)
    assert M.tables(448, 224)[1][0] == [-192, 1216, 1216, -192]               # r = D / 2: the familiar values
    assert M.tables(7, 7)[1] == [[0, 2048, 0, 0]] * 7 and [r[1] for r in M.tables(7, 7)[0]] == list(range(7))


def test_same_size_is_the_identity_and_a_constant_stays_constant():
    img = M.image("random", 13, 17, B=2)
    assert np.array_equal(M.resize(img, (13, 17)), img) and np.array_equal(_host(img, (13, 17)), img)
    for value in (0, 1, 127, 254, 255):
        flat = np.full((1, 9, 11, 3), value, np.uint8)
        for size in ((4, 5), (20, 31), (9, 40)):
            assert (M.resize(flat, size) == value).all() and (_host(flat, size) == value).all(), (value, size)


# ---- the size rules, by hand from the reference's lines ----------------------------------------------------------------------------------------------
def test_short_side_size_by_hand():
    # utils/image.py:66-77 / pre_process_dataset.py:48-54: (h, w) -> (oh, ow); int(round(float(new * long) / short)), Python 3's round (ties to even)
    for (H, W, new), want in [((448, 600, 224), (224, 300)), ((300, 200, 448), (672, 448)), ((200, 300, 200), (200, 300)),
                              ((300, 200, 200), (300, 200)), ((300, 200, 300), (450, 300)), ((5, 5, 3), (3, 3)), ((5, 5, 5), (5, 5)),
                              ((4, 6, 3), (3, 4)),             # 3 * 6 / 4 = 4.5 -> 4
                              ((4, 10, 3), (3, 8)),            # 7.5 -> 8
                              ((6, 4, 3), (4, 3)),             # 4.5 -> 4, the other axis
                              ((1080, 1920, 448), (448, 796)),     # 796.44
                              ((15, 30, 448), (448, 896))]:
        assert scale.short_side_size(H, W, new) == want, (H, W, new)
    with pytest.raises(IsxError):
        scale.short_side_size(0, 4, 3)


def test_aspect_pad_by_hand():
    # pre_process_dataset.py:29-46: short side -> ceil(long / max_ar); pad // 2 + pad % 2 in front, pad // 2 behind
    for (H, W, ar), want in [((10, 30, 2.0), (3, 0, 15, 30)),        # 5 rows: 3 on top, 2 below
                             ((30, 10, 2.0), (0, 3, 30, 15)),
                             ((9, 30, 2.0), (3, 0, 15, 30)),         # 6 rows: 3 and 3
                             ((8, 30, 2.0), (4, 0, 15, 30)),         # 7 rows: the odd one on top
                             ((10, 31, 2.0), (3, 0, 16, 31)),        # ceil(15.5) = 16
                             ((300, 1000, 2.0), (100, 0, 500, 1000)),
                             ((10, 20, 2.0), (0, 0, 10, 20)),        # exactly the ratio: not beyond it
                             ((20, 30, 2.0), (0, 0, 20, 30)), ((30, 30, 1.0), (0, 0, 30, 30)), ((10, 30, 0.5), (0, 0, 10, 30)),
                             ((10, 30, 1.0), (10, 0, 30, 30)), ((7, 30, 1.5), (7, 0, 20, 30))]:      # 13 rows: 7 on top, 6 below
        assert scale.aspect_pad(H, W, ar) == want, (H, W, ar)


@pytest.mark.parametrize("Hs,Ws,ar,pad,size", M.PAD_CASES, ids=["%dx%d" % (c[0], c[1]) for c in M.PAD_CASES])
def test_padded_source(Hs, Ws, ar, pad, size):
    assert scale.aspect_pad(Hs, Ws, ar) == pad and scale.short_side_size(pad[2], pad[3], 8) == size
    top, left, Hp, Wp = pad
    img = M.image("random", Hs, Ws, B=3)
    seed, ids = 1234567, [5, 6, 2 ** 40 + 1]
    for b in range(3):
        P = scale.padded_image(img[b], top, left, Hp, Wp, seed, ids[b])
        noise = A.noise(seed, ids[b], Hp, Wp)
        inside = np.zeros((Hp, Wp), bool)
        inside[top:top + Hs, left:left + Ws] = True
        assert np.array_equal(P[inside].reshape(Hs, Ws, 3), img[b]) and np.array_equal(P[~inside], noise[~inside])
        assert np.array_equal(P, M.padded(img[b], top, left, Hp, Wp, seed, ids[b]))
    want = M.resize(img, size, pad, seed, ids)
    got = _host(img, size, pad=pad, seed=seed, noise_ids=torch.tensor(ids))
    assert np.array_equal(got, want)
    # two noise ids on ONE image: different borders, and the outputs whose 16 taps all lie inside the image agree
    twice = np.stack([img[0], img[0]])
    a, b = M.resize(twice, size, pad, seed, [1, 2])
    assert not np.array_equal(a, b)
    ty, tx = np.array(M.tables(Hp, size[0])[0]), np.array(M.tables(Wp, size[1])[0])
    rows = (ty.min(1) >= top) & (ty.max(1) < top + Hs)
    cols = (tx.min(1) >= left) & (tx.max(1) < left + Ws)
    assert rows.any() and cols.any() and not (rows.all() and cols.all())
    assert np.array_equal(a[rows][:, cols], b[rows][:, cols])
    with pytest.raises(IsxError, match="noise_ids"):
        _host(img, size, pad=pad, seed=seed)


# ---- the boundary of libisxscale.so ------------------------------------------------------------------------------------------------------------------
def _declared():
    src = open(os.path.join(ROOT, "include", "isx_scale.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(isxs_[a-z0-9_]+)\s*\(", src)))


def _exported(path):
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm not available")
    out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return sorted({f[2] for f in (ln.split() for ln in out.splitlines()) if len(f) == 3})


def test_header_exports_and_binding_agree():
    names = _declared()
    assert names == ["isxs_last_error", "isxs_resize_cubic_u8", "isxs_version"]
    L = scale.lib()
    assert sorted(scale.EXPORTS) == names and all(hasattr(L, n) for n in names)
    assert L.isxs_version() >= 100
    exported = _exported(scale.LIB_PATH)
    assert [s for s in exported if s.startswith("isxs_")] == names
    assert not [s for s in exported if s.startswith("isx_") or s.startswith("isxp_")]


def test_the_other_libraries_export_nothing_of_this_one():
    from isx import _lib
    for path in (_lib.LIB_PATH, prep.LIB_PATH):
        assert not [s for s in _exported(path) if s.startswith("isxs_")], path


def test_refusals_without_gpu():
    L = scale.lib()
    entry = b"isxs_resize_cubic_u8"
    src, dst, ids = 4096 + 1, 65536 + 3, 8192                 # fake device pointers, never dereferenced
    good = dict(src=src, B=1, Hs=4, Ws=5, top=0, left=0, Hp=4, Wp=5, seed=0, ids=None, dst=dst, Hd=3, Wd=3)

    def call(**kw):
        a = dict(good, **kw)
        return L.isxs_resize_cubic_u8(a["src"], a["B"], a["Hs"], a["Ws"], a["top"], a["left"], a["Hp"], a["Wp"], a["seed"], a["ids"], a["dst"],
                                      a["Hd"], a["Wd"], None)

    def refused(text, **kw):
        assert call(**kw) == -1, kw
        err = L.isxs_last_error()
        assert err.startswith(entry) and text in err, err
    for side in ("Hs", "Ws", "Hp", "Wp", "Hd", "Wd"):
        refused(b"bad shape", **{side: 0})
        refused(b"bad shape", **{side: -2})
    refused(b"bad shape", B=-1)
    refused(b"bad shape", B=65536)
    refused(b"bad shape", top=-1, Hp=8, ids=ids)
    refused(b"bad shape", left=-1, Wp=8, ids=ids)
    refused(b"bad shape", top=1, ids=ids)                     # top + Hs = 5 > Hp = 4
    refused(b"bad shape", left=2, Wp=6, ids=ids)              # left + Ws = 7 > Wp = 6
    refused(b"bad shape", top=2 ** 31 - 2, ids=ids)           # top + Hs does not wrap
    refused(b"too large", Hd=16385)
    refused(b"too large", Wd=16385)
    refused(b"too large", Hp=32769, ids=ids)
    refused(b"too large", Wp=32769, ids=ids)
    refused(b"too large", Hp=26755, Wp=26755, ids=ids)        # 3 x 26755^2 = 2 147 490 075 >= 2^31
    refused(b"too large", Hd=16384, Wd=16384 * 3)             # Wd beyond its limit and 3 Hd Wd = 2^31 + 2^29
    refused(b"null pointer", src=None)
    refused(b"null pointer", dst=None)
    refused(b"null pointer", Hp=6, top=1)                     # padded, no noise ids
    refused(b"8-B aligned", Hp=6, top=1, ids=ids + 4)
    assert call(B=0, src=None, dst=None) == 0
    assert call(B=0, Hp=26750, Wp=26750, Hd=16384, Wd=16384, ids=None) == 0
    refused(b"bad shape", B=0, Hs=0, src=None, dst=None)      # the shape is checked before B == 0 returns


# ---- the wrapper's argument contract, on CPU tensors -------------------------------------------------------------------------------------------------
def u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def test_device_check_is_there_and_comes_last():
    with pytest.raises(IsxError, match="CUDA"):
        scale.resize_cubic_u8(u8(1, 4, 4, 3), (2, 2))
    with pytest.raises(IsxError, match="CUDA"):
        scale.resize_cubic_u8(u8(1, 4, 4, 3), (2, 2), out=u8(1, 2, 2, 3))


BAD = [
    ("img_u8", dict(img_u8=lambda: u8(1, 4, 4, 4))),
    ("img_u8", dict(img_u8=lambda: torch.zeros(1, 4, 4, 3))),
    ("img_u8", dict(img_u8=lambda: u8(1, 4, 8, 3)[:, :, ::2])),
    ("img_u8", dict(img_u8=lambda: u8(4, 4, 3))),
    ("out", dict(out=lambda: u8(1, 2, 3, 3))),
    ("out", dict(out=lambda: torch.zeros((1, 2, 2, 3), dtype=torch.int8))),
    ("out", dict(out=lambda: u8(1, 2, 4, 3)[:, :, ::2])),
    ("noise_ids", dict(noise_ids=lambda: torch.zeros(1, dtype=torch.int32))),
    ("noise_ids", dict(noise_ids=lambda: torch.zeros(2, dtype=torch.int64))),
    ("noise_ids", dict(pad=(1, 0, 5, 4))),
    ("bad shape", dict(pad=(1, 0, 4, 4), noise_ids=lambda: torch.zeros(1, dtype=torch.int64))),
    ("bad shape", dict(size=(0, 2))),
    ("image too large", dict(size=(2, 16385))),
    ("size", dict(size=7)),
]


@pytest.mark.parametrize("named,override", BAD, ids=["%s-%d" % (n.replace(" ", "_"), i) for i, (n, _) in enumerate(BAD)])
def test_one_wrong_argument_is_named(named, override):
    kw = dict(dict(img_u8=lambda: u8(1, 4, 4, 3), size=(2, 2), pad=None, noise_ids=None, out=None), **override)
    with pytest.raises(IsxError, match=r"^%s(:| has | must )" % named) as e:
        scale.resize_cubic_u8(**{k: v() if callable(v) else v for k, v in kw.items()})
    assert "CUDA" not in str(e.value)
    if named not in ("out", "noise_ids") or "pad" in override:  # the host twin refuses the same arguments
        kw.pop("out")
        with pytest.raises(IsxError, match=r"^%s(:| has | must )" % named):
            scale.resize_cubic_u8_host(**{k: v() if callable(v) else v for k, v in kw.items()})


def test_no_assert_statement_in_scale():
    tree = ast.parse(inspect.getsource(scale))
    assert not [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Assert)]


# ---- the tool on the host route ----------------------------------------------------------------------------------------------------------------------
def test_tool_on_the_host(tmp_path, monkeypatch, capsys):
    from PIL import Image
    import pre_process_dataset
    monkeypatch.setenv("ISX_DECODE_PROCS", "2")
    # sorted by name: two of one shape (one launch), a square, one beyond the ratio (10 x 40 -> 20 x 40 canvas, 5 rows on top), one already 16
    shapes = [(20, 30), (20, 30), (24, 24), (10, 40), (16, 20), (40, 12)]
    folder, out = tmp_path / "my_set", tmp_path / "pre_proc" / "my_set_16"
    (folder / "test").mkdir(parents=True)
    images = {}
    for i, (H, W) in enumerate(shapes):
        images["a-%d.png" % i] = M.image("random", H, W, salt=i)[0]
        Image.fromarray(images["a-%d.png" % i]).save(str(folder / ("a-%d.png" % i)))
    query = M.image("ramp", 33, 21)[0]
    Image.fromarray(query).save(str(folder / "test" / "q-0.png"))
    try:
        train, test = pre_process_dataset.main(["--dataset=" + str(folder), "--out=" + str(out), "--short-side=16", "--device=-1", "--batch=4",
                                                "--seed=9"])
        again = tmp_path / "again"
        pre_process_dataset.main(["--dataset=" + str(folder), "--out=" + str(again), "--short-side=16", "--device=-1", "--batch=1", "--seed=9"])
    finally:
        from train import _decode_farm
        _decode_farm.shutdown()
    assert "6 + 1 images written" in capsys.readouterr().out
    want_sizes = [(16, 24), (16, 24), (16, 16), (16, 32), (16, 20), (32, 16)]      # 40 x 12: 4 columns of noise on either side, 40 x 20 -> 32 x 16
    assert [os.path.basename(p) for p, _ in train] == sorted(images) and [s for _, s in train] == want_sizes
    for i, (path, size) in enumerate(train):
        name = os.path.basename(path)
        got = np.asarray(Image.open(path).convert("RGB"))
        H, W = shapes[i]
        pad = scale.aspect_pad(H, W, 2.0)
        want = M.resize(images[name][None], size, pad, 9, [i])[0]
        assert got.shape == want.shape and np.array_equal(got, want), name
        assert open(path, "rb").read() == open(str(again / name), "rb").read(), name        # --batch changes nothing
    assert np.array_equal(np.asarray(Image.open(str(out / "a-4.png")).convert("RGB")), images["a-4.png"])     # neither pad nor resize
    assert [os.path.basename(p) for p, _ in test] == ["q-0.png"] and test[0][1] == (25, 16)
    got = np.asarray(Image.open(str(out / "test" / "q-0.png")).convert("RGB"))
    assert np.array_equal(got, M.resize(query[None], (25, 16))[0])
    # --size=WxH
    fixed = tmp_path / "fixed"
    try:
        train, _ = pre_process_dataset.main(["--dataset=" + str(folder), "--out=" + str(fixed), "--size=10x7", "--device=-1", "--max-ar=0"])
    finally:
        from train import _decode_farm
        _decode_farm.shutdown()
    assert [s for _, s in train] == [(7, 10)] * 6
    assert np.array_equal(np.asarray(Image.open(str(fixed / "a-3.png")).convert("RGB")), M.resize(images["a-3.png"][None], (7, 10))[0])
    with pytest.raises(SystemExit):
        pre_process_dataset.main(["--dataset=" + str(folder), "--out=" + str(fixed), "--size=10x7", "--short-side=5", "--device=-1"])


# ---- the second scale of train.classif_regions from the 8-bit image ---------------------------------------------------------------------------------
def test_multi_scale_items_from_u8(monkeypatch):
    from train import _common as TC
    from train import classif_regions as CR
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    monkeypatch.setitem(TC.RAW_INGEST, "mean", mean)
    monkeypatch.setitem(TC.RAW_INGEST, "std", std)
    monkeypatch.setattr(CR.P, "cuda_device", -1, raising=False)
    raw = [torch.from_numpy(np.array(M.image(kind, 32, 40, salt=i)[0])) for i, kind in enumerate(("random", "ramp"))]
    train_set = [(im, "l%d" % i, "p%d" % i) for i, im in enumerate(raw)]

    def normalise(u8_hw3):
        x = torch.from_numpy(np.array(u8_hw3)).permute(2, 0, 1).float().div(255.0)
        return (x - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)
    today = CR.multi_scale_items(train_set, [None, 16])
    named = CR.multi_scale_items(train_set, [None, 16], pixels="normalised")
    u8_items = CR.multi_scale_items(train_set, [None, 16], pixels="u8")
    for i, im in enumerate(raw):
        full = normalise(im.numpy())
        old = torch.nn.functional.interpolate(full.unsqueeze(0), size=(16, 20), mode="bicubic", align_corners=False)[0]
        assert torch.equal(today[i][0][0], full) and torch.equal(today[i][0][1], old)                # the default: today's result
        assert all(torch.equal(a, b) for a, b in zip(today[i][0], named[i][0]))
        want = normalise(M.resize(im.numpy()[None], (16, 20))[0])
        assert torch.equal(u8_items[i][0][0], full) and torch.equal(u8_items[i][0][1], want)
        assert u8_items[i][0][1].shape == old.shape and not torch.equal(u8_items[i][0][1], old)
        assert u8_items[i][1:] == train_set[i][1:]
    with pytest.raises(ValueError, match="uint8"):
        CR.multi_scale_items([(today[0][0][0], "l", "p")], [None, 16], pixels="u8")
    with pytest.raises(ValueError, match="pixels"):
        CR.multi_scale_items(train_set, [None, 16], pixels="bgr")
    assert TC.parse_scale_pixels("u8") == "u8" and TC.parse_scale_pixels("normalised") == "normalised"
    with pytest.raises(ValueError):
        TC.parse_scale_pixels("fp16")
