"""Dataset statistics without a GPU: isx.prep.mean_std against the float64 model of the reference's two conventions (tests/_mean_std_model.py),
the file it writes, the tool on the host path, the wrapper's argument contract on CPU tensors (the style of tests/test_ops_contract.py) and
the boundary of libisxprep.so (the style of tests/test_abi.py): header == exports == binding, every refusal, no symbol shared with libisx.so.

Tolerance of the model comparisons: 1e-12 relative.  The model is a two-pass float64 evaluation with numpy's pairwise sums over at most 2e5
values -- its own error is a few tens of ulp (2.2e-16 each) --, mean_std is exact rational arithmetic rounded once (std: twice)."""
import ast
import decimal
import inspect
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import _mean_std_model as M
from isx import prep
from isx._lib import IsxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-12
SPEC = "synthetic:CLICIDE_video_224sq:n=12:q=4:labels=3:size=32"


def _sets():
    rng = np.random.default_rng(11)
    return {"1x1x2": M.random_images(rng, 1, 1, 2), "5x7x9": M.random_images(rng, 5, 7, 9), "64x32x32": M.random_images(rng, 64, 32, 32),
            "ragged9": M.ragged_images(rng)}


SETS = _sets()


def _moments(images):
    return np.concatenate([M.moments(im[None]) for im in images]), [im.shape[0] * im.shape[1] for im in images]


def _close(got, want):
    assert len(got) == len(want) == 3 and all(type(g) is float for g in got), got
    for g, w in zip(got, want):
        assert abs(g - w) <= RTOL * abs(w), (g, w, abs(g - w) / abs(w))


@pytest.mark.parametrize("per_image", [False, True], ids=["pooled", "per_image"])
@pytest.mark.parametrize("name", sorted(SETS))
def test_mean_std_matches_the_model(name, per_image):
    images = SETS[name]
    mom, pixels = _moments(images)
    mean, std = prep.mean_std(mom, pixels, per_image)
    want_mean, want_std = (M.per_image if per_image else M.pooled)(images)
    _close(mean, want_mean)
    _close(std, want_std)
    # a torch tensor of moments and a tensor of pixel counts are the same input
    assert prep.mean_std(torch.from_numpy(mom), torch.tensor(pixels), per_image) == (mean, std)


@pytest.mark.parametrize("per_image", [False, True], ids=["pooled", "per_image"])
def test_equal_images_have_no_deviation(per_image):
    img = np.empty((4, 6, 5, 3), np.uint8)
    img[...] = (7, 130, 255)
    mean, std = prep.mean_std(M.moments(img), [30] * 4, per_image)
    assert std == [0.0, 0.0, 0.0]
    assert mean == [7 / 255, 130 / 255, 1.0]                  # Python's int / int is correctly rounded


def test_one_image_of_two_values_is_the_closed_form():
    a, b = (3, 200, 17), (250, 100, 17)
    img = np.array([[[a, b]]], np.uint8)                       # (1, 1, 2, 3)
    mom = M.moments(img)
    mean, std = prep.mean_std(mom, [2])
    assert mean == [(x + y) / 510 for x, y in zip(a, b)]
    assert std == [math.sqrt(float(Fraction((x - y) ** 2, 2 * 65025))) for x, y in zip(a, b)]          # (d/255)^2 / 2 over n - 1 = 1
    mean, std = prep.mean_std(mom, [2], per_image=True)
    assert mean == [(x + y) / 510 for x, y in zip(a, b)]
    assert std == [math.sqrt(float(Fraction((x - y) ** 2, 4 * 65025))) for x, y in zip(a, b)]          # biased: over n = 2
    # one value has no unbiased deviation (Tensor.std() of one element)
    assert all(math.isnan(s) for s in prep.mean_std(M.moments(img[:, :, :1]), [1])[1])


def test_pooled_is_at_least_as_close_to_the_exact_value_as_fp32():
    """The reference takes T[:, c].mean() / .std() of an fp32 tensor; the exact values are rationals of the integers (the deviation: the root of
    one, here to 60 digits).  A <= on two distances: what fp32 represents exactly is reproduced exactly."""
    images = SETS["64x32x32"]
    mom, pixels = _moments(images)
    mean, std = prep.mean_std(mom, pixels)
    T = torch.from_numpy(np.stack(images)).permute(0, 3, 1, 2).float().div(255)
    n = sum(pixels)
    for c in range(3):
        s1, s2 = int(mom[:, c, 0].sum()), int(mom[:, c, 1].sum())
        exact_mean = Fraction(s1, 255 * n)
        exact_var = Fraction(s2 * n - s1 * s1, 65025 * n * (n - 1))
        ref_mean, ref_std = float(T[:, c].mean()), float(T[:, c].std())
        assert abs(Fraction(mean[c]) - exact_mean) <= abs(Fraction(ref_mean) - exact_mean)
        with decimal.localcontext() as ctx:
            ctx.prec = 60
            exact_std = (decimal.Decimal(exact_var.numerator) / decimal.Decimal(exact_var.denominator)).sqrt()
            assert abs(decimal.Decimal(std[c]) - exact_std) <= abs(decimal.Decimal(ref_std) - exact_std)


def test_host_moments_are_the_models():
    for cid, _, _, _ in M.KERNEL_CASES[:7]:
        img = M.kernel_image(cid)
        got = prep.channel_moments_u8_host(torch.from_numpy(img))
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), M.moments(img)), cid
    ones = np.full((1, 258, 257, 3), 255, np.uint8)
    assert prep.channel_moments_u8_host(torch.from_numpy(ones))[0, 0].tolist() == [255 * 258 * 257, 4311547650]


def test_file_round_trip(tmp_path):
    from utils.general import read_mean_std
    mom, pixels = _moments(SETS["5x7x9"])
    mean, std = prep.mean_std(mom, pixels)
    path = str(tmp_path / "ms.txt")
    prep.write_mean_std(path, mean, std)
    assert read_mean_std(path) == (mean, std)
    text = open(path).read()
    assert text == " ".join(map(repr, mean)) + "\n" + " ".join(map(repr, std)) + "\n"
    lines = text.split("\n")
    assert len(lines) == 3 and lines[2] == "" and all(len(ln.split(" ")) == 3 for ln in lines[:2])
    assert [float(v) for ln in lines[:2] for v in ln.split(" ")] == mean + std


# ---- the tool on the host path ---------------------------------------------------------------------------------------------------------------------
def _tool(*argv):
    import create_mean_std_file
    return create_mean_std_file.main(list(argv))


def _spec_images():
    from test._common import load_sets
    from train._common import _raw_u8_set
    _, ref = load_sets(SPEC, [])
    return [im.numpy() for im, _, _ in _raw_u8_set(ref)]


def test_tool_on_the_host(tmp_path):
    from utils.general import read_mean_std
    images = _spec_images()
    assert len(images) == 12 and images[0].shape == (32, 32, 3) and images[0].dtype == np.uint8
    out = str(tmp_path / "new_dir" / "ms.txt")                 # the directory does not exist yet
    _tool("--dataset=" + SPEC, "--device=-1", "--out=" + out)
    mean, std = read_mean_std(out)
    want_mean, want_std = M.pooled(images)
    _close(mean, want_mean)
    _close(std, want_std)
    small = str(tmp_path / "batch5.txt")
    _tool("--dataset=" + SPEC, "--device=-1", "--batch=5", "--out=" + small)
    large = str(tmp_path / "batch256.txt")
    _tool("--dataset=" + SPEC, "--device=-1", "--batch=256", "--out=" + large)
    assert open(small, "rb").read() == open(large, "rb").read() == open(out, "rb").read()
    per = str(tmp_path / "per_image.txt")
    _tool("--dataset=" + SPEC, "--device=-1", "--per-image", "--out=" + per)
    mean, std = read_mean_std(per)
    want_mean, want_std = M.per_image(images)
    _close(mean, want_mean)
    _close(std, want_std)
    assert std != read_mean_std(out)[1]


def test_tool_default_output_and_unknown_dataset(tmp_path, monkeypatch, capsys):
    from train.global_p import mean_std_files
    monkeypatch.chdir(tmp_path)
    _tool("--dataset=" + SPEC, "--device=-1")
    assert os.path.exists(os.path.join(str(tmp_path), mean_std_files["CLICIDE_video_224sq"]))
    assert "pooled" in capsys.readouterr().out
    with pytest.raises(SystemExit) as e:
        _tool("--dataset=synthetic:no_such_dataset:n=4:size=8", "--device=-1")
    assert e.value.code == 2 and "usage:" in capsys.readouterr().err


def test_tool_reads_the_folder_not_its_test_subfolder(tmp_path, monkeypatch):
    """A ragged folder of PNGs: listed like utils.dataset.get_images_labels, decoded to 8-bit RGB, per-image convention; test/ is not read."""
    from PIL import Image
    from utils.general import read_mean_std
    monkeypatch.setenv("ISX_DECODE_PROCS", "2")
    rng = np.random.default_rng(5)
    images = M.ragged_images(rng, n=7, lo=5, hi=12)
    folder = tmp_path / "my_set"
    (folder / "test").mkdir(parents=True)
    for i, im in enumerate(images):
        Image.fromarray(im).save(str(folder / ("a-%d.png" % i)))
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(str(folder / "test" / "q-0.png"))
    out = str(tmp_path / "ms.txt")
    try:
        _tool("--dataset=" + str(folder), "--device=-1", "--batch=3", "--out=" + out)
    finally:
        from train import _decode_farm
        _decode_farm.shutdown()
    mean, std = read_mean_std(out)
    want_mean, want_std = M.per_image(images)
    _close(mean, want_mean)
    _close(std, want_std)


# ---- the wrapper's argument contract, on CPU tensors -----------------------------------------------------------------------------------------------
def u8(*shape):
    return torch.zeros(shape, dtype=torch.uint8)


def test_device_check_is_there_and_comes_last():
    with pytest.raises(IsxError, match="CUDA"):
        prep.channel_moments_u8(u8(1, 2, 2, 3))
    with pytest.raises(IsxError, match="CUDA"):
        prep.channel_moments_u8(u8(1, 2, 2, 3), out=torch.zeros((1, 3, 2), dtype=torch.int64))


BAD = [
    ("img_u8", dict(img_u8=lambda: u8(1, 2, 2, 4))),
    ("img_u8", dict(img_u8=lambda: torch.zeros(1, 2, 2, 3))),
    ("img_u8", dict(img_u8=lambda: u8(1, 2, 4, 3)[:, :, ::2])),
    ("out", dict(out=lambda: torch.zeros((1, 3, 1), dtype=torch.int64))),
    ("out", dict(out=lambda: torch.zeros((1, 3, 2), dtype=torch.int32))),
    ("out", dict(out=lambda: torch.zeros((1, 3, 4), dtype=torch.int64)[:, :, ::2])),
]


@pytest.mark.parametrize("named,override", BAD, ids=["%s-%d" % (n, i) for i, (n, _) in enumerate(BAD)])
def test_one_wrong_argument_is_named(named, override):
    kw = dict(dict(img_u8=lambda: u8(1, 2, 2, 3), out=None), **override)
    with pytest.raises(IsxError, match=r"^%s (has|must) " % named) as e:
        prep.channel_moments_u8(**{k: v() if callable(v) else v for k, v in kw.items()})
    assert "CUDA" not in str(e.value)


def test_no_assert_statement_in_prep():
    tree = ast.parse(inspect.getsource(prep))
    assert not [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Assert)]


# ---- the boundary of libisxprep.so -----------------------------------------------------------------------------------------------------------------
def _declared():
    src = open(os.path.join(ROOT, "include", "isx_prep.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(isxp_[a-z0-9_]+)\s*\(", src)))


def _exported(path):
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm not available")
    out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return sorted({f[2] for f in (ln.split() for ln in out.splitlines()) if len(f) == 3})


def test_header_exports_and_binding_agree():
    names = _declared()
    assert names == ["isxp_channel_moments_u8", "isxp_last_error", "isxp_version"]
    L = prep.lib()
    assert sorted(prep.EXPORTS) == names and all(hasattr(L, n) for n in names)
    assert L.isxp_version() >= 100
    exported = _exported(prep.LIB_PATH)
    assert [s for s in exported if s.startswith("isxp_")] == names
    assert not [s for s in exported if s.startswith("isx_")]


def test_libisx_exports_nothing_of_the_preparation_library():
    from isx import _lib
    assert not [s for s in _exported(_lib.LIB_PATH) if s.startswith("isxp_")]


def test_refusals_without_gpu():
    L = prep.lib()
    entry = b"isxp_channel_moments_u8"
    img, mom = 4096 + 1, 8192                                 # fake device pointers, never dereferenced: any alignment for img, 8-B for moments

    def refused(text, *args):
        assert L.isxp_channel_moments_u8(*args, None) == -1
        err = L.isxp_last_error()
        assert err.startswith(entry) and text in err, err
    refused(b"bad shape", img, 1, 0, 4, mom)
    refused(b"bad shape", img, 1, 4, 0, mom)
    refused(b"bad shape", img, 1, -3, 4, mom)
    refused(b"bad shape", img, -1, 4, 4, mom)
    refused(b"bad shape", img, 65536, 4, 4, mom)
    refused(b"too large", img, 1, 26755, 26755, mom)          # 3 x 26755^2 = 2 147 490 075 >= 2^31
    refused(b"too large", img, 1, 1, 715827883, mom)          # 3 W = 2^31 + 1
    refused(b"null pointer", None, 1, 4, 4, mom)
    refused(b"null pointer", img, 1, 4, 4, None)
    refused(b"8-B aligned", img, 1, 4, 4, mom + 4)
    refused(b"8-B aligned", img, 1, 4, 4, mom + 1)
    assert L.isxp_channel_moments_u8(None, 0, 4, 4, None, None) == 0
    assert L.isxp_channel_moments_u8(img, 0, 26750, 26750, mom, None) == 0
    refused(b"bad shape", None, 0, 0, 4, None)                # the shape is checked before B == 0 returns
