"""The CPU model of libisxalex (tests/_alex_model.py) against what it has to equal -- oracle.conv3x3_nhwc bit for bit where both define the layer,
float64 within fp32 bounds, torch's CPU max-pool bit for bit -- and against the wrong orders it has to tell apart; the route of
model.nn_utils.fold_batch_norm for AlexNet-style trunks on CPU tensors; and the boundary of libisxalex.so: header == ctypes table == exports,
refusals before any launch, the wrapper's argument contract.  No GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as Fn

import _alex_model as A
import _guards as G
import oracle as O
from isx import alex
from isx._lib import IsxError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = 2.0 ** -24                                      # unit roundoff of fp32


# ---- the convolution model ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3x3s1_32to64", "3x3s2_32to64", "3x3s1_192to384", "3x3s2_192to384"])
@pytest.mark.parametrize("relu", [True, False])
def test_model_is_the_oracle_on_3x3(name, relu):
    x, w, bias, y = A.conv_case(name, relu)
    stride = A.CONV_CASES[name][6]
    G.assert_bits(y, O.conv3x3_nhwc(x, w, bias, stride, None, relu), name)


@pytest.mark.parametrize("name", ["11x11s4_3to64", "5x5_64to192", "6x6_32to32", "1x1_4to64", "3x3s3_5to32", "3x3s1_192to384"])
def test_model_within_fp32_bounds_of_float64(name):
    """A chain of c terms is off by at most gamma_c sum|terms|, the n chunk sums are added with n roundings and the bias with one more:
    |y - y64| <= (c + n + 1) u (1 + small) sum|x w| + |bias|, c = 64 terms per chunk.  ReLU is 1-Lipschitz."""
    x, w, bias, y = A.conv_case(name)
    B, H, W, Cin, Cout, K, stride, pad = A.CONV_CASES[name]
    y64, mag = A.conv2d_f64(x, w, bias, stride, pad, True)
    n = -(-K * K * Cin // A.CHUNK)
    err = np.abs(y.astype(np.float64) - y64)
    bound = (min(A.CHUNK, K * K * Cin) + n + 1) * U * 1.001 * mag
    print("%s: largest error / bound = %.3f" % (name, float((err / bound).max())))
    assert (err <= bound).all()
    assert float((err / bound).max()) > 1e-4, "a model this close to float64 is not rounding in fp32"


@pytest.mark.parametrize("name", ["11x11s4_3to64", "5x5_64to192", "3x3s1_32to64", "3x3s1_192to384"])
def test_model_is_told_apart_from_wrong_orders(name):
    """One chain over the whole reduction, and chunks counted over the live taps only.  The second order IS the model's where a tap is a whole number
    of chunks (Cin % 64 == 0: leaving a padding tap out removes chains that are +0) -- what lets a kernel skip such taps -- and is not anywhere else."""
    x, w, bias, y = A.conv_case(name)
    B, H, W, Cin, Cout, K, stride, pad = A.CONV_CASES[name]
    one = A.conv2d_one_chain(x, w, bias, stride, pad, True)
    assert (G.bits(one) != G.bits(y)).mean() > 0.05, "one chain over the whole reduction gives the model's bits"
    skip = A.conv2d_chunks_skip_padding(x, w, bias, stride, pad, True)
    inside = A.tap_inside(H, W, K, stride, pad)
    whole = inside.all(1)                                                   # output pixels whose window has no padding tap
    assert whole.any() and not whole.all()
    differs = (G.bits(skip) != G.bits(y)).reshape(B, -1, Cout)
    assert not differs[:, whole].any(), "without a padding tap the two orders are one"
    if Cin % A.CHUNK == 0:
        assert not differs.any()
    else:
        assert differs[:, ~whole].mean() > 0.05, "chunks counted without the padding taps give the model's bits"


def test_padding_terms_past_the_reduction_change_nothing():
    """The kernel runs the last chain on over zero-weight, zero-activation terms up to its k-tile: the model with such terms appended is the model."""
    x, w, bias, y = A.conv_case("11x11s4_3to64")
    Acol, (B, Ho, Wo) = A.im2col(x, 11, 4, 2)
    Wm = w.reshape(64, -1)
    z = lambda a, n: np.concatenate([a, np.zeros((a.shape[0], n), F)], 1)
    padded = A.epilogue(A.two_level(z(Acol, 21), z(Wm, 21)), bias, True).reshape(B, Ho, Wo, 64)
    assert Acol.shape[1] == 363 and (363 + 21) % 32 == 0
    G.assert_bits(padded, y)


# ---- the pool model ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", A.POOL_CASES, ids=lambda s: "x".join(map(str, s)))
def test_pool_model_is_torch_cpu(shape):
    x, y = A.pool_case(shape)
    assert np.isnan(x).any() and np.isinf(x).any() and (G.bits(x) == 0x80000000).any()
    want = Fn.max_pool2d(torch.from_numpy(np.array(x)).permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1).contiguous().numpy()
    G.assert_bits(y, want, shape)
    want_cl = Fn.max_pool2d(torch.from_numpy(np.array(x)).permute(0, 3, 1, 2).contiguous(), 3, 2).permute(0, 2, 3, 1).contiguous().numpy()
    G.assert_bits(y, want_cl, shape)
    assert G.bits(y[0, 0, 0, :4]).tolist() == [0x80000000, 0x00000000, 0xFFC00001, 0xFF800000]


# ---- the route ---------------------------------------------------------------------------------------------------------------------------------
def _nets():
    from isx import backbones
    from model.ModelDefinition import Maxnet
    torch.manual_seed(3)
    return [("alexnet", backbones.alexnet(pretrained=True).eval()), ("Maxnet", Maxnet(17).eval())]


@pytest.mark.parametrize("mode", ["auto", "1"])
def test_fold_builds_the_alex_modules(mode, monkeypatch):
    from model import nn_utils
    monkeypatch.setattr(nn_utils, "_ALEX_MODE", mode)
    for name, net in _nets():
        f = nn_utils.fold_batch_norm(net.features)
        kinds = [type(m).__name__ for m in f]
        assert kinds == ["_ChannelsLastEntry", "_AlexConv", "_AlexPool", "_AlexConv", "_AlexPool", "_AlexConv", "_AlexConv", "_AlexConv", "_AlexPool"], (name, kinds)
        convs = [m for m in f if isinstance(m, nn_utils._AlexConv)]
        assert [c.kind for c in convs] == ["conv11", "conv5", "conv3", "conv3", "conv3"]
        assert [c.libisx_3x3 for c in convs] == [False, False, True, True, True] and all(c.act is not None for c in convs)
        assert not any(m is o for m in f.modules() for o in net.features.modules()), "the folded trunk shares a module with the original"


def test_mode_0_is_the_parent_route(monkeypatch):
    from model import nn_utils
    monkeypatch.setattr(nn_utils, "_ALEX_MODE", "0")
    for name, net in _nets():
        f = nn_utils.fold_batch_norm(net.features)
        assert [type(m) for m in f][1:] == [type(m) for m in net.features], name


def test_resnet_trunk_has_no_alex_module():
    from isx import backbones
    from model import nn_utils
    f = nn_utils.fold_batch_norm(nn_utils.extract_layers(backbones.resnet18(pretrained=True).eval())[0])
    assert not [m for m in f.modules() if isinstance(m, (nn_utils._AlexConv, nn_utils._AlexPool))]


@pytest.mark.parametrize("mode", ["auto", "1", "0"])
def test_folded_trunk_on_cpu_is_the_unfolded_one(mode, monkeypatch):
    from model import nn_utils
    monkeypatch.setattr(nn_utils, "_ALEX_MODE", mode)
    x = torch.randn(2, 3, 67, 99, generator=torch.Generator().manual_seed(1))
    for name, net in _nets():
        f = nn_utils.fold_batch_norm(net.features)
        with torch.no_grad():
            assert torch.equal(f(x), net.features(x)), name
        y = f(x)                                                           # with autograd: the modules themselves
        assert y.requires_grad and torch.equal(y.detach(), net.features(x).detach())


@pytest.mark.parametrize("mode,folded", [("1", True), ("auto", True), ("0", False)])
def test_prepare_for_inference_folds_where_the_route_is_active(mode, folded, monkeypatch):
    import types
    from model import nn_utils
    from train import _common as TC
    monkeypatch.setattr(nn_utils, "_ALEX_MODE", mode)
    assert nn_utils._ALEX_AUTO_KINDS == {"conv11", "conv5", "conv3", "pool"}        # what DESIGN 4.1 measured `auto` into
    for name, net in _nets():
        assert nn_utils.alex_route_active(net.features) == folded
        TC.prepare_for_inference(net, types.SimpleNamespace(fold_bn=True))
        assert isinstance(net.features[0], nn_utils._ChannelsLastEntry) == folded, name
        assert not nn_utils.alex_route_active(net.features) or not folded              # a folded trunk is not folded twice
    monkeypatch.setattr(nn_utils, "_ALEX_AUTO_KINDS", frozenset())
    monkeypatch.setattr(nn_utils, "_ALEX_MODE", "auto")
    assert not nn_utils.alex_route_active(_nets()[0][1].features)                        # `auto` with no kind taken: the trunk stays as it is


def test_applicability():
    ok = lambda *a, **k: alex.conv2d_applicable(nn.Conv2d(*a, **k))
    assert ok(3, 64, 11, stride=4, padding=2) and ok(64, 192, 5, padding=2) and ok(192, 384, 3, padding=1) and ok(8, 32, 1)
    assert not ok(3, 48, 3) and not ok(4, 32, (3, 5)) and not ok(4, 32, 3, stride=(1, 2)) and not ok(4, 32, 3, padding=3) and not ok(4, 32, 3, stride=5)
    assert not ok(4, 32, 3, groups=2) and not ok(4, 32, 3, dilation=2) and not ok(4, 32, 3, padding="same") and not ok(4, 32, 17)
    assert not ok(4, 32, 3, padding=1, padding_mode="reflect")


# ---- the boundary of libisxalex.so -------------------------------------------------------------------------------------------------------------
_CTYPE = {"int": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p}


def _prototypes():
    """name -> (restype, [argtypes]) from include/isx_alex.h: every pointer parameter (and the stream handle) is a c_void_p."""
    src = open(os.path.join(ROOT, "include", "isx_alex.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for res, name, params in re.findall(r"^\s*((?:const\s+)?\w+\s*\*?)\s*\b(isxa_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src, flags=re.M):
        args = []
        for p in [q.strip() for q in params.split(",") if q.strip() and q.strip() != "void"]:
            ctype = re.sub(r"\s+", " ", re.match(r"(.*?)\w+$", p, flags=re.S).group(1)).strip().replace(" *", "*")      # the parameter without its name
            args.append(C.c_void_p if ctype.endswith("*") or ctype == "isxa_stream_t" else _CTYPE[ctype])
        out[name] = (_CTYPE[re.sub(r"\s+", " ", res).strip().replace(" *", "*")], args)
    return out


def _exported(path, kinds="TDBR"):
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm not available")
    out = subprocess.run([nm, "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return sorted({f[2] for f in (ln.split() for ln in out.splitlines()) if len(f) == 3 and f[1] in kinds})


def test_header_binding_and_exports_agree():
    protos = _prototypes()
    assert sorted(protos) == ["isxa_conv2d_nhwc", "isxa_last_error", "isxa_maxpool3s2_nhwc", "isxa_version"]
    assert protos == alex._SIGNATURES and sorted(alex.EXPORTS) == sorted(protos)
    L = alex.lib()
    assert all(hasattr(L, n) for n in protos) and L.isxa_version() >= 100
    assert _exported(alex.LIB_PATH, "T") == sorted(protos), "the library's functions are the header's, all isxa_"
    assert [s for s in _exported(alex.LIB_PATH) if s.startswith("isx")] == sorted(protos)


def test_the_other_libraries_export_nothing_of_this_one():
    from isx import _lib, prep, scale
    for path in (_lib.LIB_PATH, prep.LIB_PATH, scale.LIB_PATH):
        assert not [s for s in _exported(path) if s.startswith("isxa_")], path


def test_header_constants_match():
    src = open(os.path.join(ROOT, "include", "isx_alex.h")).read()
    assert int(re.search(r"#define ISXA_CONV_CHUNK (\d+)", src).group(1)) == A.CHUNK
    assert int(re.search(r"#define ISXA_MAX_K (\d+)", src).group(1)) == alex.MAX_K
    assert int(re.search(r"#define ISX_CONV_CHUNK (\d+)", open(os.path.join(ROOT, "include", "isx.h")).read()).group(1)) == A.CHUNK


def test_refusals_without_gpu():
    L = alex.lib()
    for entry, good, cases in (("isxa_conv2d_nhwc", A.CONV_GOOD, A.CONV_REFUSALS), ("isxa_maxpool3s2_nhwc", A.POOL_GOOD, A.POOL_REFUSALS)):
        for text, kw in cases:
            assert A.call_abi(L, entry, dict(good, **kw), None) == -1, (entry, kw)
            err = L.isxa_last_error()
            assert err.startswith(entry.encode() + b":") and text.encode() in err, (kw, err)
    # B == 0 launches nothing and needs no pointer; the shape is still checked first
    assert A.call_abi(L, "isxa_conv2d_nhwc", dict(A.CONV_GOOD, B=0, x=None, w=None, bias=None, y=None), None) == 0
    assert A.call_abi(L, "isxa_maxpool3s2_nhwc", dict(A.POOL_GOOD, B=0, x=None, y=None), None) == 0
    assert A.call_abi(L, "isxa_conv2d_nhwc", dict(A.CONV_GOOD, B=0, K=0), None) == -1
    assert A.call_abi(L, "isxa_maxpool3s2_nhwc", dict(A.POOL_GOOD, B=0, C=6), None) == -1


# ---- the wrappers' argument contract, on CPU tensors -------------------------------------------------------------------------------------------
def _cl(*shape):
    return torch.zeros(shape).contiguous(memory_format=torch.channels_last)


def test_device_check_is_there_and_comes_last():
    with pytest.raises(IsxError, match="CUDA"):
        alex.conv2d_nhwc(_cl(1, 4, 5, 5), torch.zeros(32, 3, 3, 4), torch.zeros(32), 1, 1)
    with pytest.raises(IsxError, match="CUDA"):
        alex.maxpool3s2(_cl(1, 4, 5, 5))


CONV_BAD = [
    ("x", dict(x=lambda: torch.zeros(1, 4, 5, 5))),                               # NCHW memory
    ("x", dict(x=lambda: _cl(1, 4, 5, 5).double())),
    ("x", dict(x=lambda: torch.zeros(4, 5, 5))),
    ("x", dict(x=lambda: _cl(1, 4, 2, 5), pad=0)),                                # no output
    ("w_ohwi", dict(w=lambda: torch.zeros(32, 3, 3, 8))),                         # Cin of x is 4
    ("w_ohwi", dict(w=lambda: torch.zeros(32, 3, 2, 4))),
    ("w_ohwi", dict(w=lambda: torch.zeros(48, 3, 3, 4))),
    ("w_ohwi", dict(w=lambda: torch.zeros(32, 17, 17, 4))),
    ("w_ohwi", dict(w=lambda: torch.zeros(32, 3, 3, 4, dtype=torch.float16))),
    ("bias", dict(bias=lambda: torch.zeros(31))),
    ("stride", dict(stride=0)),
    ("stride", dict(stride=5)),
    ("stride", dict(pad=3)),
    ("stride", dict(pad=-1)),
]


@pytest.mark.parametrize("named,override", CONV_BAD, ids=["%s-%d" % (n, i) for i, (n, _) in enumerate(CONV_BAD)])
def test_one_wrong_conv_argument_is_named(named, override):
    kw = dict(dict(x=lambda: _cl(1, 4, 5, 5), w=lambda: torch.zeros(32, 3, 3, 4), bias=lambda: torch.zeros(32), stride=1, pad=1), **override)
    kw = {k: v() if callable(v) else v for k, v in kw.items()}
    with pytest.raises(IsxError, match=r"^%s(=| has | must )" % named) as e:
        alex.conv2d_nhwc(kw["x"], kw["w"], kw["bias"], kw["stride"], kw["pad"], True)
    assert "CUDA" not in str(e.value)


@pytest.mark.parametrize("x", [lambda: torch.zeros(1, 4, 5, 5), lambda: _cl(1, 6, 5, 5), lambda: _cl(1, 4, 2, 5), lambda: _cl(1, 4, 5, 5).int()])
def test_one_wrong_pool_argument_is_named(x):
    with pytest.raises(IsxError, match=r"^x (has|must) ") as e:
        alex.maxpool3s2(x())
    assert "CUDA" not in str(e.value)
