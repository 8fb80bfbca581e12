"""libisxalex.so (csrc/alex.hip) on the GPU: isxa_conv2d_nhwc and isxa_maxpool3s2_nhwc bit for bit against tests/_alex_model.py between guards, at the
shapes of _alex_model.CONV_CASES / POOL_CASES (every tile shape, both operand gathers, aligned and ragged weight rows); batch independence; behind a
late producer on a side stream and captured into a HIP graph (tests/_streams.py, as tests/test_gpu_prep.py runs its cases); one output past 2^31
elements per entry; every refusal of the header with nothing launched; and the AlexNet / Maxnet `features` trunks through model.nn_utils under
ISX_ALEX = 1 and 0.

Every call here is valid or refused on the host: every pointer is a live buffer of the size the shape says."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as Fn

import _alex_model as A
import _guards as G
import _streams as S
from isx import alex, ops
from isx._lib import IsxError

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 4096


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _conv_regions(x, w, bias, out_shape):
    return G.in_f32(x, GUARD), G.in_f32(w, GUARD), G.in_f32(bias, GUARD), G.out_f32(out_shape, GUARD)


def _conv_call(xr, wr, br, yr, case, relu, stream=None):
    B, H, W, Cin, Cout, K, stride, pad = case
    L = alex.lib()
    rc = L.isxa_conv2d_nhwc(xr.ptr, B, H, W, Cin, wr.ptr, Cout, K, stride, pad, br.ptr, 1 if relu else 0, yr.ptr, _stream() if stream is None else stream)
    assert rc == 0, (rc, L.isxa_last_error())


# ---- the kernels against the model -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(A.CONV_CASES))
def test_conv_bit_for_bit(name):
    case = A.CONV_CASES[name]
    x, w, bias, want = A.conv_case(name)
    regs = _conv_regions(x, w, bias, want.shape)
    _conv_call(*regs, case, True)
    G.assert_clean([regs[3]], regs[:3], name)
    G.assert_bits(regs[3], want, name)
    first = regs[3].raw().clone()
    _conv_call(*regs, case, True)                                           # two launches agree in every bit; the call overwrites
    G.assert_clean([regs[3]], regs[:3], name + " (second launch)")
    assert torch.equal(regs[3].raw(), first)
    if name.startswith("3x3s") and case[3] % 32 == 0:                       # the layers both libraries take: the same bits from either
        xt = regs[0].body.permute(0, 3, 1, 2)
        y = ops.conv3x3_nhwc(xt, regs[1].body, regs[2].body, case[6], None, True)
        G.assert_bits(y.permute(0, 2, 3, 1).contiguous(), want, name + " (isx_conv3x3_nhwc)")


@pytest.mark.parametrize("name", ["11x11s4_3to64", "5x5_64to192", "1x1_4to64"])
def test_conv_without_relu(name):
    case = A.CONV_CASES[name]
    x, w, bias, want = A.conv_case(name, False)
    assert (want < 0).any()
    regs = _conv_regions(x, w, bias, want.shape)
    _conv_call(*regs, case, False)
    G.assert_clean([regs[3]], regs[:3], name)
    G.assert_bits(regs[3], want, name)


def test_conv_nan_goes_to_zero_under_relu_and_through_without():
    """The epilogue is isx_conv3x3_nhwc's: fmaxf(y, 0)."""
    name = "1x1_4to64"
    case = A.CONV_CASES[name]
    x, w, bias = (np.array(a) for a in A.conv_inputs(name))
    x[0, 0, 0, 0] = np.nan
    x[1, 2, 3, 1] = np.inf
    for relu in (True, False):
        with np.errstate(invalid="ignore"):
            want = A.conv2d(x, w, bias, case[6], case[7], relu)
        assert np.isnan(want).any() != relu
        regs = _conv_regions(x, w, bias, want.shape)
        _conv_call(*regs, case, relu)
        G.assert_clean([regs[3]], regs[:3], name)
        got = regs[3].host()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        keep = ~np.isnan(want)
        assert np.array_equal(G.bits(got)[keep], G.bits(want)[keep])


@pytest.mark.parametrize("shape", A.POOL_CASES, ids=lambda s: "x".join(map(str, s)))
def test_pool_bit_for_bit(shape):
    x, want = A.pool_case(shape)
    xr, yr = G.in_f32(x, GUARD), G.out_f32(want.shape, GUARD)
    L = alex.lib()
    for what in ("first launch", "second launch"):
        rc = L.isxa_maxpool3s2_nhwc(xr.ptr, shape[0], shape[1], shape[2], shape[3], yr.ptr, _stream())
        assert rc == 0, (rc, L.isxa_last_error())
        assert xr.guards_intact() and yr.guards_intact(), what
        G.assert_bits(yr, want, (shape, what))                              # (a NaN of the input is a legitimate result: the bits decide, not the poison count)
    got = alex.maxpool3s2(xr.body.permute(0, 3, 1, 2))
    assert got.is_contiguous(memory_format=torch.channels_last)
    G.assert_bits(got.permute(0, 2, 3, 1).contiguous(), want, shape)
    torch_gpu = Fn.max_pool2d(xr.body.permute(0, 3, 1, 2), 3, 2)
    G.assert_bits(torch_gpu.permute(0, 2, 3, 1).contiguous(), want, (shape, "torch on the GPU"))


# ---- batch independence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["11x11s4_3to64", "5x5_64to192", "3x3s1_192to384"])
def test_an_image_does_not_depend_on_its_batch(name):
    _, H, W, Cin, Cout, K, stride, pad = A.CONV_CASES[name]
    g = torch.Generator().manual_seed(7)
    x = torch.randn(5, H, W, Cin, generator=g).cuda().permute(0, 3, 1, 2)
    w, bias = (torch.randn(Cout, K, K, Cin, generator=g) * (K * K * Cin) ** -0.5).cuda(), torch.randn(Cout, generator=g).cuda()
    y5 = alex.conv2d_nhwc(x, w, bias, stride, pad, True)
    y1 = alex.conv2d_nhwc(x[3:4].clone(memory_format=torch.channels_last), w, bias, stride, pad, True)     # (a buffer of its own: 16-byte aligned)
    assert y5.shape[0] == 5 and torch.equal(y5[3:4].view(torch.int32), y1.view(torch.int32))
    assert min(y1.shape[2:]) >= 3
    assert torch.equal(alex.maxpool3s2(y5)[3:4].view(torch.int32), alex.maxpool3s2(y1).view(torch.int32))


# ---- behind a late producer on a side stream, and captured into a HIP graph ---------------------------------------------------------------------
def _stream_cases():
    name = "5x5_64to192"
    B, H, W, Cin, Cout, K, stride, pad = A.CONV_CASES[name]
    x, w, bias, y = A.conv_case(name)
    conv_ref = lambda a: dict(y=y if a.x is x or np.array_equal(a.x, x) else A.conv2d(a.x, a.w, a.bias, stride, pad, True))
    conv_ins, conv_outs = dict(x=x, w=w, bias=bias), dict(y=("f32", y.shape))
    pshape = A.POOL_CASES[0]
    px, py = A.pool_case(pshape)
    pool_ref = lambda a: dict(y=A.maxpool3s2(a.x))
    pool_ins, pool_outs = dict(x=px), dict(y=("f32", py.shape))
    nchw = lambda t: t.permute(0, 3, 1, 2)
    nhwc = lambda t: t.permute(0, 2, 3, 1)
    return [
        ("conv2d abi", S.Case(conv_ins, lambda L, p, st: alex.lib().isxa_conv2d_nhwc(p.x, B, H, W, Cin, p.w, Cout, K, stride, pad, p.bias, 1, p.y, st), conv_ref,
                              outs=conv_outs, level="abi")),
        ("conv2d ops", S.Case(conv_ins, lambda r: dict(y=alex.conv2d_nhwc(nchw(r.x.body), r.w.body, r.bias.body, stride, pad, True)), conv_ref,
                              sample=dict(y=nhwc), level="ops")),
        ("maxpool3s2 abi", S.Case(pool_ins, lambda L, p, st: alex.lib().isxa_maxpool3s2_nhwc(p.x, pshape[0], pshape[1], pshape[2], pshape[3], p.y, st), pool_ref,
                                  outs=pool_outs, level="abi")),
        ("maxpool3s2 ops", S.Case(pool_ins, lambda r: dict(y=alex.maxpool3s2(nchw(r.x.body))), pool_ref, sample=dict(y=nhwc), level="ops")),
    ]


def test_behind_a_late_producer():
    cases = _stream_cases()
    slowest = max(c.run_plain() for _, c in cases)             # default stream, real operands: loads the kernels, measures the host side of a call
    cycles, _ = S.delay_cycles(slowest, S.sleep_cycles_per_second())
    for name, c in cases:
        took = c.run_late(cycles)
        print("%s: host call %.3f ms behind the late producer" % (name, took * 1e3))


def test_captured_into_a_graph_and_replayed():
    for name, c in _stream_cases():
        c.run_plain()
        c.run_captured()                                        # decoys, then the real operands over stale results, then over poison


# ---- outputs past 2^31 elements ----------------------------------------------------------------------------------------------------------------
def _need(nbytes):
    if torch.cuda.mem_get_info()[0] < nbytes:
        pytest.skip("needs %.0f GB of free device memory" % (nbytes / 2 ** 30))


def _tiled_randn(n, seed):
    """n standard normals on the device, a block of 2^24 + 3 values repeated: cheap to make, and its period divides no row length used here."""
    base = torch.randn((1 << 24) + 3, generator=torch.Generator().manual_seed(seed)).cuda()
    x = torch.empty(n, dtype=torch.float32, device="cuda")
    for lo in range(0, n, base.numel()):
        m = min(base.numel(), n - lo)
        x[lo:lo + m] = base[:m]
    return x


def _unwritten(y):
    flat, left = y.view(-1).view(torch.int32), 0
    for lo in range(0, flat.numel(), 1 << 28):
        left += int((flat[lo:lo + (1 << 28)] == G._signed(G.POISON_F32, torch.int32)).sum())
    return left


def test_conv_output_past_2_31_elements():
    """K = 1, Cin = 4, Cout = 64 on 4097 x 8192 pixels: 2^25 + 8192 rows of y, 2^31 + 2^19 elements, 128 x 64 tiles.  A 32-bit element index
    anywhere lands a row of the second half on one of the first."""
    H, W, Cin, Cout = 4097, 8192, 4, 64
    M = H * W
    assert M * Cout > 1 << 31
    _need((M * Cout + M * Cin) * 4 + (3 << 30))
    x = _tiled_randn(M * Cin, 11).view(1, H, W, Cin)
    g = torch.Generator().manual_seed(12)
    w, bias = (torch.randn(Cout, 1, 1, Cin, generator=g) * 0.5).cuda(), torch.randn(Cout, generator=g).cuda()
    y = torch.empty((1, H, W, Cout), dtype=torch.float32, device="cuda")
    y.view(torch.int32).fill_(G._signed(G.POISON_F32, torch.int32))
    L = alex.lib()
    rc = L.isxa_conv2d_nhwc(x.data_ptr(), 1, H, W, Cin, w.data_ptr(), Cout, 1, 1, 0, bias.data_ptr(), 0, y.data_ptr(), _stream())
    assert rc == 0, (rc, L.isxa_last_error())
    torch.cuda.synchronize()
    assert _unwritten(y) == 0
    rng = np.random.default_rng(13)
    rows = np.unique(np.r_[0, 1, 127, 128, (1 << 25) - 129, (1 << 25) - 1, 1 << 25, (1 << 25) + 1, M - 130, M - 2, M - 1, rng.integers(0, M, 4096)])
    at = torch.from_numpy(rows).cuda()
    xs = x.view(M, Cin)[at].cpu().numpy()
    want = A.conv2d(xs.reshape(1, 1, -1, Cin), w.cpu().numpy(), bias.cpu().numpy(), 1, 0, False).reshape(-1, Cout)
    G.assert_bits(y.view(M, Cout)[at].cpu().numpy(), want, "sampled rows")
    del x, y


def test_pool_output_past_2_31_elements():
    """C = 8 on 32771 x 32771 pixels: 16385 x 16385 x 8 = 2^31 + 262 152 elements of y from 8.6e9 of x."""
    H = W = 32771
    C = 8
    Ho = Wo = (H - 3) // 2 + 1
    assert Ho * Wo * C > 1 << 31
    _need((H * W * C + Ho * Wo * C) * 4 + (3 << 30))
    x = _tiled_randn(H * W * C, 21).view(1, H, W, C)
    y = torch.empty((1, Ho, Wo, C), dtype=torch.float32, device="cuda")
    y.view(torch.int32).fill_(G._signed(G.POISON_F32, torch.int32))
    L = alex.lib()
    rc = L.isxa_maxpool3s2_nhwc(x.data_ptr(), 1, H, W, C, y.data_ptr(), _stream())
    assert rc == 0, (rc, L.isxa_last_error())
    torch.cuda.synchronize()
    assert _unwritten(y) == 0
    rng = np.random.default_rng(23)
    P = Ho * Wo
    pix = np.unique(np.r_[0, 1, Wo - 1, Wo, (1 << 28) - 1, 1 << 28, (1 << 28) + 1, P - Wo, P - 2, P - 1, rng.integers(0, P, 4096)])
    ho, wo = pix // Wo, pix % Wo
    win = ((2 * ho[:, None, None] + np.arange(3)[None, :, None]) * W + (2 * wo[:, None, None] + np.arange(3)[None, None, :])).reshape(-1)     # (pixel, kh, kw)
    xs = x.view(H * W, C)[torch.from_numpy(win).cuda()].cpu().numpy().reshape(len(pix), 3, 3, C)
    want = A.maxpool3s2(xs).reshape(len(pix), C)
    G.assert_bits(y.view(P, C)[torch.from_numpy(pix).cuda()].cpu().numpy(), want, "sampled pixels")
    del x, y


# ---- a refused call launches nothing -----------------------------------------------------------------------------------------------------------
def test_refused_calls_launch_nothing():
    L = alex.lib()
    x = torch.randn(1, 5, 6, 8, device="cuda")                            # covers CONV_GOOD (Cin = 4) and POOL_GOOD (C = 8)
    w, bias = torch.randn(32, 3, 3, 4, device="cuda"), torch.randn(32, device="cuda")
    yr = G.out_f32((1, 5, 6, 32), GUARD)
    live = dict(x=x.data_ptr(), w=w.data_ptr(), bias=bias.data_ptr(), y=yr.ptr)
    for entry, good, cases in (("isxa_conv2d_nhwc", A.CONV_GOOD, A.CONV_REFUSALS), ("isxa_maxpool3s2_nhwc", A.POOL_GOOD, A.POOL_REFUSALS)):
        good = dict(good, **{k: v for k, v in live.items() if k in good})
        for text, kw in cases:
            assert A.call_abi(L, entry, dict(good, **kw), _stream()) == -1, (entry, kw)
            err = L.isxa_last_error()
            assert err.startswith(entry.encode() + b":") and text.encode() in err, (kw, err)
        torch.cuda.synchronize()
        assert yr.unwritten() == yr.n and yr.guards_intact(), entry
    # the wrappers refuse in Python, before the library is reached
    xt = x.permute(0, 3, 1, 2)
    for bad in (lambda: alex.conv2d_nhwc(xt[:, :4].contiguous(), w, bias, 1, 1), lambda: alex.conv2d_nhwc(xt, w, bias, 1, 1),
                lambda: alex.conv2d_nhwc(xt.cpu(), w, bias, 1, 1), lambda: alex.maxpool3s2(xt.contiguous()), lambda: alex.maxpool3s2(xt.cpu())):
        with pytest.raises(IsxError):
            bad()
    # a base pointer off its 16-byte boundary reaches the library through the wrapper and comes back as its refusal
    off = torch.randn(1 * 5 * 6 * 4 + 1, device="cuda")[1:].view(1, 5, 6, 4).permute(0, 3, 1, 2)
    with pytest.raises(IsxError, match="isxa_conv2d_nhwc: x, w_ohwi and y must be 16-B aligned"):
        alex.conv2d_nhwc(off, w, bias, 1, 1)
    # and the same buffers, given a call that is right, receive the result
    assert A.call_abi(L, "isxa_conv2d_nhwc", dict(A.CONV_GOOD, **live), _stream()) == 0
    G.assert_clean([yr])
    want = A.conv2d(x[..., :4].cpu().numpy(), w.cpu().numpy(), bias.cpu().numpy(), 1, 1, True)
    got = alex.conv2d_nhwc(x[..., :4].contiguous().permute(0, 3, 1, 2), w, bias, 1, 1, True)
    G.assert_bits(got.permute(0, 2, 3, 1).contiguous(), want)
    assert alex.conv2d_nhwc(xt[:0, :4].contiguous(memory_format=torch.channels_last), w, bias, 1, 1).shape == (0, 32, 5, 6)


# ---- the whole trunk through model.nn_utils ----------------------------------------------------------------------------------------------------
def _nets():
    from isx import backbones
    from model.ModelDefinition import Maxnet
    torch.manual_seed(3)
    return [("alexnet", backbones.alexnet(pretrained=True).eval()), ("Maxnet", Maxnet(17).eval())]


def _layers(features):
    out = []
    mods = list(features)
    for i, m in enumerate(mods):
        if isinstance(m, nn.Conv2d):
            relu = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            out.append(("conv", m.weight.detach().permute(0, 2, 3, 1).contiguous().numpy(), m.bias.detach().numpy(), m.stride[0], m.padding[0], relu))
        elif isinstance(m, nn.MaxPool2d):
            out.append(("pool",))
    return out


_IMAGES = {"2x67x99": (2, 67, 99), "1x224x224": (1, 224, 224)}


@pytest.mark.parametrize("images", list(_IMAGES))
def test_trunk_under_mode_1_is_the_model(images, monkeypatch):
    from model import nn_utils
    monkeypatch.setattr(nn_utils, "_ALEX_MODE", "1")
    B, H, W = _IMAGES[images]
    x = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(B))
    pools = []
    real_pool = Fn.max_pool2d
    monkeypatch.setattr(Fn, "max_pool2d", lambda *a, **k: (pools.append(1), real_pool(*a, **k))[1])
    for name, net in _nets():
        want = A.trunk(_layers(net.features), x.permute(0, 2, 3, 1).contiguous().numpy())
        f = nn_utils.fold_batch_norm(net.features).cuda()
        nn_utils.TORCH_CONV_CALLS.clear()
        with torch.no_grad():
            y = f(x.cuda())
            y_again = f(x.cuda())
        assert nn_utils.TORCH_CONV_CALLS == {} and pools == [], (name, nn_utils.TORCH_CONV_CALLS, len(pools))
        assert y.is_contiguous(memory_format=torch.channels_last)
        G.assert_bits(y.permute(0, 2, 3, 1).contiguous(), want, (name, images))
        assert torch.equal(y.view(torch.int32), y_again.view(torch.int32))
        if B > 1:                                                           # an image's map does not depend on the batch it rides in
            with torch.no_grad():
                alone = f(x[1:2].cuda())
            assert torch.equal(alone.view(torch.int32), y[1:2].view(torch.int32))


def test_trunk_under_mode_0_is_the_parent_route(monkeypatch):
    """ISX_ALEX = 0 folds to the modules themselves behind the channels-last entry, which is what the parent commit built.  Compared with torch's
    deterministic algorithm choice: MIOpen's default one is not run-to-run reproducible (tests/test_train_hooks.py)."""
    from model import nn_utils
    monkeypatch.setattr(nn_utils, "_ALEX_MODE", "0")
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    x = torch.randn(2, 3, 67, 99, generator=torch.Generator().manual_seed(2)).cuda()
    for name, net in _nets():
        f = nn_utils.fold_batch_norm(net.features).cuda()
        parent = nn.Sequential(nn_utils._ChannelsLastEntry(), *copy.deepcopy(list(net.features))).eval().cuda()
        assert [type(m) for m in f] == [type(m) for m in parent], name
        with torch.no_grad():
            a, b = f(x), parent(x)
        assert a.stride() == b.stride() and torch.equal(a, b), name


def test_default_mode_keeps_the_descriptor(monkeypatch):
    """Whatever kinds `auto` takes: the folded trunk's map stays within the cosine 1e-5 of the existing AlexNet tests of the plain modules'."""
    from model import nn_utils
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(5)).cuda()
    for mode in ("auto", "1"):
        monkeypatch.setattr(nn_utils, "_ALEX_MODE", mode)
        for name, net in _nets():
            f = nn_utils.fold_batch_norm(net.features).cuda()
            with torch.no_grad():
                a, b = f(x).flatten(1).double(), copy.deepcopy(net.features).cuda()(x).flatten(1).double()
            cos = Fn.cosine_similarity(a, b, dim=1)
            assert float((1 - cos).abs().max()) <= 1e-5, (mode, name, cos.tolist())
