"""isxs_resize_cubic_u8 (csrc/scale.hip, libisxscale.so) on the GPU: bit for bit against the integer model (tests/_resize_model.py) between
guards and into a poisoned dst, at the case table of the model file, at every byte alignment of src and dst, with padding and distinct noise
ids, across several column tiles and at the limits the entry accepts; behind a late producer on a side stream and captured into a graph
(tests/_streams.py, as tests/test_gpu_prep.py and tests/test_gpu_graph_capture.py run their cases); a refused call writes nothing; and the tool
end to end, device against host.

Every call here is valid or refused on the host: every pointer is a live buffer of the size the shapes say."""
import os

import numpy as np
import pytest
import torch

import _guards as G
import _resize_model as M
import _streams as S
from isx import scale
from isx._lib import IsxError

pytestmark = pytest.mark.gpu

GUARD = 4096                                                  # guard bytes around src and dst
OFFSETS = (0, 1, 2, 3, 13)


def _call(src, img_shape, pad, seed, ids, dst, size, stream=None):
    L = scale.lib()
    B, Hs, Ws = img_shape[:3]
    top, left, Hp, Wp = pad if pad is not None else (0, 0, Hs, Ws)
    rc = L.isxs_resize_cubic_u8(src, B, Hs, Ws, top, left, Hp, Wp, seed, ids, dst, size[0], size[1],
                                torch.cuda.current_stream().cuda_stream if stream is None else stream)
    assert rc == 0, (rc, L.isxs_last_error())


def _check(src_r, dst_r, want, what):
    torch.cuda.synchronize()
    assert src_r.guards_intact() and dst_r.guards_intact(), ("store outside dst (or into the guards of src)", what)
    got = dst_r.host()
    bad = got != want
    assert got.shape == want.shape and not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


def _run(img, size, want, what, pad=None, seed=0, ids=None, src_off=0, dst_off=0, twice=False):
    B = img.shape[0]
    src_r = G.Region("u8", img.shape, GUARD, src_off, data=np.array(img))       # a copy: the shared cases are read-only
    dst_r = G.Region("u8", (B, size[0], size[1], 3), GUARD, dst_off)              # poisoned
    ids_r = None if ids is None else G.in_i64(np.asarray(ids, np.int64))
    assert src_r.ptr % 256 == src_off and dst_r.ptr % 256 == dst_off
    _call(src_r.ptr, img.shape, pad, seed, G.ptr(ids_r), dst_r.ptr, size)
    _check(src_r, dst_r, want, what)
    if twice:                                                  # the call overwrites: a second call into the first result gives the same bits
        _call(src_r.ptr, img.shape, pad, seed, G.ptr(ids_r), dst_r.ptr, size)
        _check(src_r, dst_r, want, what + " (second call into the first result)")


@pytest.mark.parametrize("c", M.CASES, ids=[M.case_id(c) for c in M.CASES])
def test_case_table_bit_for_bit(c):
    for kind in M.KINDS:
        img, want = M.case(c, kind)
        _run(img, c[2:], want, "%s %s" % (M.case_id(c), kind), twice=(kind == "random"))


@pytest.mark.parametrize("c", [M.CASES[1], M.CASES[4], M.CASES[5]], ids=[M.case_id(c) for c in (M.CASES[1], M.CASES[4], M.CASES[5])])
def test_every_byte_alignment(c):
    """src and dst 0, 1, 2, 3 and 13 bytes past a 256-byte boundary, every pair: the rows of dst then start at every offset inside a 16-byte line."""
    img, want = M.case(c, "random")
    for so in OFFSETS:
        for do in OFFSETS:
            _run(img, c[2:], want, "%s src + %d dst + %d" % (M.case_id(c), so, do), src_off=so, dst_off=do)


# the pad cases of the model file and one whose footprint is not staged: 300 x 20 on a 300 x 150 canvas, brought to 8 x 4
GPU_PAD_CASES = [(c[0], c[1], c[3], c[4]) for c in M.PAD_CASES] + [(300, 20, (0, 65, 300, 150), (8, 4)), (20, 300, (65, 0, 150, 300), (150, 300))]


@pytest.mark.parametrize("Hs,Ws,pad,size", GPU_PAD_CASES, ids=["%dx%d" % (c[0], c[1]) for c in GPU_PAD_CASES])
def test_padding_three_images_three_noise_ids(Hs, Ws, pad, size):
    assert scale.aspect_pad(Hs, Ws, 2.0) == pad
    img = M.image("random", Hs, Ws, B=3)
    seed, ids = 0xDEADBEEFCAFE, [7, 0, 2 ** 41 + 3]
    want = M.resize(img, size, pad, seed, ids)
    assert not np.array_equal(want[0], M.resize(img[:1], size, pad, seed, [8])[0])                # the border is the noise id's
    for off in (0, 13):
        _run(img, size, want, "%dx%d padded to %dx%d, dst + %d" % (Hs, Ws, pad[2], pad[3], off), pad=pad, seed=seed, ids=ids, dst_off=off, twice=(off == 0))


def test_wide_rows_over_several_column_tiles():
    B, Hs, Ws, Hd, Wd = M.WIDE
    assert (3 * Wd) % 16 != 0 and Wd > 8 * 128
    img = M.image("random", Hs, Ws, B=B)
    want = M.resize(img, (Hd, Wd))
    for off in (0, 3):
        _run(img, (Hd, Wd), want, "wide, dst + %d" % off, src_off=off, dst_off=off, twice=(off == 0))


@pytest.mark.parametrize("shape,size", [((2, 1), (16384, 1)), ((1, 2), (1, 16384)), ((32768, 1), (3, 1)), ((1, 32768), (2, 5))],
                         ids=["Hd=16384", "Wd=16384", "Hp=32768", "Wp=32768"])
def test_accepted_limits(shape, size):
    img = M.image("random", shape[0], shape[1])
    _run(img, size, M.resize(img, size), "%s -> %s" % (shape, size))


# ---- behind a late producer on a side stream, and captured into a graph -----------------------------------------------------------------------------
def _stream_cases():
    Hs, Ws, _, pad, size = M.PAD_CASES[0]
    img, ids, seed = M.image("random", Hs, Ws, B=3), np.array([4, 9, 1], np.int64), 77
    top, left, Hp, Wp = pad
    ref = lambda a: dict(dst=M.resize(a.img, size, pad, seed, a.ids))
    outs = dict(dst=("u8", (3, size[0], size[1], 3)))
    abi = S.Case(dict(img=img, ids=ids), lambda L, p, st: scale.lib().isxs_resize_cubic_u8(p.img, 3, Hs, Ws, top, left, Hp, Wp, seed, p.ids, p.dst,
                                                                                            size[0], size[1], st), ref, outs=outs, level="abi")
    ops = S.Case(dict(img=img, ids=ids), lambda r: (scale.resize_cubic_u8(r.img.body, size, pad=pad, seed=seed, noise_ids=r.ids.body, out=r.dst.body),
                                                    None)[1], ref, outs=outs, level="ops")
    return [("abi", abi), ("ops", ops)]


def test_behind_a_late_producer():
    cases = _stream_cases()
    slowest = max(c.run_plain() for _, c in cases)             # default stream, real operands: loads the kernel, measures the host side of a call
    cycles, _ = S.delay_cycles(slowest, S.sleep_cycles_per_second())
    for name, c in cases:
        took = c.run_late(cycles)
        print("resize_cubic_u8 (%s): host call %.3f ms behind the late producer" % (name, took * 1e3))


def test_captured_and_replayed():
    """Captured on a fresh stream under decoys, then the one graph replayed on decoys, on the real operands over those leftovers (into its own
    earlier result) and on poisoned buffers (Case.run_captured)."""
    for name, c in _stream_cases():
        c.run_plain()
        c.run_captured()


# ---- a refused call writes nothing ------------------------------------------------------------------------------------------------------------------
def _untouched(t):
    torch.cuda.synchronize()
    return bool((t == G.POISON_U8).all())


def test_refused_call_does_not_write():
    img = torch.from_numpy(np.array(M.image("random", 6, 9, B=2))).cuda()
    ids = torch.tensor([1, 2], dtype=torch.int64, device="cuda")
    poisoned = lambda *shape: torch.full(shape, G.POISON_U8, dtype=torch.uint8, device="cuda")
    short, base = poisoned(1, 4, 5, 3), poisoned(2, 4, 10, 3)
    for out, whole in ((short, short), (base[:, :, ::2], base)):
        with pytest.raises(IsxError, match="^out "):
            scale.resize_cubic_u8(img, (4, 5), out=out)
        assert _untouched(whole), (tuple(out.shape), out.stride())
    good = poisoned(2, 4, 5, 3)
    wide = torch.zeros((2, 6, 9, 4), dtype=torch.uint8, device="cuda")
    for bad in (wide, img.float(), wide[..., :3], img.cpu()):
        with pytest.raises(IsxError, match="^img_u8 "):
            scale.resize_cubic_u8(bad, (4, 5), out=good)
        assert _untouched(good), (tuple(bad.shape), bad.dtype, bad.stride())
    for kw, text in ((dict(pad=(1, 0, 6, 9), noise_ids=ids), "^bad shape"), (dict(pad=(1, 0, 8, 9)), "^noise_ids "),
                     (dict(pad=(1, 0, 8, 9), noise_ids=ids.int()), "^noise_ids "), (dict(pad=(1, 0, 8, 9), noise_ids=ids.cpu()), "^noise_ids ")):
        with pytest.raises(IsxError, match=text):
            scale.resize_cubic_u8(img, (4, 5), out=good, **kw)
        assert _untouched(good), kw
    # at the C ABI: refused before any launch
    L = scale.lib()
    st = torch.cuda.current_stream().cuda_stream
    assert L.isxs_resize_cubic_u8(img.data_ptr(), 2, 6, 9, 3, 0, 8, 9, 0, ids.data_ptr(), good.data_ptr(), 4, 5, st) == -1          # top + Hs > Hp
    assert L.isxs_resize_cubic_u8(img.data_ptr(), 2, 6, 9, 1, 0, 8, 9, 0, None, good.data_ptr(), 4, 5, st) == -1                    # padded, no ids
    assert _untouched(good)
    # and the same buffer, given a call that is right, receives the result
    want = M.resize(img.cpu().numpy(), (4, 5), (1, 0, 8, 9), 5, [1, 2])
    assert scale.resize_cubic_u8(img, (4, 5), pad=(1, 0, 8, 9), seed=5, noise_ids=ids, out=good) is good
    assert np.array_equal(good.cpu().numpy(), want)
    assert np.array_equal(scale.resize_cubic_u8(img, (4, 5), pad=(1, 0, 8, 9), seed=5, noise_ids=ids).cpu().numpy(), want)


# ---- the tool, device against host ------------------------------------------------------------------------------------------------------------------
def test_tool_device_and_host_write_the_same_files(tmp_path, monkeypatch):
    from PIL import Image
    import pre_process_dataset
    from test._common import load_sets
    from train._common import _raw_u8_set
    monkeypatch.setenv("ISX_DECODE_PROCS", "2")
    test_set, ref_set = load_sets("synthetic:CLICIDE_video_224sq:n=40:q=4:labels=4:size=48", [])
    folder = tmp_path / "synthetic_48"
    (folder / "test").mkdir(parents=True)
    sources = {}
    for where, items in (("", _raw_u8_set(ref_set)), ("test", _raw_u8_set(test_set))):
        for i, (im, _, _) in enumerate(items):
            a = im.numpy()
            a = a[:20] if i % 7 == 3 else a[:, :36] if i % 7 == 5 else a          # ragged: 20 x 48 is beyond the ratio and gets padded
            name = os.path.join(where, "im-%03d.%s" % (i, "jpg" if i % 2 else "png"))
            Image.fromarray(np.ascontiguousarray(a)).save(str(folder / name), quality=95)
            sources[name] = a.shape[:2]
    assert len(sources) == 44
    # the pixels before encoding: a run of each shape through both routes
    for H, W in sorted(set(sources.values())):
        run = [torch.from_numpy(np.array(M.image("random", H, W, salt=k)[0])) for k in range(3)]
        on_dev = pre_process_dataset.resize_run(run, [5, 6, 7], 2.0, 32, None, 0, 3)
        on_host = pre_process_dataset.resize_run(run, [5, 6, 7], 2.0, 32, None, -1, 3)
        assert on_dev.dtype == torch.uint8 and not on_dev.is_cuda and torch.equal(on_dev, on_host), (H, W)
    dev, host = tmp_path / "dev", tmp_path / "host"
    try:
        pre_process_dataset.main(["--dataset=" + str(folder), "--out=" + str(dev), "--short-side=32", "--device=0", "--batch=16", "--seed=3"])
        pre_process_dataset.main(["--dataset=" + str(folder), "--out=" + str(host), "--short-side=32", "--device=-1", "--seed=3"])
    finally:
        from train import _decode_farm
        _decode_farm.shutdown()
    for name, (H, W) in sources.items():
        a, b = open(str(dev / name), "rb").read(), open(str(host / name), "rb").read()
        assert a == b and len(a) > 0, name
        pad = scale.aspect_pad(H, W, 2.0)
        want = scale.short_side_size(pad[2], pad[3], 32)
        with Image.open(str(dev / name)) as im:
            assert im.size == (want[1], want[0]), name
        if name.endswith(".png"):                              # lossless: the decoded output is the model's
            src = np.asarray(Image.open(str(folder / name)).convert("RGB"))
            i = sorted(n for n in sources if os.path.dirname(n) == os.path.dirname(name)).index(name)
            got = np.asarray(Image.open(str(dev / name)).convert("RGB"))
            assert np.array_equal(got, M.resize(src[None], want, pad, 3, [i])[0]), name
