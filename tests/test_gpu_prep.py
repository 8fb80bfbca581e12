"""isxp_channel_moments_u8 (csrc/prep.hip, libisxprep.so) on the GPU: bit for bit against integer numpy between guards, at the shapes of
tests/_mean_std_model.KERNEL_CASES and at the limits of what the entry accepts; behind a late producer on a side stream (tests/_streams.py, run
as tests/test_gpu_stream_order.py runs its cases); a refused call launches nothing (the style of tests/test_gpu_ops_contract.py); and the tool
end to end, device against host.

Every call here is valid or refused on the host: every pointer is a live buffer of the size the shape says."""
import os

import numpy as np
import pytest
import torch

import _guards as G
import _mean_std_model as M
import _streams as S
from isx import prep
from isx._lib import IsxError

pytestmark = pytest.mark.gpu

GUARD = 4096                                                  # guard bytes around the image, guard elements around the moments


def _call(img_ptr, B, H, W, mom_ptr, stream=None):
    L = prep.lib()
    rc = L.isxp_channel_moments_u8(img_ptr, B, H, W, mom_ptr, torch.cuda.current_stream().cuda_stream if stream is None else stream)
    assert rc == 0, (rc, L.isxp_last_error())


def _regions(img, offset=0):
    """The image between guards of a byte its sums do not contain, the moments poisoned between guards."""
    return G.Region("u8", img.shape, GUARD, offset, data=img), G.Region("i64", (img.shape[0], 3, 2), GUARD)


def _check(img_r, mom_r, want, what):
    G.assert_clean([mom_r], [img_r], what)
    G.assert_bits(mom_r, want, what)


@pytest.mark.parametrize("cid,shape,offset", [(c[0], c[1], c[2]) for c in M.KERNEL_CASES], ids=[c[0] for c in M.KERNEL_CASES])
def test_moments_bit_for_bit(cid, shape, offset):
    img = M.kernel_image(cid)
    B, H, W = shape
    want = M.moments(img)
    if cid.startswith("1x258x257"):
        assert want[0, 0, 1] == 4311547650 > 1 << 32
    img_r, mom_r = _regions(img, offset)
    assert img_r.ptr % 256 == offset
    _call(img_r.ptr, B, H, W, mom_r.ptr)
    _check(img_r, mom_r, want, cid)
    # the call overwrites: a second call into the first result gives the same bits
    _call(img_r.ptr, B, H, W, mom_r.ptr)
    _check(img_r, mom_r, want, cid + " (second call into the first result)")


def test_most_images_of_one_pixel():
    B = 65535
    img = np.random.default_rng(65535).integers(0, 256, (B, 1, 1, 3), dtype=np.uint8)
    img_r, mom_r = _regions(img)
    _call(img_r.ptr, B, 1, 1, mom_r.ptr)
    _check(img_r, mom_r, M.moments(img), "65535 x 1 x 1")


def test_largest_accepted_image():
    """3 H W = 2 146 687 500 < 2^31, every byte 0xFF: the sums are closed forms, and a 32-bit partial anywhere wraps (per thread, per workgroup or
    in the output: 65025 H W = 4.65e13)."""
    H = W = 26750
    assert 3 * H * W == 2146687500 < 1 << 31
    if torch.cuda.mem_get_info()[0] < 3 << 30:
        pytest.skip("needs 3 GB of free device memory")
    img = torch.full((1, H, W, 3), 255, dtype=torch.uint8, device="cuda")
    mom = torch.full((1, 3, 2), G.POISON_I64, dtype=torch.int64, device="cuda")
    _call(img.data_ptr(), 1, H, W, mom.data_ptr())
    torch.cuda.synchronize()
    assert mom.cpu().tolist() == [[[255 * H * W, 65025 * H * W]] * 3]
    del img


# ---- behind a late producer on a side stream -------------------------------------------------------------------------------------------------------
def _stream_cases():
    img = M.kernel_image("3x5x7_misaligned_images")
    ref = lambda a: dict(moments=M.moments(a.img))
    outs = dict(moments=("i64", (3, 3, 2)))
    abi = S.Case(dict(img=img), lambda L, p, st: prep.lib().isxp_channel_moments_u8(p.img, 3, 5, 7, p.moments, st), ref, outs=outs, level="abi")
    ops = S.Case(dict(img=img), lambda r: (prep.channel_moments_u8(r.img.body, out=r.moments.body), None)[1], ref, outs=outs, level="ops")
    return [("abi", abi), ("ops", ops)]


def test_behind_a_late_producer():
    cases = _stream_cases()
    slowest = max(c.run_plain() for _, c in cases)             # default stream, real operands: loads the kernel, measures the host side of a call
    cycles, _ = S.delay_cycles(slowest, S.sleep_cycles_per_second())
    for name, c in cases:
        took = c.run_late(cycles)
        print("channel_moments_u8 (%s): host call %.3f ms behind the late producer" % (name, took * 1e3))


# ---- a refused call launches nothing ----------------------------------------------------------------------------------------------------------------
POISON = 0x7FF8DEADBEEF0001


def _poisoned(shape, dtype=torch.int64):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(torch.int64 if t.element_size() == 8 else torch.int32).fill_(POISON if t.element_size() == 8 else 0x7FC0BEEF)
    return t


def _untouched(t):
    torch.cuda.synchronize()
    return bool((t.view(torch.int64) == POISON).all()) if t.element_size() == 8 else bool((t.view(torch.int32) == 0x7FC0BEEF).all())


def test_refused_call_does_not_write():
    B, H, W = 2, 5, 7
    img = torch.from_numpy(M.kernel_image("3x5x7_misaligned_images")[:B]).cuda()
    short, narrow, base = _poisoned((B - 1, 3, 2)), _poisoned((B, 3, 2), torch.int32), _poisoned((B, 3, 4))
    for out, whole in ((short, short), (narrow, narrow), (base[:, :, ::2], base)):
        with pytest.raises(IsxError, match="^out "):
            prep.channel_moments_u8(img, out=out)
        assert _untouched(whole), (tuple(out.shape), out.dtype, out.stride())
    good = _poisoned((B, 3, 2))
    wide = torch.zeros((B, H, W, 4), dtype=torch.uint8, device="cuda")
    for bad in (wide, img.float(), wide[..., :3], img.cpu()):
        with pytest.raises(IsxError, match="^img_u8 "):
            prep.channel_moments_u8(bad, out=good)
        assert _untouched(good), (tuple(bad.shape), bad.dtype, bad.stride())
    # and the same buffer, given a call that is right, receives the result
    assert prep.channel_moments_u8(img, out=good) is good
    assert np.array_equal(good.cpu().numpy(), M.moments(img.cpu().numpy()))
    assert np.array_equal(prep.channel_moments_u8(img).cpu().numpy(), good.cpu().numpy())


# ---- the tool, device against host ------------------------------------------------------------------------------------------------------------------
def test_tool_device_and_host_write_the_same_bytes(tmp_path):
    import create_mean_std_file
    from isx import ops
    from utils.general import read_mean_std
    spec = "synthetic:CLICIDE_video_224sq:n=40:q=4:labels=4:size=48"
    dev, host = str(tmp_path / "dev.txt"), str(tmp_path / "host.txt")
    create_mean_std_file.main(["--dataset=" + spec, "--device=0", "--batch=16", "--out=" + dev])
    create_mean_std_file.main(["--dataset=" + spec, "--device=-1", "--out=" + host])
    assert open(dev, "rb").read() == open(host, "rb").read() and os.path.getsize(dev) > 0
    mean, std = read_mean_std(dev)
    assert len(mean) == len(std) == 3 and all(0.0 < m < 1.0 for m in mean) and all(0.0 < s < 1.0 for s in std)
    x = ops.images_u8_to_f32(torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device="cuda"), mean, std)
    torch.cuda.synchronize()
    assert tuple(x.shape) == (1, 3, 4, 4) and bool(torch.isfinite(x).all())
