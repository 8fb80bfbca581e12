"""What tests/test_ops_contract.py cannot show without a GPU: a call isx/ops.py refuses has launched nothing (the caller's buffers keep every
bit), and a correct out= / ws= gives the bits of the same call without them.  Every call here is refused on the host or is valid."""
import pytest
import torch

from isx import ops
from isx._lib import IsxError

pytestmark = pytest.mark.gpu

M, N, D, B, C, H, W, L = 3, 5, 8, 2, 4, 3, 3, 3
BITS = {1: (torch.uint8, 0xA5), 4: (torch.int32, 0x7FC0BEEF), 8: (torch.int64, 0x7FF8DEADBEEF0001)}     # NaNs no kernel here writes


def bits(t):
    return t.view(BITS[t.element_size()][0])


def poisoned(shape, dtype=torch.float32):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    bits(t).fill_(BITS[t.element_size()][1])
    return t


def untouched(*bases):
    torch.cuda.synchronize()
    return all(bool((bits(t) == BITS[t.element_size()][1]).all()) for t in bases)


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    return dict(Q=r(M, D), G=r(N, D), x=r(B, C), rows=r(L, D), fmap=r(B, C, H, W), Gk=r(300, D))


# wrapper -> (call with out, shape of out)
WITH_OUT = {
    "cosine_sim": (lambda d, out: ops.cosine_sim(d["Q"], d["G"], out=out), (M, N)),
    "gap_l2": (lambda d, out: ops.gap_l2(d["fmap"], out=out), (B, C)),
    "gap_l2_nhwc": (lambda d, out: ops.gap_l2(d["fmap"].contiguous(memory_format=torch.channels_last), out=out), (B, C)),
    "l2norm_rows": (lambda d, out: ops.l2norm_rows(d["x"], out=out), (B, C)),
    "tree_sum_rows": (lambda d, out: ops.tree_sum_rows(d["rows"], out=out), (D,)),
}


def bad_outs(shape):
    """(out, the allocation it lives in): one row short, float64, a strided view."""
    short = poisoned((shape[0] - 1,) + shape[1:])
    wide = poisoned(shape, torch.float64)
    base = poisoned(shape[:-1] + (2 * shape[-1],))
    return [(short, short), (wide, wide), (base[..., ::2], base)]


@pytest.mark.parametrize("wrapper", sorted(WITH_OUT))
def test_refused_out_is_not_written(data, wrapper):
    fn, shape = WITH_OUT[wrapper]
    for out, base in bad_outs(shape):
        assert tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous()
        with pytest.raises(IsxError, match="^out "):
            fn(data, out)
        assert untouched(base), (wrapper, tuple(out.shape), out.dtype, out.stride())


@pytest.mark.parametrize("fast", [False, True])
def test_refused_topk_buffers_are_not_written(data, fast):
    k = 2
    fn = ops.cosine_topk_fast if fast else ops.cosine_topk
    nbytes = (ops.cosine_topk_fast_workspace if fast else ops.cosine_topk_workspace)(M, 300, D, k)
    ws32, ts, ti = poisoned((nbytes,)), poisoned((M, k)), poisoned((M, k), torch.int64)          # 4x the bytes asked for, but float32
    with pytest.raises(IsxError, match="^ws must be torch.uint8"):
        fn(data["Q"], data["Gk"], k, ws=ws32, out=(ts, ti))
    assert untouched(ws32, ts, ti)
    ws, short_s, short_i = poisoned((nbytes,), torch.uint8), poisoned((M - 1, k)), poisoned((M - 1, k), torch.int64)
    for pair, named in (((short_s, ti), r"^out\[0\] has shape"), ((ts, short_i), r"^out\[1\] has shape")):
        with pytest.raises(IsxError, match=named):
            fn(data["Q"], data["Gk"], k, ws=ws, out=pair)
        assert untouched(ws, ts, ti, short_s, short_i)


def test_out_on_another_device_is_refused(data):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second GPU: every tensor here would be on the current device")
    out = torch.full((M, N), 3.0, device="cuda:1")
    with pytest.raises(IsxError, match="^out lives on cuda:1"):
        ops.cosine_sim(data["Q"], data["G"], out=out)
    assert bool((out == 3.0).all())


@pytest.mark.parametrize("wrapper", sorted(WITH_OUT))
def test_out_gives_the_bits_of_the_call_without(data, wrapper):
    fn, shape = WITH_OUT[wrapper]
    out = poisoned(shape)
    got, ref = fn(data, out), fn(data, None)
    assert got is out and ref.dtype == out.dtype and ref.shape == out.shape and ref.stride() == out.stride()
    assert torch.equal(bits(out), bits(ref))


@pytest.mark.parametrize("fast", [False, True])
def test_topk_ws_and_out_give_the_bits_of_the_call_without(data, fast):
    k = 2
    fn = ops.cosine_topk_fast if fast else ops.cosine_topk
    nbytes = (ops.cosine_topk_fast_workspace if fast else ops.cosine_topk_workspace)(M, 300, D, k)
    ws, ts, ti = poisoned((nbytes,), torch.uint8), poisoned((M, k)), poisoned((M, k), torch.int64)
    got = fn(data["Q"], data["Gk"], k, idx_base=11, ws=ws, out=(ts, ti))
    ref = fn(data["Q"], data["Gk"], k, idx_base=11)
    assert got[0] is ts and got[1] is ti
    assert torch.equal(bits(ts), bits(ref[0])) and torch.equal(ti, ref[1]) and ref[1].dtype == torch.int64
    assert int(ti.min()) >= 11 and int(ti.max()) < 311
