"""Every launching entry of include/isx.h CAPTURED into a HIP graph and replayed, and called from four host threads on four streams.

include/isx.h opens with a contract every entry inherits: a call "only ENQUEUES work on `stream` ... no allocation, no synchronisation, no global
state ... safe to capture in a hipGraph and re-entrant from several host threads on distinct streams"; include/isx_prep.h repeats it for
isxp_channel_moments_u8.  tests/test_gpu_stream_order.py holds the first half (stream order).  This file runs the SAME table -- its cases, its
decoys, its guarded Regions, its CPU references and its comparisons; no new shape, reference or tolerance -- in two more ways:

  * Case.run_captured (tests/_streams.py): the call is captured on a fresh stream under decoys (an allocation, a synchronisation or a pageable
    copy inside the entry breaks the capture; a call that executes instead of being recorded shows in the poison), then the ONE graph is replayed on
    decoys, on boosted operands, on the real operands over those leftovers (carry lists of better keys, thresholds of a higher-scoring gallery,
    a non-zero fallback counter, accumulated moments: every replay of a graph meets such state) and on freshly poisoned buffers.  A host-side value
    baked into a launch, a memset a replay does not repeat or a result that depends on what a workspace held gives wrong bits.
  * test_four_host_threads_on_four_streams: the thread-local error string and the launch paths under four threads at once.

The capture is of one stream: every graph is a linear chain.  Nothing here sets an environment variable."""
import threading
import time
import types

import numpy as np
import pytest
import torch

import _guards as G
import _streams as S
import test_gpu_stream_order as so

gpu = pytest.mark.gpu
FIVE = ("ops_gap_l2", "ops_cosine_sim", "ops_search_sequence", "ops_cosine_topk_ws", "ops_suffix_conv1x1")     # wrapper rows that MUST run captured

# wrapper rows that cannot be captured as they stand: the host-side step that prevents it -- (a) a pinned host allocation or a host-array operand
# copied per call, (b) a host read of a device value or an event query that steers a later call, (c) a Python object whose first call differs from
# its later ones -- and the line that does it
NOT_CAPTURED = {
    "ops_affine_noisy_host_parameters":
        "(a) host-array operands copied per call: the case hands rows / mats / noise ids as numpy arrays (tests/test_gpu_stream_order.py:1081) and "
        "ops.affine_noisy packs them into a pinned host allocation per call (isx/ops.py:297 torch.cat(parts).pin_memory()); a replay would repeat "
        "the copy from a block that is gone.  The case also drops ops._MEAN_STD first, so the constant is a second pinned allocation (isx/ops.py:268)",
    "ops_sharded_gallery_local_search_twice":
        "(b) an event query that steers a later call: ShardedGallery._check_fallback (isx/retrieval.py:231-233) queries the event behind the "
        "asynchronous read of the fallback counter and reads the pinned host word (allocated at isx/retrieval.py:256) to decide whether the NEXT "
        "search takes the fp16 path; the second search of the case (tests/test_gpu_stream_order.py:1161) depends on it",
    "ops_shard_head_sgd_update_rows":
        "(c) a Python object whose first call differs from its later ones: the case builds a torch.optim.SGD inside the call "
        "(tests/test_gpu_stream_order.py:1137) and shard_head.sgd_update_rows creates the momentum buffer in its state on the first call and passes "
        "first = 1 to the kernel (isx/shard_head.py:206-208, :215); a replay would repeat a FIRST step",
}

PREP = "prep_channel_moments_u8"                  # the "abi" case of tests/test_gpu_prep.py::_stream_cases(): isxp_channel_moments_u8 of libisxprep


def _prep_case():
    import test_gpu_prep
    return dict(test_gpu_prep._stream_cases())["abi"]


CASES = [(i, b) for i, _, b in so.TABLE if i not in NOT_CAPTURED] + [(PREP, _prep_case)]
ABI_IDS = [i for i, e, _ in so.TABLE if e.startswith("isx_") and not i.startswith("ops_")]


def test_every_case_is_captured_or_excused():
    ids = [i for i, _ in CASES]
    assert len(ids) == len(set(ids)) and PREP in ids
    wrappers = {i for i, _, _ in so.TABLE if i.startswith("ops_")}
    assert len(ABI_IDS) >= 70 and set(ABI_IDS) | wrappers == {i for i, _, _ in so.TABLE} and not set(ABI_IDS) & wrappers
    for i, _, _ in so.TABLE:
        assert (i in ids) != (i in NOT_CAPTURED), ("a row of the table is captured or has a reason, not both and not neither", i)
    assert set(ABI_IDS) <= set(ids), "no C-ABI row may be left out"
    assert set(NOT_CAPTURED) <= wrappers, "only wrapper rows can be excused"
    assert not set(NOT_CAPTURED) & set(FIVE) and set(FIVE) <= set(ids)
    for i, reason in NOT_CAPTURED.items():
        assert isinstance(reason, str) and len(reason) > 20 and reason[:3] in ("(a)", "(b)", "(c)") and ".py:" in reason, i


def test_no_entry_zeroes_with_a_memset_node():
    """What this file found: a hipMemsetAsync captured into a graph zeroes on the first replay and fills with stale bits on every later one (ROCm 7.0),
    so isxp_channel_moments_u8 accumulated onto garbage from the second replay on, and the carry / statistics memsets of the search entries were
    right only because the garbage happened to rank below every real key.  The library zeroes with kernels (zero_words_async, csrc/cosine.hip)."""
    import glob
    import os
    import re
    src = sorted(glob.glob(os.path.join(so.ROOT, "instance-search_amd", "csrc", "*.*")))
    src = [p for p in src if p.endswith((".hip", ".cpp", ".hpp"))]
    assert len(src) > 20
    for p in src:
        code = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(p).read(), flags=re.S)
        assert not re.search(r"\bhipMemset\w*\s*\(", code), (os.path.basename(p), "zero with isx::zero_words_async: a memset node replays wrongly")


# ---- the pass --------------------------------------------------------------------------------------------------------------------------------------
_BUILT = {}
_PLAIN_FAILED = {}
_ABORTED = []                                      # the first exception that was not an assertion: nothing more is launched by this file


def _built(cid):
    if cid not in _BUILT:
        _BUILT[cid] = next(b for i, b in CASES if i == cid)()
    return _BUILT[cid]


def _launching(what):
    assert not _ABORTED, "nothing more is launched: %s aborted the pass of this file (%r)" % _ABORTED[0]
    return what


def _guarded(cid, fn):
    """The failure handling of the stream-order file's `delay` fixture: an AssertionError fails the case and the pass goes on; any other exception
    may be the device's -- it fails this case and every later one, and nothing more is launched."""
    _launching(cid)
    try:
        return fn()
    except AssertionError:
        raise
    except Exception as e:
        _ABORTED.append((cid, e))
        raise


@pytest.fixture(scope="module")
def plain():
    """Every case once on the default stream with its real operands (Case.run_plain): loads the code objects, so that nothing is loaded inside a
    capture, and shows a case that is wrong already."""
    t0 = time.perf_counter()
    for cid, _ in CASES:
        if _ABORTED:
            break
        try:
            _built(cid).run_plain()
        except AssertionError as e:
            _PLAIN_FAILED[cid] = e
        except Exception as e:
            _PLAIN_FAILED[cid] = e
            _ABORTED.append((cid + " (default-stream pass)", e))
    print("graph capture: default-stream pass of %d cases %.1f s" % (len(CASES), time.perf_counter() - t0))
    yield
    _BUILT.clear()
    _PLAIN_FAILED.clear()


@gpu
@pytest.mark.parametrize("cid", [i for i, _ in CASES])
def test_captured_and_replayed(cid, plain):
    if cid in _PLAIN_FAILED:
        raise AssertionError("the case fails on the default stream already: %r" % (_PLAIN_FAILED[cid],)) from _PLAIN_FAILED[cid]
    c = _built(cid)
    t0 = time.perf_counter()
    _guarded(cid, c.run_captured)
    print("%s: captured and replayed in %.3f s" % (cid, time.perf_counter() - t0))


# ---- the trunk pass of tools/graph_lab.py, small -------------------------------------------------------------------------------------------------
@gpu
def test_trunk_pass_replayed():
    """ResNet-50 features (every fused trunk kernel: stem, the fused bottlenecks of the four layers, the dual projections) -> ops.gap_l2(out=) on two
    channels-last images of 64 x 64, captured with batch A in `img`: a replay gives eager's bits for A, and for B once B has been copied into `img`.
    The eager path is pinned to the oracle elsewhere; this pins replay to eager."""
    from bench_legs.common import build_net
    from isx import ops
    _launching("the trunk pass")
    dev = torch.device("cuda", torch.cuda.current_device())
    net = build_net("resnet50", "f32", dev, channels_last=True, fold_bn=True)
    gen = torch.Generator().manual_seed(16)
    A, B = (torch.randn((2, 3, 64, 64), generator=gen).to(dev).contiguous(memory_format=torch.channels_last) for _ in range(2))
    img = torch.empty_like(A)
    out = torch.empty((2, 2048), device=dev)

    def forward():
        with torch.no_grad():
            ops.gap_l2(net.features(img), out=out)

    def run():
        eager = []
        for batch in (A, B):                                                 # the first pass builds the derived weights
            img.copy_(batch)
            out.fill_(float("nan"))
            forward()
            torch.cuda.synchronize()
            eager.append(out.clone())
        assert bool(torch.isfinite(eager[0]).all()) and not torch.equal(eager[0], eager[1])
        img.copy_(A)
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        g, stream = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.graph(g, stream=stream, capture_error_mode="global"):
            forward()
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), "the captured pass executed"
        for name, batch, want in (("A", A, eager[0]), ("B", B, eager[1]), ("A again", A, eager[0])):
            img.copy_(batch)
            out.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            G.assert_bits(out, want.cpu().numpy(), "replay on batch " + name)
        del g
    _guarded("the trunk pass", run)


# ---- the harness's teeth: torch ops only, no libisx call ----------------------------------------------------------------------------------------
class _TorchCase(S.Case):
    """A fake entry made of torch ops on the Regions (captured because torch.cuda.graph makes the capturing stream current); `before` runs at the end
    of the set-up, on the default stream, before the capture begins."""
    def __init__(self, fn, before=None, ws=None):
        x = np.arange(1, 65, dtype=np.float32)
        S.Case.__init__(self, dict(x=x), None, lambda a: dict(out=a.x * np.float32(2)), outs=dict(out=("f32", (64,))), ws=ws)
        self.fn, self.before = fn, before

    def _regions(self, data):
        r = S.Case._regions(self, data)
        if self.before is not None:
            self.before(types.SimpleNamespace(**r))
        return r

    def _invoke(self, r, stream):
        self.fn(types.SimpleNamespace(**r))
        return {}, 0.0


def _double(r):
    torch.mul(r.x.body, 2.0, out=r.out.body)


def _fake(expect, *args, **kw):
    """One fake through run_captured.  torch's own kernels are loaded by an eager call first, as run_plain() does for the library's."""
    def run():
        a, b = torch.ones(64, device="cuda"), torch.zeros(64, device="cuda")
        torch.mul(a, 2.0, out=b)
        b.add_(a)
        torch.cuda.synchronize()
        if expect is None:
            return _TorchCase(*args, **kw).run_captured()
        with pytest.raises(AssertionError, match=expect):
            _TorchCase(*args, **kw).run_captured()
    _guarded("harness self-test", run)


@gpu
def test_harness_passes_a_right_fake_entry():
    _fake(None, _double, ws=dict(ws=256))


@gpu
def test_harness_fails_a_result_that_depends_on_what_the_output_held():
    """out += x: the result depends on what the output held, so the replay over the leftovers of the earlier replays is wrong."""
    _fake("replay on stale state", lambda r: r.out.body.add_(r.x.body))


@gpu
def test_harness_fails_a_call_that_enqueues_nothing():
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                      # torch warns that the graph is empty
        _fake("left poisoned", lambda r: None)


@gpu
def test_harness_fails_an_output_written_before_the_capture_begins():
    _fake("the captured call EXECUTED", _double, before=_double)


# ---- four host threads on four streams -------------------------------------------------------------------------------------------------------------
WAIT = 120                                         # seconds: a safety net of the barriers, never waited for
ROUND = 6                                          # cases per thread and round: 24 Region sets alive at a time


@gpu
def test_four_host_threads_on_four_streams(plain):
    """Every C-ABI row without debug hooks (the hooks are process-global) from four threads at once: thread j walks the list rotated by
    j * len // 4, so the four launch DIFFERENT entries at the same time, each on its own stream and its own Regions.  A thread does nothing but
    case.call(L, pointers, its stream) and looks at the return code (ctypes releases the GIL: the launch paths overlap).  Thread 0 also makes a
    REFUSED call after each of its cases and reads its own error string; the others read theirs after a successful call.  The refused call is
    isx_l2norm_rows with D = -1 and live pointers; D = 0 is made as well, but the entry accepts it as an empty problem (csrc/pool.hip: returns 0
    and launches nothing), so it is asserted as that.  Neither may touch the poisoned y they are handed."""
    from isx._lib import lib
    _launching("the thread walk")
    L = lib()
    ids = [i for i in ABI_IDS if i not in _PLAIN_FAILED and _built(i).hooks is None]
    assert len(ids) >= 60 and all(_built(i).level == "abi" for i in ids)
    n = len(ids)
    walks = [ids[j * n // 4:] + ids[:j * n // 4] for j in range(4)]
    streams = [torch.cuda.Stream() for _ in range(4)]
    x = torch.ones((5, 8), device="cuda")
    y = G.out_f32((5, 8), 4096)
    work = [None] * 4                                                        # per thread: [(case, pointers)] of the round
    errors, seen = [[] for _ in range(4)], [[] for _ in range(4)]
    go, done = threading.Barrier(5), threading.Barrier(5)

    def walk(j):
        st = streams[j].cuda_stream
        while True:
            try:
                go.wait()
            except threading.BrokenBarrierError:
                return
            if work[j] is None:
                return
            try:
                for cid, c, p in work[j]:
                    rc = c.call(L, p, st)
                    if rc != 0:
                        errors[j].append((cid, rc, L.isx_last_error()))
                        break
                    if j == 0:
                        rc_empty = L.isx_l2norm_rows(x.data_ptr(), 5, 0, so.EPS, y.ptr, st)       # D = 0: an empty problem, accepted, launches nothing
                        rc = L.isx_l2norm_rows(x.data_ptr(), 5, -1, so.EPS, y.ptr, st)            # refused on the host
                        seen[j].append((cid, rc_empty, rc, L.isx_last_error()))
                    else:
                        seen[j].append((cid, L.isx_last_error()))
            except Exception as e:                                           # reported by the main thread; the barriers are still kept
                errors[j].append(("exception", repr(e)))
            try:
                done.wait()
            except threading.BrokenBarrierError:
                return

    threads = [threading.Thread(target=walk, args=(j,)) for j in range(4)]

    def run():
        for t in threads:
            t.start()
        try:
            for lo in range(0, n, ROUND):
                regions = [[(cid, _built(cid), _built(cid)._regions(_built(cid).ins)) for cid in walks[j][lo:lo + ROUND]] for j in range(4)]
                for j in range(4):
                    work[j] = [(cid, c, types.SimpleNamespace(**{k: G.ptr(v) for k, v in r.items()})) for cid, c, r in regions[j]]
                torch.cuda.synchronize()
                go.wait(WAIT)
                done.wait(WAIT)
                assert not any(errors), errors
                torch.cuda.synchronize()
                for j in range(4):
                    for cid, c, r in regions[j]:
                        c._verify(r, {}, c.expected(), "thread %d of four, %s" % (j, cid))
                del regions
        finally:
            for j in range(4):
                work[j] = None
            if not go.broken and not done.broken:
                go.wait(WAIT)
            for t in threads:
                t.join(WAIT)
    try:
        _guarded("the thread walk", run)
    finally:
        go.abort()
        done.abort()
    assert [len(s) for s in seen] == [n] * 4
    for cid, rc_empty, rc, msg in seen[0]:
        assert rc_empty == 0 and rc == -1 and msg.startswith(b"isx_l2norm_rows"), (cid, rc_empty, rc, msg)
    for j in (1, 2, 3):
        for cid, msg in seen[j]:
            assert b"isx_l2norm_rows" not in msg, ("thread %d sees thread 0's error string" % j, cid, msg)
    assert y.unwritten() == y.n and y.guards_intact(), "the refused and the empty call launched something"
