"""The late-producer harness of tests/test_gpu_stream_order.py, on top of tests/_guards.py.

Every other GPU test launches on torch's current stream with nothing else in flight: the `isx_stream_t stream` argument of the C ABI carries
no information there, everything serialises.  A Case here runs its entry on a fresh SIDE stream S behind a producer that is late:

  1. default stream: every Region of the case is allocated -- operands hold a DECOY (zeros, or the case's own valid decoy), outputs their
     poison, workspaces the byte pattern of _guards.workspace -- and the real operands lie in separate device tensors; torch.cuda.synchronize().
  2. on S (non-blocking: nothing on the null stream waits for it): a delay (torch.cuda._sleep), then the late producer -- device-to-device
     copies of the real operands into the operand bodies, every output re-poisoned, every workspace refilled --, an event `produced`, then the
     entry under test on S (C ABI: S.cuda_stream as the last argument; ops level: the wrapper under torch.cuda.stream(S)).
  3. host, as soon as the call returns: produced.query() must be False -- the call returned while its operands did not exist yet, so it did
     not wait for the device, and whatever it put on another stream has run against decoys / is about to be overwritten by the producer.
     An event that has fired FAILS the case ("delay too short"); it never passes in that state.
  4. S.synchronize(); guards intact, nothing left poisoned, results bit for bit the reference's; torch.cuda.synchronize().

Decoys are never NaN and never poison, and every operand a kernel derives an address from (indices, labels, rows, matrices) is in range as a
decoy: a stream-order mistake shows as wrong bits, not as a fault.  Every case asserts on the CPU that its reference gives something else
for the decoys than for the real operands.

Case.run_captured (tests/test_gpu_graph_capture.py) runs the same case a third way: the call captured into a HIP graph on a fresh stream under
the decoys, then the one graph replayed on decoys, on boosted operands, on the real operands over those leftovers and on poisoned buffers."""
import functools
import time
import types

import numpy as np
import torch

import _guards as G

_IN_KIND = {np.dtype(np.float32): ("f32", G.GUARD_IN_F32), np.dtype(np.int32): ("i32", None), np.dtype(np.int64): ("i64", None),
            np.dtype(np.uint64): ("i64", None), np.dtype(np.uint8): ("u8", None), np.dtype(np.float16): ("f16", G.GUARD_IN_F16),
            np.dtype(np.float64): ("f64", None)}
_INT = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}
MIN_DELAY_S = 0.020
DELAY_FACTOR = 20


def _flat_ints(a):
    a = np.array(a, order="C")                              # a copy: the shared cases of the model files are read-only
    return a.reshape(-1).view(_INT[a.dtype.itemsize])


class Case(object):
    """One entry (or wrapper) behind the late producer.
    ins     name -> host array (the REAL operand; None: an optional operand left out).  dtype decides the Region kind.
    io      names of `ins` that the entry updates in place: sentinel guards, compared with ref()[name] afterwards.
    outs    name -> (kind, shape): poisoned outputs.
    ws      name -> bytes: workspaces (the pattern of _guards.workspace).
    decoy   name -> host array: a case's own valid decoy where zeros are not one.
    guard   name -> guard elements (default 4096).
    call    level "abi": call(L, p, st) -> rc with p.<name> the pointers (None for an absent operand) and st the stream handle;
            level "ops": call(r) -> {name: tensor} of the results the wrapper allocated itself; r.<name> are the Regions (r.x.body: the tensor).
    ref     ref(a) -> {name: host array} from the operand arrays a.<name>: the existing reference of the entry.
    sample  name -> fn(body tensor) -> tensor: the part of a large output that ref() describes.
    check   name -> fn(got, want, a): a comparison other than bit for bit, where the entry's existing tests have one (never a new tolerance).
    hooks   (gemm, conv, f16) debug settings around the call, as the existing tests force a path."""
    def __init__(self, ins, call, ref, outs=None, io=(), ws=None, decoy=None, guard=None, sample=None, check=None, hooks=None, level="abi"):
        self.ins, self.call, self.ref, self.outs, self.io, self.ws = ins, call, ref, outs or {}, tuple(io), ws or {}
        self.decoy, self.guard, self.sample, self.check, self.hooks, self.level = decoy or {}, guard or {}, sample or {}, check or {}, hooks, level
        self.host_seconds, self.post, self._want = None, None, None           # post(L, p): a check after the stream has drained that needs the pointers

    # ---- CPU side ------------------------------------------------------------------------------------------------------------------------------
    def decoys(self):
        d = {}
        for n, a in self.ins.items():
            d[n] = None if a is None else np.ascontiguousarray(self.decoy[n], a.dtype).reshape(a.shape) if n in self.decoy else np.zeros_like(a)
        return d

    def expected(self):
        """The reference on the real operands -- after asserting that it says something else on the decoys.  Computed once per case."""
        if self._want is not None:
            return self._want
        want = self.ref(types.SimpleNamespace(**self.ins))
        with np.errstate(all="ignore"):
            on_decoys = self.ref(types.SimpleNamespace(**self.decoys()))
        assert set(want) == set(on_decoys)
        differs = any(np.asarray(want[n]).shape != np.asarray(on_decoys[n]).shape or
                      np.asarray(want[n]).tobytes() != np.asarray(on_decoys[n]).tobytes() for n in want)
        assert differs, "the reference gives the same result for the decoys: the case would pass on them"
        self._want = want
        return want

    # ---- GPU side ------------------------------------------------------------------------------------------------------------------------------
    def _regions(self, data):
        r = {}
        for n, a in data.items():
            if a is None:
                r[n] = None
                continue
            kind, gv = _IN_KIND[a.dtype]
            r[n] = G.Region(kind, a.shape, self.guard.get(n, 4096), data=_flat_ints(a), guard_value=None if n in self.io else gv)
        for n, (kind, shape) in self.outs.items():
            r[n] = G.Region(kind, shape, self.guard.get(n, 4096))
        for n, nbytes in self.ws.items():
            r[n] = G.workspace(nbytes)
        return r

    def _invoke(self, r, stream):
        L = None
        if self.hooks is not None:
            from isx._lib import lib
            L = lib()
            L.isx_debug_set_gemm_cfg(self.hooks[0]); L.isx_debug_set_conv_cfg(self.hooks[1]); L.isx_debug_set_f16_tile(self.hooks[2])
        try:
            t0 = time.perf_counter()
            if self.level == "abi":
                from isx._lib import lib
                L = lib()
                rc = self.call(L, types.SimpleNamespace(**{n: G.ptr(x) for n, x in r.items()}), stream.cuda_stream)
                took = time.perf_counter() - t0
                assert rc == 0, (rc, L.isx_last_error())
                return {}, took
            res = self.call(types.SimpleNamespace(**r))
            return res or {}, time.perf_counter() - t0
        finally:
            if self.hooks is not None:
                L.isx_debug_set_gemm_cfg(-1); L.isx_debug_set_conv_cfg(-1); L.isx_debug_set_f16_tile(-1)

    def _verify(self, r, res, want, what):
        outs = [r[n] for n in self.outs if self.outs[n][0] != "u8"]          # a byte output may legitimately hold the poison byte: its bits decide
        G.assert_clean(outs, [x for n, x in r.items() if n in self.ins and x is not None], what)
        for n in list(self.outs) + list(self.ws) + list(self.io):
            assert r[n].guards_intact(), ("store outside", n, what)
        a = types.SimpleNamespace(**self.ins)
        assert set(want) == set(self.outs) | set(self.io) | set(res), ("every output is compared", sorted(want), what)
        for n in want:
            got = res[n] if n in res else r[n].body
            if n in self.sample:
                got = self.sample[n](got)
            got = got.contiguous().cpu().numpy()
            if n in self.check:
                self.check[n](got, want[n], a)
            elif got.dtype.itemsize == 1:
                assert np.array_equal(got, np.asarray(want[n]).reshape(got.shape)), (n, what, int((got != np.asarray(want[n]).reshape(got.shape)).sum()))
            else:
                G.assert_bits(got, np.ascontiguousarray(want[n]).reshape(got.shape), (n, what))
        if self.post is not None:
            from isx._lib import lib
            self.post(lib(), types.SimpleNamespace(**{n: G.ptr(x) for n, x in r.items()}))

    def run_plain(self):
        """The case on the default stream with its real operands: warms the kernels up, measures the host time of the call (what the delay is sized
        from) and checks the result, so that a failure behind the late producer is one of stream order."""
        want = self.expected()
        r = self._regions(self.ins)
        torch.cuda.synchronize()
        st = torch.cuda.current_stream()
        res, _ = self._invoke(r, st)                                        # the first call of a kernel loads its code object
        torch.cuda.synchronize()
        for n in list(self.outs) + list(self.ws):
            r[n].raw().fill_(r[n].poison)
        for n in self.io:
            r[n].raw().copy_(torch.from_numpy(_flat_ints(self.ins[n])).cuda())
        torch.cuda.synchronize()
        res, took = self._invoke(r, st)
        torch.cuda.synchronize()
        self._verify(r, res, want, "default stream")
        self.host_seconds = took
        return took

    def run_late(self, cycles):
        want = self.expected()
        r = self._regions(self.decoys())
        real = {n: torch.from_numpy(_flat_ints(a)).cuda() for n, a in self.ins.items() if a is not None}
        torch.cuda.synchronize()
        S = torch.cuda.Stream()
        try:
            with torch.cuda.stream(S):
                torch.cuda._sleep(cycles)
                for n, t in real.items():
                    r[n].raw().copy_(t)
                for n in list(self.outs) + list(self.ws):
                    r[n].raw().fill_(r[n].poison)
                produced = torch.cuda.Event()
                produced.record(S)
                res, took = self._invoke(r, S)
                fired = produced.query()
            assert not fired, ("delay too short: the late producer had finished when the call returned after %.1f ms -- the run proves nothing" % (took * 1e3))
            S.synchronize()
            self._verify(r, res, want, "side stream behind a late producer")
        finally:
            torch.cuda.synchronize()                                        # also after a failure: nothing of S is pending when the regions go out of scope
        return took

    # ---- captured into a HIP graph and replayed (tests/test_gpu_graph_capture.py) ----------------------------------------------------------------
    def _dev(self, data):
        return {n: torch.from_numpy(_flat_ints(a)).cuda() for n, a in data.items() if a is not None}

    def _fresh(self, r, res=()):
        """Outputs their poison, workspaces their pattern, and whatever the wrapper allocated itself a value no result holds."""
        for n in list(self.outs) + list(self.ws):
            r[n].raw().fill_(r[n].poison)
        for t in res:
            t.fill_(float("nan") if t.is_floating_point() else G.POISON_U8 if t.dtype == torch.uint8 else G.POISON_I32)

    def _nothing_executed(self, r, decoy):
        """After the capture has closed: the captured call ran nothing.  Every output is entirely poison, every workspace its pattern, every
        in-place operand its decoy, every guard intact."""
        for n in list(self.outs) + list(self.ws):
            left = r[n].unwritten()
            assert left == r[n].n, ("the captured call EXECUTED: %d of %d elements of %s written before any replay" % (r[n].n - left, r[n].n, n), "capture")
        for n in self.io:
            assert torch.equal(r[n].raw(), decoy[n]), ("the captured call EXECUTED: the in-place operand %s changed before any replay" % n, "capture")
        self._guards(r, "capture")

    def _guards(self, r, what):
        for n, x in r.items():
            assert x is None or x.guards_intact(), ("store outside", n, what)

    def _replayed(self, g, r, what):
        g.replay()
        torch.cuda.synchronize()
        self._guards(r, what)

    def _wrote_something(self, r, what):
        for n in self.outs:
            assert r[n].unwritten() < r[n].n, ("left poisoned: the replay wrote nothing of %s" % n, what)

    def run_captured(self):
        """The case captured into a graph on a fresh stream and replayed -- after the caller's run_plain(), which has loaded the code objects.

        C ABI:  1. capture under DECOYS (nothing but the call inside the capture; the return code is asserted after it has closed; nothing executed)
                2. replay on the decoys: real leftovers in outputs and workspaces
                3. (cases with a workspace) replay on BOOSTED operands, every fp32 operand x 4: leftovers that beat every real score
                4. real operands, outputs NOT re-poisoned, workspaces NOT refilled: replay, the reference's bits ("replay on stale state")
                5. outputs poisoned, workspaces refilled, in-place operands restored: replay, the reference's bits ("replay on poisoned state")
        Wrappers (level "ops"): capture under decoys (what the wrapper allocates lies in the graph's pool and comes back as its results), nothing
        of `outs` written; real operands, replay, verify; re-poison, replay, verify.
        An AssertionError leaves the device drained; any other exception launches nothing more (the caller stops its pass)."""
        from isx._lib import IsxError
        want = self.expected()
        r = self._regions(self.decoys())
        real, decoy = self._dev(self.ins), self._dev(self.decoys())
        boosted = self._dev({n: a * a.dtype.type(4) if a is not None and a.dtype == np.float32 else a for n, a in self.ins.items()})
        torch.cuda.synchronize()
        stream, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        refused, res = None, {}
        try:
            with torch.cuda.graph(g, stream=stream, capture_error_mode="global"):
                try:
                    res, _ = self._invoke(r, stream)
                except (AssertionError, IsxError) as e:                     # a non-zero return code: reported once the capture has closed
                    refused = e
            torch.cuda.synchronize()
            if refused is not None:
                raise AssertionError("the call was refused under capture: %r" % (refused,)) from refused
            self._nothing_executed(r, decoy)
            if self.level == "abi":
                self._replayed(g, r, "replay on decoys")
                if self.ws:
                    for n, t in boosted.items():
                        r[n].raw().copy_(t)
                    self._replayed(g, r, "replay on boosted operands")
                for n, t in real.items():
                    r[n].raw().copy_(t)
                self._replayed(g, r, "replay on stale state")
                self._wrote_something(r, "replay on stale state")
                post, self.post = self.post, None                           # Case.post runs once, after the last replay
                try:
                    self._verify(r, {}, want, "replay on stale state")
                finally:
                    self.post = post
            else:
                for n, t in real.items():
                    r[n].raw().copy_(t)
                self._replayed(g, r, "replay on real operands")
                self._wrote_something(r, "replay on real operands")
                self._verify(r, res, want, "replay on real operands")
            self._fresh(r, res.values())
            for n in self.io:
                r[n].raw().copy_(real[n])
            self._replayed(g, r, "replay on poisoned state")
            self._wrote_something(r, "replay on poisoned state")
            self._verify(r, res, want, "replay on poisoned state")
        except AssertionError:
            torch.cuda.synchronize()                                        # nothing of the replays is pending when the regions go out of scope
            raise
        finally:
            del res, g


@functools.lru_cache(maxsize=None)
def sleep_cycles_per_second():
    """torch.cuda._sleep between two events on an idle GPU: cycles per second of the counter it spins on.  Measured once per process (it
    synchronises the device: call it outside any side-stream work)."""
    torch.cuda.synchronize()
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    best = None
    for cycles in (2000000, 20000000):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        torch.cuda.synchronize()
        best = cycles / (a.elapsed_time(b) * 1e-3)
    return best


def delay_cycles(slowest_host_call_s, rate):
    """(cycles, seconds): DELAY_FACTOR x the slowest host-side call of the file, at least MIN_DELAY_S."""
    seconds = max(DELAY_FACTOR * slowest_host_call_s, MIN_DELAY_S)
    return int(seconds * rate), seconds
