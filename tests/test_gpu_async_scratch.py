"""GPU tier: calls in flight must not share the context slot's scratch across streams.

A context slot (DevState in zerocaf_hip.hip) owns scratch that outlives a call: `bal`, `fast` / `ring`, `msm` / `ris_sum` with
the side streams `aux` and `grp`, the lazily built `base_table` / `odd_table`, `part`, the staging areas.  Device-resident calls
are asynchronous on the slot's stream; the library keeps them apart by stream order, by one event when the stream changes
(zc_ctx_set_stream_dev) and by the fork / join events inside the MSM, and Engine binds the slot to torch's current stream before
every call on tensors.

The common shape of a case (tests/async_cases.py holds the calls and the pairs): two calls that reach the same buffer, of equal
shapes but different values -- an index that leaks from one into the other still lies inside both calls' buffers, so an ordering
defect shows as wrong bytes, never as a fault.  Inputs are uploaded and synchronised; then, without a host synchronisation in
between, a filler (strict scalar-mul of 2^15 rows) and the first call go on stream 1 and the second under torch.cuda.stream(side);
then both streams are synchronised.  Both outputs must equal, byte for byte, what the same call returns alone on a fresh,
synchronised engine, and a fixed sample of those rows must equal the oracle.  Each pair runs in both orders and once more with
both calls on one stream.  Every case prints the scratch it reaches with the size constant that proves it, and per call whether
it was left pending behind the filler (asynchronous) or synchronised internally (then the case checks the switch only)."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

from tests import async_cases as AC
from tests import vectors as V

pytestmark = pytest.mark.gpu

FILLER_CALLS = 1                        # strict scalar-muls of FILLER_ROWS rows in front of the first call (the calibration test says whether one is seen)
SEED_A, SEED_B = 1, 2


def dev(a):
    import torch
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def host(x):
    """an output as a numpy array: tensors come back from the device (the caller has synchronised), bytes become uint8"""
    if isinstance(x, (bytes, bytearray)):
        return np.frombuffer(x, dtype=np.uint8)
    if isinstance(x, np.ndarray):
        return x
    a = x.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


class Bench:
    """Inputs, their device copies and the results of every call alone, made once per module and never changed."""

    def __init__(self, oracle):
        self.oracle, self._ins, self._dev, self._alone = oracle, {}, {}, {}

    def ins(self, call, seed):
        key = (call.id, seed)
        if key not in self._ins:
            arrays = call.gen(self.oracle, seed)
            for a in arrays:
                a.setflags(write=False)
            self._ins[key] = arrays
        return self._ins[key]

    def dev(self, call, seed):
        import torch
        key = (call.id, seed)
        if key not in self._dev:
            self._dev[key] = tuple(dev(np.array(a)) for a in self.ins(call, seed))
            torch.cuda.synchronize()
        return self._dev[key]

    def filler(self):
        return self.dev(FILLER, 0)

    def alone(self, call, seed, env):
        """the call on a fresh engine with nothing else in flight, synchronised; its sampled rows checked against the oracle"""
        import torch
        key = (call.id, seed, tuple(sorted(env.items())))
        if key not in self._alone:
            with V.tuned(**env) as e:
                d = self.dev(call, seed)
                st = call.setup(e, d) if call.setup else None
                torch.cuda.synchronize()
                outs = call.run(e, d, st)
                torch.cuda.synchronize()
                outs = tuple(np.array(host(o)) for o in outs)
                if st is not None:
                    st.close()
            call.check(self.oracle, self.ins(call, seed), outs)
            self._alone[key] = outs
        return self._alone[key]


FILLER = AC.Call("filler", "-", "-", lambda o, s: (AC.points(o, AC.FILLER_ROWS, 7), AC.scalars(AC.FILLER_ROWS, 7)), None, None)


@pytest.fixture(scope="module")
def bench(oracle):
    import torch  # noqa: F401  (before the library, so that one HIP runtime is shared)
    return Bench(oracle)


def run_filler(e, bench, calls=None):
    fP, fK = bench.filler()
    return [e.ed_scalar_mul(fP, fK) for _ in range(FILLER_CALLS if calls is None else calls)]


def run_two(bench, first, second, how, env):
    """(outputs of the first, outputs of the second) as numpy arrays: `first` = (call, seed) behind the filler on stream 1,
    `second` under the side stream ("switch"); the first under the side stream, the second at once on stream 1, nothing in
    front ("side_first"); both behind the filler on stream 1 ("same")."""
    import torch
    (c1, s1), (c2, s2) = first, second
    with V.tuned(**env) as e:
        d1, d2 = bench.dev(c1, s1), bench.dev(c2, s2)
        st1 = c1.setup(e, d1) if c1.setup else None
        st2 = c2.setup(e, d2) if c2.setup else None
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        keep = []
        if how == "side_first":
            with torch.cuda.stream(side):
                o1 = c1.run(e, d1, st1)
            o2 = c2.run(e, d2, st2)
        else:
            keep = run_filler(e, bench)
            o1 = c1.run(e, d1, st1)
            if how == "switch":
                with torch.cuda.stream(side):
                    o2 = c2.run(e, d2, st2)
            else:
                o2 = c2.run(e, d2, st2)
        side.synchronize()
        torch.cuda.current_stream().synchronize()
        got = tuple(np.array(host(o)) for o in o1), tuple(np.array(host(o)) for o in o2)
        del keep
        for st in (st1, st2):
            if st is not None:
                st.close()
    return got


def same_bytes(got, want, what):
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, j, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), "%s: output %d differs from the call alone in rows %s" % (
            what, j, np.flatnonzero((g.reshape(len(g), -1) != w.reshape(len(w), -1)).any(axis=1))[:8])


@pytest.mark.parametrize("pair", AC.PAIRS, ids=["%s+%s" % (a, b) for a, b, _ in AC.PAIRS])
def test_two_calls_in_flight_share_scratch(bench, pair):
    """One pair of tests/async_cases.py PAIRS in three orders: A then B across the stream switch, B then A, A then B on one
    stream.  Asynchronous calls (every row-wise entry point on device tensors, zc_msm_partial) are left pending behind the
    filler while the next is enqueued; zc_msm_batch, zc_msm_fixed and zc_ris_lincomb_sum end in hipStreamSynchronize, so a pair
    with one of them as the first call checks the stream switch and the reuse of the workspace, and cannot overlap."""
    a, b, how = pair
    A, B = (AC.CALLS[a], SEED_A), (AC.CALLS[b], SEED_B)
    env = dict(A[0].env, **B[0].env)
    t0 = time.perf_counter()
    want = {A: bench.alone(A[0], SEED_A, env), B: bench.alone(B[0], SEED_B, env)}
    t1 = time.perf_counter()
    for first, second, h in ((A, B, how), (B, A, how), (A, B, "same")):
        got1, got2 = run_two(bench, first, second, h, env)
        what = "%s(seed %d) then %s(seed %d), %s" % (first[0].id, first[1], second[0].id, second[1], h)
        same_bytes(got1, want[first], what + ": the first")
        same_bytes(got2, want[second], what + ": the second")
    said = lambda c: "%s reaches %s (%s), %s" % (c.id, c.scratch, c.proof, "synchronises internally: the switch only" if c.sync else "asynchronous: left pending")
    print("\n[async] %s | %s | orders: A-B %s, B-A %s, A-B one stream | alone + oracle %.2f s, orders %.2f s" % (
        said(A[0]), said(B[0]), how, how, t1 - t0, time.perf_counter() - t1))


def test_fold_of_partials_behind_an_unfinished_msm_partial(bench, oracle):
    """`part`: zc_ed_fold_ordered of 8 partials whose last row an unfinished zc_msm_partial (MSM_BUCKET_MIN_N pairs, behind the
    filler on stream 1) is still to write -- on device rows under the side stream (asynchronous: the fold kernel reads the
    caller's rows, ordered by the switch event), and on host rows (the fold stages them in `part` on the slot's stream and
    synchronises).  The fold is limb-exact against the oracle's unified additions over the rows it was given."""
    import torch
    from tests import entry_table as ET
    msm = AC.CALLS["msm_partial"]
    last = bench.alone(msm, SEED_A, {})[0]
    parts = np.concatenate([AC.points(oracle, 7, 5), last])
    want = ET._fold_want(ET.Gen(oracle), parts)[0]
    dP, dK = bench.dev(msm, SEED_A)
    for rows_on_device in (True, False):
        with V.tuned() as e:
            dparts = dev(np.concatenate([parts[:7], np.zeros((1, 20), dtype=np.uint64)]))
            side = torch.cuda.Stream()
            torch.cuda.synchronize()
            keep = run_filler(e, bench)
            e.msm_partial(dP, dK, out=dparts[7:8])
            if rows_on_device:
                with torch.cuda.stream(side):
                    got = e.ed_fold_ordered(dparts)
            else:
                pending = e.msm_partial(dP, dK)                    # still in flight when the host rows are staged behind it
                got = e.ed_fold_ordered(parts)
            side.synchronize()
            torch.cuda.current_stream().synchronize()
            assert np.array_equal(host(got), want), "fold of %s rows" % ("device" if rows_on_device else "host")
            assert np.array_equal(host(dparts[7:8]), last)
            if not rows_on_device:
                assert np.array_equal(host(pending), last)
            del keep
    print("\n[async] zc_ed_fold_ordered of 8 partials behind an unfinished zc_msm_partial (%d pairs): device rows asynchronous under the side "
          "stream; host rows reach `part` ((count + 1) * 160 bytes) and synchronise internally" % AC.BUCKET_N)


@pytest.mark.parametrize("device_first", [True, False], ids=["device_call_first", "host_call_first"])
def test_host_array_calls_beside_a_device_resident_call(bench, oracle, device_first):
    """Staging (`scratch[]`, the copy streams): host-array calls (zc_fe_mul, zc_ed_scalar_mul, 2500 rows, ZC_HOST_CHUNKS=3: three
    ragged chunks through copy_in / the slot's stream / copy_out) issued while a device-resident strict scalar-mul of 2^15 rows on
    a torch side stream is still running, and the reverse order.  The host-array calls synchronise internally; the device call
    is asynchronous."""
    import torch
    n = 2500
    a, b = V.rand_fe_np(n, AC.SEED + 400), V.rand_fe_np(n, AC.SEED + 401)
    P, K = AC.points(oracle, n, 9), AC.scalars(n, 9)
    fwant = bench.alone(AC.Call("filler_alone", "-", "-", FILLER.gen, lambda e, d, st: (e.ed_scalar_mul(d[0], d[1]),), AC._check_strict), 0, {})[0]
    with V.tuned(ZC_HOST_CHUNKS=3) as e:
        side = torch.cuda.Stream()
        fP, fK = bench.filler()
        torch.cuda.synchronize()
        if device_first:
            with torch.cuda.stream(side):
                f = e.ed_scalar_mul(fP, fK)
        m = e.fe_mul(a, b)
        q = e.ed_scalar_mul(P, K)
        if not device_first:
            with torch.cuda.stream(side):
                f = e.ed_scalar_mul(fP, fK)
        side.synchronize()
        assert np.array_equal(m, oracle.fe_mul(a, b)) and np.array_equal(q, oracle.mt(oracle.ed_scalar_mul, P, K))
        assert np.array_equal(host(f), fwant)
    print("\n[async] staging: zc_fe_mul and zc_ed_scalar_mul on host arrays (2500 rows, ZC_HOST_CHUNKS=3) %s a device-resident strict scalar-mul of "
          "%d rows on a side stream; host calls synchronise internally" % ("behind" if device_first else "before", AC.FILLER_ROWS))


# ------------------------------------------------------------------ 2b: threads with their own streams, one Engine
@pytest.mark.parametrize("sync_thread", [False, True], ids=["launchers", "launchers_and_synchronize"])
def test_threads_with_their_own_streams_share_an_engine(bench, sync_thread):
    """One Engine, three threads, each under its own torch.cuda.Stream, each a few rounds of one family on its own tensors --
    the persistent strict scalar-mul (`bal`), zc_msm_partial at the bucket size (`msm`, `aux`), zc_ris_lincomb of 2 terms + base
    at 4097 rows (`fast` / `ring`, `base_table`) -- and each consumes its output on its own stream with out.clone(), without a
    host synchronisation.  Compared after joining with the calls alone.  With `sync_thread` a fourth thread calls
    Engine.synchronize() 50 times meanwhile: it reads the slot's stream while the others switch it."""
    import torch
    families = [AC.CALLS["strict_pw"], AC.CALLS["msm_partial"], AC.CALLS["ris_lincomb2b"]]
    want = [bench.alone(c, SEED_A, {}) for c in families]
    devs = [bench.dev(c, SEED_A) for c in families]
    rounds, clones, errs = 3, [[] for _ in families], []
    with V.tuned() as e:
        streams = [torch.cuda.Stream() for _ in families]
        torch.cuda.synchronize()
        start = threading.Barrier(len(families) + (1 if sync_thread else 0))

        def launcher(i):
            try:
                start.wait()
                with torch.cuda.stream(streams[i]):
                    for _ in range(rounds):
                        outs = families[i].run(e, devs[i], None)
                        clones[i].append(tuple(o.clone() for o in outs))
            except Exception as ex:                                # noqa: BLE001
                errs.append((families[i].id, ex))

        def synchroniser():
            try:
                start.wait()
                for _ in range(50):
                    e.synchronize()
            except Exception as ex:                                # noqa: BLE001
                errs.append(("synchronize", ex))

        ts = [threading.Thread(target=launcher, args=(i,)) for i in range(len(families))]
        if sync_thread:
            ts.append(threading.Thread(target=synchroniser))
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for s in streams:
            s.synchronize()
        assert not errs, errs
        for i, c in enumerate(families):
            assert len(clones[i]) == rounds
            for r, outs in enumerate(clones[i]):
                same_bytes(tuple(np.array(host(o)) for o in outs), want[i], "%s, round %d, consumed on its thread's stream" % (c.id, r))
    print("\n[async] three threads under their own streams on one Engine%s: %s; all asynchronous, consumed by clone() without a host sync"
          % (" + Engine.synchronize() x 50" if sync_thread else "", ", ".join("%s (%s)" % (c.id, c.scratch) for c in families)))


# ------------------------------------------------------------------ 2c: zc_ctx_synchronize across a stream switch, raw ABI
def test_ctx_synchronize_covers_work_on_both_sides_of_a_stream_switch(bench):
    """zc_ctx_set_stream with an external stream; a launch; zc_ctx_set_stream(NULL, 0); a launch on the context's own stream;
    zc_ctx_synchronize must cover both, because the switch event orders the own stream behind the external one.  Both outputs
    were pre-filled, and are read back after the library's synchronisation alone."""
    import torch
    from dusk_zerocaf_amd import _lib
    strict = AC.Call("filler_alone", "-", "-", FILLER.gen, lambda e, d, st: (e.ed_scalar_mul(d[0], d[1]),), AC._check_strict)
    want = bench.alone(strict, 0, {})[0]
    fP, fK = bench.filler()
    n = AC.FILLER_ROWS
    with V.tuned() as e:
        ext = torch.cuda.Stream()
        out1, out2 = torch.zeros((n, 20), dtype=torch.int64, device="cuda"), torch.zeros((n, 20), dtype=torch.int64, device="cuda")
        pin1, pin2 = torch.empty((n, 20), dtype=torch.int64).pin_memory(), torch.empty((n, 20), dtype=torch.int64).pin_memory()
        torch.cuda.synchronize()
        _lib.check(e.lib.zc_ctx_set_stream(e.ctx, C.c_void_p(ext.cuda_stream), 1), "zc_ctx_set_stream", e.lib)
        e._call("zc_ed_scalar_mul", fP.data_ptr(), fK.data_ptr(), out1.data_ptr(), n, 0)
        _lib.check(e.lib.zc_ctx_set_stream(e.ctx, None, 0), "zc_ctx_set_stream", e.lib)
        e._call("zc_ed_scalar_mul", fP.data_ptr(), fK.data_ptr(), out2.data_ptr(), n, 0)
        _lib.check(e.lib.zc_ctx_synchronize(e.ctx), "zc_ctx_synchronize", e.lib)
        # read on a third stream that is ordered with neither: only the library's wait stands between the kernels and the copies
        reader = torch.cuda.Stream()
        with torch.cuda.stream(reader):
            pin1.copy_(out1, non_blocking=True)
            pin2.copy_(out2, non_blocking=True)
        reader.synchronize()
        assert np.array_equal(pin2.numpy().view(np.uint64), want), "the launch on the context's own stream"
        assert np.array_equal(pin1.numpy().view(np.uint64), want), "the launch on the external stream, before the switch"
        ext.synchronize()
    print("\n[async] zc_ctx_synchronize after external stream -> own stream: both launches (strict scalar-mul, %d rows, asynchronous) complete" % n)


# ------------------------------------------------------------------ 3: can this harness see a missing order at all?
def test_calibration_an_unordered_read_behind_the_filler(bench):
    """Torch-owned memory only: the filler and a library call write `out` (pre-filled with a sentinel) on stream 1, and a plain
    out.clone() on the side stream does NOT wait for them.  Five repetitions per filler length; the count of clones that still
    hold the sentinel says whether a missing event behind a filler of that length would be seen.  Nothing is asserted about the
    count -- an unordered read may legitimately see either -- it is printed.  (A read of initialised memory: it cannot fault.)"""
    import torch
    sentinel = 0x5A5A5A5A5A5A5A5A
    fP, fK = bench.filler()
    counts = {}
    with V.tuned() as e:
        side = torch.cuda.Stream()
        for fillers in (1, 2):
            stale = 0
            for _ in range(5):
                out = torch.full((AC.FILLER_ROWS, 20), sentinel, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                keep = run_filler(e, bench, fillers)
                e.ed_scalar_mul(fP, fK, out=out)
                with torch.cuda.stream(side):
                    seen = out.clone()                           # unordered with stream 1 on purpose
                torch.cuda.synchronize()
                stale += int((seen == sentinel).all(dim=1).any().item())
                assert not (out == sentinel).all(dim=1).any().item()
                del keep
            counts[fillers] = stale
    print("\n[async] calibration: an unordered clone on the side stream still held the sentinel in %d of 5 runs behind 1 filler call, "
          "%d of 5 behind 2 (the cases use %d)" % (counts[1], counts[2], FILLER_CALLS))
