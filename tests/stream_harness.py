"""The stream contract of include/wlhip.h, made testable: "every call is asynchronous on `stream` unless it returns a host scalar, in
which case it synchronises that stream".

On the default stream everything a process launches is serialised, so work that the library puts on the wrong stream, a fork taken from the
wrong stream, a missing join or a read-back that waits for the wrong stream all go unnoticed.  run_on_streams() runs a scenario (a list of
Step: one library call each, plus the device arrays it owns) once on the default stream — the baseline: every array after every step and
every returned host scalar, as bits — and then again on a non-blocking side stream S with two arming devices in force:

  inputs behind a delay   before every step the scenario's arrays are cloned, overwritten with a finite sentinel (3.0e30f) and S is synchronised;
                          then a delay and, behind it, the copy of the clones back into the arrays are queued on S, and the call is made on S.
                          Work that runs ahead of S — on another stream, or on a forked stream that did not wait — reads the sentinel.
  default stream blocked  a long delay is queued on the default stream before the first step.  Non-blocking streams do not wait for it; whatever the
                          library puts on stream 0 is held until everything on S is over.  This is the only device that arms the parts of a call
                          that follow its own host read-back (after that read the per-step delay has run out).

Arrays are snapshot on S right after each call, with no synchronisation in between, and compared with np.array_equal after one
synchronisation at the end; host scalars are compared as the call returned them.  Each run checks its own arming: S.query() must be False
when an asynchronous call returns, and the default stream must still be busy at the end — a run that was not armed FAILS ("not armed").
The side streams are chosen by pick_streams(): streams that share the default stream's hardware queue are held behind the blocker and cannot arm anything.
Nothing here provokes a fault: every array is allocated and a misplaced launch reads finite values.

Delays (torch.cuda._sleep, cycles per ms calibrated once per process with an event pair): per step max(2 ms, 10 × the host time the baseline
needed to enqueue that step, and 10 × the host time of queueing the restore); the blocker max(50 ms, 5 × T, 3 × (T + Σ step delays)) with T the baseline's wall time measured in the same
test (the third term because the armed run is longer than the baseline by its own delays).
Sizes measured on an MI355X: see MEASURED below.
"""
import ctypes as C
import time
from dataclasses import dataclass, field
from typing import Any, Callable, List, Optional

import numpy as np

SENTINEL = 3.0e30
MIN_STEP_MS, STEP_FACTOR = 2.0, 10.0
MIN_BLOCK_MS, BLOCK_FACTOR, BLOCK_RUN_FACTOR = 50.0, 5.0, 3.0

# one run of tests/test_gpu_streams.py on an MI355X (every armed run prints its own figures with `pytest -s`)
MEASURED = ("torch.cuda._sleep: 2.04e6 cycles per ms; baselines T = 0.4–8.5 ms; blockers 50–370 ms (leaf tables 98–370 ms, handle scenarios 50–284 ms); "
            "step delays 2.0–27.8 ms (2.0 ms for almost every leaf row, the larger ones for wl_sim_mom_steps and wl_sim_phase)")


class NotArmed(AssertionError):
    pass


class Raw:
    """a device array the library owns, named by a getter of its CURRENT pointer (the roles of a handle's arrays rotate) and its size in floats;
    it is reached with wl_d2d on the stream in force"""

    def __init__(self, name, getter, nfloats):
        self.name, self.getter, self.nfloats = name, getter, int(nfloats)


@dataclass
class Step:
    name: str                                 # the entry point this step is about ("wl_fill")
    call: Callable[[Any], Any]                # call(stream_pointer) -> host scalars (ctypes objects / numpy arrays / numbers) or None
    arrays: List[Any] = field(default_factory=list)    # torch tensors and Raw: everything the call reads or writes
    sync: bool = False                        # the call returns a host scalar: it synchronises its stream
    stream: int = 0                           # index of the side stream (armed run); −1: the default stream
    pre: Optional[Callable[[list], None]] = None       # armed run only: pre(streams) before the step (wait_stream, synchronize, ...)


def _host_bits(v):
    if v is None:
        return None
    if isinstance(v, (tuple, list)):
        return tuple(_host_bits(q) for q in v)
    if isinstance(v, np.ndarray):
        return v.tobytes()
    if isinstance(v, (C._SimpleCData, C.Array, C.Structure)):
        return bytes(v)
    if isinstance(v, float):
        return np.float64(v).tobytes()
    return v


_cycles_per_ms = None


def cycles_per_ms():
    global _cycles_per_ms
    if _cycles_per_ms is None:
        import torch
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        n = 20_000_000
        torch.cuda._sleep(1000)
        a.record(); torch.cuda._sleep(n); b.record()
        torch.cuda.synchronize()
        _cycles_per_ms = n / max(a.elapsed_time(b), 1e-3)
    return _cycles_per_ms


def sleep_ms(ms):
    import torch
    torch.cuda._sleep(int(ms * cycles_per_ms()))


def pick_streams(n, probe_ms=30.0):
    """n fresh non-blocking torch streams that really do not wait for the default stream.  A process has a few hardware queues (4 here) and the
    runtime deals its streams onto them: a side stream that landed on the default stream's queue is held behind the blocker although nothing orders
    the two (measured on the MI355X: 1 of 6 torch streams, 255 ms behind a 300 ms blocker).  Such a stream cannot arm anything, so the candidates are
    probed behind a short blocker of their own and the held ones are left out.  The assignment is made once per stream: a stream found free stays free."""
    import torch
    cycles_per_ms()
    cands = [torch.cuda.Stream() for _ in range(n + 6)]
    flag = torch.zeros(len(cands), dtype=torch.float32, device="cuda")
    evs = [torch.cuda.Event() for _ in cands]
    torch.cuda.synchronize()
    sleep_ms(probe_ms)
    for i, c in enumerate(cands):
        with torch.cuda.stream(c):
            flag[i:i + 1].fill_(1.0)
            evs[i].record()
    t0 = time.perf_counter()
    free = []
    while time.perf_counter() - t0 < 0.4e-3 * probe_ms:
        free = [i for i, e in enumerate(evs) if e.query()]
        if len(free) == len(cands):
            break
    held_default = not torch.cuda.default_stream().query()
    torch.cuda.synchronize()
    if not held_default or len(free) < n:
        raise NotArmed(f"not armed: {len(free)} of {len(cands)} candidate streams ran ahead of the default stream (blocker still busy: {held_default}), {n} needed")
    return [cands[i] for i in free[:n]]


class _Arrays:
    """clone / sentinel / restore / snapshot of a step's arrays on the current torch stream; every buffer is allocated up front"""

    def __init__(self, lib, steps, nstreams):
        import torch
        self.lib, self.torch = lib, torch
        self.snap = []                                   # per step: list of uint8 buffers
        biggest = 0
        for st in steps:
            row = []
            for a in st.arrays:
                nb = self.nbytes(a)
                row.append(torch.empty(nb, dtype=torch.uint8, device="cuda"))
                biggest = max(biggest, nb)
            self.snap.append(row)
        nmax = max([len(st.arrays) for st in steps] + [0])
        # clone buffers: one set per stream (a set is free again once the restore queued on that stream has run: stream order)
        self.clone = [[torch.empty(biggest, dtype=torch.uint8, device="cuda") for _ in range(nmax)] for _ in range(nstreams + 1)]
        self.sent = torch.full(((biggest + 3) // 4,), SENTINEL, dtype=torch.float32, device="cuda")

    @staticmethod
    def nbytes(a):
        return a.nfloats * 4 if isinstance(a, Raw) else a.numel() * a.element_size()

    def _d2d(self, dst, src, nb, sp):
        rc = self.lib.wl_d2d(C.c_void_p(dst), C.c_void_p(src), nb, sp)
        assert rc == 0, rc

    def _flat(self, t):
        """the dense memory of a (possibly permuted) tensor as bytes"""
        torch = self.torch
        base = t.permute(*reversed(range(t.dim()))) if (t.dim() > 1 and not t.is_contiguous()) else t
        assert base.is_contiguous()
        return base.reshape(-1).view(torch.uint8)

    def copy_out(self, a, buf, sp):        # array -> buffer
        nb = self.nbytes(a)
        if isinstance(a, Raw):
            self._d2d(buf.data_ptr(), a.getter(), nb, sp)
        else:
            buf[:nb].copy_(self._flat(a))

    def copy_in(self, a, buf, sp):         # buffer -> array
        nb = self.nbytes(a)
        if isinstance(a, Raw):
            self._d2d(a.getter(), buf.data_ptr(), nb, sp)
        else:
            self._flat(a).copy_(buf[:nb])

    def sentinel(self, a, sp):
        nb = self.nbytes(a)
        if isinstance(a, Raw):
            self._d2d(a.getter(), self.sent.data_ptr(), nb, sp)
        else:
            self._flat(a).copy_(self.sent.view(self.torch.uint8)[:nb])


def _stream_ptr(s):
    return C.c_void_p(s.cuda_stream)


def run_baseline(lib, steps):
    """the scenario on the default stream: (per-step array bits, per-step host bits, per-step enqueue time [s], wall time T [s])"""
    import torch
    arr = _Arrays(lib, steps, 0)
    torch.cuda.synchronize()
    host, enq = [], []
    t0 = time.perf_counter()
    for k, st in enumerate(steps):
        ta = time.perf_counter()
        host.append(_host_bits(st.call(None)))
        enq.append(time.perf_counter() - ta)
        for a, buf in zip(st.arrays, arr.snap[k]):
            arr.copy_out(a, buf, None)
    torch.cuda.synchronize()
    T = time.perf_counter() - t0
    return [[b.cpu().numpy() for b in row] for row in arr.snap], host, enq, T


def run_armed(lib, steps, enq, T, nstreams=1, report=None):
    """the scenario on side streams with both arming devices; returns (per-step array bits, per-step host bits); raises NotArmed"""
    import torch
    arr = _Arrays(lib, steps, nstreams)
    delays = [max(MIN_STEP_MS, STEP_FACTOR * 1e3 * e) for e in enq]
    block_ms = max(MIN_BLOCK_MS, BLOCK_FACTOR * 1e3 * T, BLOCK_RUN_FACTOR * (1e3 * T + sum(delays)))
    cycles_per_ms()
    streams = pick_streams(nstreams)
    torch.cuda.synchronize()                    # last touch of the default stream before the blocker
    dflt = torch.cuda.default_stream()
    host = []
    used_default = False
    try:
        sleep_ms(block_ms)                      # default stream blocked
        t_block = time.perf_counter()
        for k, st in enumerate(steps):
            if st.pre is not None:
                st.pre(streams)
            if st.stream < 0:                   # a step on the default stream itself: it runs behind the blocker
                if not used_default and dflt.query():
                    raise NotArmed(f"not armed: the default-stream blocker ({block_ms:.0f} ms) ran out before step {k} ({st.name})")
                used_default = True
                host.append(_host_bits(st.call(None)))
                for a, buf in zip(st.arrays, arr.snap[k]):
                    arr.copy_out(a, buf, None)
                continue
            S = streams[st.stream]
            sp = _stream_ptr(S)
            with torch.cuda.stream(S):
                cl = arr.clone[st.stream]
                t_a = time.perf_counter()
                for a, buf in zip(st.arrays, cl):
                    arr.copy_out(a, buf, sp)
                t_copy = time.perf_counter() - t_a       # the restore below costs the host as much: the delay has to outlast it as well
                for a in st.arrays:
                    arr.sentinel(a, sp)
                S.synchronize()
                delays[k] = max(delays[k], STEP_FACTOR * 1e3 * t_copy)
                sleep_ms(delays[k])
                for a, buf in zip(st.arrays, cl):
                    arr.copy_in(a, buf, sp)
                host.append(_host_bits(st.call(sp)))
                if not st.sync and S.query():
                    raise NotArmed(f"not armed: step {k} ({st.name}) returned with nothing left on its stream (delay {delays[k]:.1f} ms)")
                for a, buf in zip(st.arrays, arr.snap[k]):
                    arr.copy_out(a, buf, sp)
            if not used_default and dflt.query():
                raise NotArmed(f"not armed: the default-stream blocker ({block_ms:.0f} ms) was over after step {k} ({st.name}), "
                               f"{1e3 * (time.perf_counter() - t_block):.0f} ms after it was queued (this step took {1e3 * (time.perf_counter() - t_a):.1f} ms)")
        for S in streams:
            S.synchronize()
        if not used_default and dflt.query():
            raise NotArmed(f"not armed: the default-stream blocker ({block_ms:.0f} ms) ran out before the scenario ended")
    finally:
        torch.cuda.synchronize()                # drain the default stream (and everything else) before anyone goes on
    if report is not None:
        report.update(T_ms=1e3 * T, block_ms=block_ms, delays_ms=(min(delays), max(delays)), armed=True)
    return [[b.cpu().numpy() for b in row] for row in arr.snap], host


def run_on_streams(lib, make, nstreams=1, label=""):
    """make() -> (steps, keep): a fresh scenario (its tensors and handles created and synchronised on the default stream; `keep` holds what must
    outlive the run).  Runs it on the default stream, then armed on side streams, and asserts that every array after every step and every
    host scalar has the same bits.  Returns the report of the armed run."""
    warm, keep0 = make()                        # lazy initialisation (code objects, workspaces, auxiliary streams) stays out of the timings
    run_baseline(lib, warm)
    del warm, keep0
    steps, keep = make()
    base_arr, base_host, enq, T = run_baseline(lib, steps)
    steps2, keep2 = make()
    assert [s.name for s in steps2] == [s.name for s in steps]
    report = {}
    arm_arr, arm_host = run_armed(lib, steps2, enq, T, nstreams, report)
    bad = []
    for k, st in enumerate(steps):
        if base_host[k] != arm_host[k]:
            bad.append(f"step {k} {st.name}: host scalars differ")
        for q, (a, b) in enumerate(zip(base_arr[k], arm_arr[k])):
            if not np.array_equal(a, b):
                what = st.arrays[q].name if isinstance(st.arrays[q], Raw) else f"array {q}"
                bad.append(f"step {k} {st.name}: {what} differs in {int((a != b).sum())} of {a.size} bytes")
    assert report.get("armed")
    print(f"[streams] {label}: armed, {len(steps)} steps, T = {report['T_ms']:.1f} ms, blocker {report['block_ms']:.0f} ms, "
          f"step delays {report['delays_ms'][0]:.1f}–{report['delays_ms'][1]:.1f} ms")
    assert not bad, f"{label}: " + "; ".join(bad[:8])
    del keep, keep2
    return report
