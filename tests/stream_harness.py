"""Harness of tests/test_gpu_streams.py: runs one library call (or a chain of calls) on a non-blocking stream behind a
delay, and captures it in a graph that is replayed on new data.  Plain helper module, no tests.

A Case names its device buffers and says how to call the library on them and what must come out:

  inputs   {name: [a0, a1, a2]}  three value sets per buffer the call reads (or adds to), numpy arrays in the buffer's type
  outputs  {name: (dtype, n)}    buffers the call only writes
  call(bufs, stream)             enqueues the library call(s) on `stream`; bufs[name] are torch tensors on the GPU
  check(k, got, ret)             asserts: got[name] are the buffers on the host after the call ran on value set k, ret is
                                 what call returned (the host result of a blocking call)

Value set 2 is the warm-up (first-call allocations, code-object loads), sets 0 and 1 are what the tests compare."""
import time

import numpy as np

import pymfgpu as mf

NSETS = 3
MIN_DELAY_MS = 50.0  # see the docstring of test_gpu_streams.py for the measured enqueue times behind this choice
ENQUEUE_MS = {}      # case name -> wall clock from the first enqueue to the return of the call (ordered runs)

_torch = None
_cycles_per_ms = None


def torch():
    global _torch
    if _torch is None:
        import torch as t
        _torch = t
    return _torch


def sets(make, seed):
    """NSETS value sets: make(rng) for three seeds"""
    return [make(np.random.default_rng(1000 * seed + k)) for k in range(NSETS)]


class Case:
    def __init__(self, name, inputs, outputs, call, check, offset=0, blocking=False):
        self.name, self.inputs, self.outputs, self.call, self.check = name, inputs, outputs, call, check
        self.offset, self.blocking = offset, blocking
        self.on_run = None  # on_run(k): told after every execution on value set k (cases whose handle keeps state)
        for vals in inputs.values():
            assert len(vals) == NSETS

    def alloc(self):
        """(bufs, stage): NaN-filled device buffers (views `offset` elements into their allocation) and the value sets on
        the device"""
        t = torch()
        dev = t.device("cuda", 0)
        bufs, stage = {}, {}
        for name, vals in self.inputs.items():
            a = np.ascontiguousarray(vals[0])
            bufs[name] = t.full((a.size + self.offset,), float("nan"), device=dev, dtype=t.from_numpy(a).dtype)[self.offset:]
            stage[name] = [t.from_numpy(np.ascontiguousarray(v).reshape(-1)).to(dev) for v in vals]
        for name, (dtype, n) in self.outputs.items():
            td = t.from_numpy(np.zeros(1, dtype=dtype)).dtype
            bufs[name] = t.full((n + self.offset,), float("nan"), device=dev, dtype=td)[self.offset:]
        return bufs, stage

    def ran(self, k):
        if self.on_run:
            self.on_run(k)

    def host(self, bufs):
        return {name: b.cpu().numpy() for name, b in bufs.items()}


def delay_cycles(ms):
    """torch.cuda._sleep cycles for `ms` milliseconds, from one timed _sleep per process"""
    global _cycles_per_ms
    t = torch()
    if _cycles_per_ms is None:
        probe = 20_000_000
        t.cuda._sleep(1000)  # (loads the kernel)
        t.cuda.synchronize()
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record()
        t.cuda._sleep(probe)
        e1.record()
        t.cuda.synchronize()
        took = e0.elapsed_time(e1)
        assert took > 1.0, f"torch.cuda._sleep({probe}) took {took} ms: no usable delay"
        _cycles_per_ms = probe / took
        print(f"calibration: _sleep({probe}) = {took:.2f} ms, {_cycles_per_ms:.0f} cycles per ms")
    return int(ms * _cycles_per_ms)


def fill_nan(bufs):
    for b in bufs.values():
        b.fill_(float("nan"))


def warm_up(case, bufs, stage):
    """the call once, eagerly, on value set 2: first-call allocations and code-object loads happen here"""
    t = torch()
    for name in case.inputs:
        bufs[name].copy_(stage[name][2])
    t.cuda.synchronize()
    s = t.cuda.Stream()
    with t.cuda.stream(s):
        case.call(bufs, s.cuda_stream)
    t.cuda.synchronize()
    case.ran(2)


def runs_beside(busy_stream, other_stream):
    """does a kernel on other_stream run while busy_stream is busy?  Streams share a few hardware queues: two streams on
    the same queue are serialised by the hardware whatever their flags say."""
    t = torch()
    t.cuda.synchronize()
    slept, done = t.cuda.Event(), t.cuda.Event()
    scratch = _probe_scratch()
    with t.cuda.stream(busy_stream):
        t.cuda._sleep(delay_cycles(5.0))
        slept.record(busy_stream)
    with t.cuda.stream(other_stream):
        scratch.add_(1.0)
        done.record(other_stream)
    done.synchronize()
    beside = not slept.query()
    t.cuda.synchronize()
    return beside


_scratch = None
_streams = None


def _probe_scratch():
    global _scratch
    if _scratch is None:
        _scratch = torch().zeros(64, device=torch().device("cuda", 0))
    return _scratch


def ordering_streams():
    """Two non-blocking streams (S1, S2) on which the ordering checks run, found once per process by probing: work on the
    null stream runs beside a busy S1 and beside a busy S2, and S1 and S2 run beside each other.  So they sit on hardware
    queues of their own, and ANY other stream -- the null stream, a handle's side stream -- is on a different queue than
    at least one of them: a launch that is not ordered behind the caller's stream cannot hide behind the delay in both
    runs.  (torch.cuda.Stream() hands out streams of a pool; in a long process a fresh one may share the null stream's
    hardware queue, where the control would see the null-stream call wait for the delay.)"""
    global _streams
    if _streams is None:
        t = torch()
        delay_cycles(1.0)  # (calibrates on the first call)
        null = t.cuda.default_stream()
        found, tried = [], []
        for _ in range(32):
            s = t.cuda.Stream()
            tried.append(s)  # (kept, so that the next one is another stream of the pool)
            if runs_beside(s, null) and all(runs_beside(s, f) and runs_beside(f, s) for f in found):
                found.append(s)
                if len(found) == 2:
                    break
        assert len(found) == 2, (f"found {len(found)} stream(s) that run beside the null stream and each other among "
                                 f"{len(tried)}: the ordering cannot be tested on this device configuration")
        print(f"ordering streams: the {[tried.index(f) + 1 for f in found]}th streams tried")
        _streams = tuple(found)
    return _streams


def run_behind_delay(case, bufs, stage, k, S, stream_of_call="S", delay_ms=MIN_DELAY_MS):
    """Steps 1-3 of the ordering check on value set k.  Everything is NaN and the device idle; then, on the non-blocking
    stream S and without a host synchronisation: the delay, the copies that produce the inputs, the call.  Only S is
    synchronised.  Returns (ret, delay_was_running): whether the delay was still running when the call returned, i.e.
    whether a launch on any other stream had the chance to overtake the inputs.
    stream_of_call = None hands the call the null stream instead of S (the control)."""
    t = torch()
    fill_nan(bufs)
    t.cuda.synchronize()
    slept = t.cuda.Event()
    cycles = delay_cycles(delay_ms)
    with t.cuda.stream(S):
        t0 = time.perf_counter()
        t.cuda._sleep(cycles)
        slept.record(S)
        for name in case.inputs:
            bufs[name].copy_(stage[name][k])
        ret = case.call(bufs, S.cuda_stream if stream_of_call == "S" else None)
        t1 = time.perf_counter()
        running = not slept.query()
    S.synchronize()
    ENQUEUE_MS[case.name] = max(ENQUEUE_MS.get(case.name, 0.0), (t1 - t0) * 1e3)
    print(f"enqueue {case.name}: {(t1 - t0) * 1e3:.3f} ms (delay {delay_ms:.0f} ms, still running at return: {running})")
    return ret, running


def check_ordered(case):
    """the call behind the delay gives the reference for the inputs produced behind the delay, on both ordering streams"""
    bufs, stage = case.alloc()
    warm_up(case, bufs, stage)
    for S in ordering_streams():
        for delay_ms in (MIN_DELAY_MS, 8 * MIN_DELAY_MS):
            ret, running = run_behind_delay(case, bufs, stage, 0, S, delay_ms=delay_ms)
            case.check(0, case.host(bufs), ret)
            case.ran(0)
            if running or case.blocking:  # (a blocking call returns after the delay by design)
                break
        else:  # the host was too slow twice: the run proved nothing about ordering
            raise AssertionError(f"{case.name}: the delay was over before the call returned; the ordering was not tested")


def check_graph(case):
    """warm up eagerly, capture once, replay on value sets 0 and 1 with the outputs refilled with NaN: each replay
    against the reference of ITS inputs"""
    t = torch()
    assert not case.blocking
    bufs, stage = case.alloc()
    warm_up(case, bufs, stage)
    g = t.cuda.CUDAGraph()
    with t.cuda.graph(g):
        case.call(bufs, t.cuda.current_stream().cuda_stream)
    for k in (0, 1):
        fill_nan(bufs)
        for name in case.inputs:
            bufs[name].copy_(stage[name][k])
        g.replay()
        t.cuda.synchronize()
        case.check(k, case.host(bufs), None)
        case.ran(k)


def dvec(tensor, nt):
    """DeviceVector view of a torch tensor (never freed by the view)"""
    return mf.DeviceVector.view(tensor.data_ptr(), tensor.numel(), nt)
