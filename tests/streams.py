"""A stalled side stream: the harness that checks the ordering contract of include/ditherpie_hip.h -- "All work is enqueued
asynchronously on [stream]; the caller synchronises" -- as tests/arena.py checks the memory contract.

Why: on torch's default stream a launch, memset or copy that the library put on stream 0 instead of the caller's stream is
still ordered with everything else a test does, so no value test can see it.  Here every case runs on a fresh
torch.cuda.Stream() (non-blocking: not ordered with the null stream; side_stream() takes one that the hardware also runs
beside it).  A warm run first (values only; it builds lazy tables and the per-stream workspace, and its wall time t_warm
sizes the stall: T = max(20 ms, 4 t_warm)), then twice behind a bounded spin (torch.cuda._sleep: one thread of one wave,
never longer than MAX_STALL_MS):

  A, late input.  The inputs hold a DECOY (a second valid input whose reference output differs), the stream is stalled, and
     behind the stall the stream receives: copies of the real inputs into place, the call, copies of the outputs away.  An
     event E recorded right behind the stall must not have completed when the call returns -- the proof that the call was
     enqueued while its inputs were still the decoy ("vacuous" otherwise; there is no retry).  Whatever part of the call
     went to another stream ran early, on the decoy, and shows in the bytes.
  B, busy default stream.  The real inputs are in place, the DEFAULT stream is stalled, the call and the output copies go
     to the side stream, which is then synchronised.  E, recorded on the default stream behind its stall, must still be
     pending ("waited" otherwise: something in the call waited for the default stream).  Whatever part of the call went to
     stream 0 ran late, so what followed it on the side stream read stale bytes; a mis-placed memset shows only here.

The reference bytes of a case come from the CPU statements of the suite, never from a second run of the library.  A failure
is a StreamOrderError naming the entry point, the variant and which condition failed: "vacuous", "waited" or "bytes".

Kinds: "async" (every condition); "syncs_stream" (the header says the call waits for its stream, or a Python wrapper reads
a size back: A cannot ask for a pending E, B asks for everything); "cold" (the first call with a fresh palette, which the
header allows to allocate, build on the null stream and wait: no warm run, the stall of the matching warm case, bytes only).

What this cannot see: an input-independent operation, such as a memset, that the library places on a THIRD stream that is
neither the caller's nor the null stream; it is ordered with neither stall."""
import gc
import time

import numpy as np
import torch

MAX_STALL_MS = 1000.0
MIN_STALL_MS = 20.0
STALL_FACTOR = 4.0          # T = max(MIN_STALL_MS, STALL_FACTOR * t_warm)
KINDS = ("async", "syncs_stream", "cold")

STATS = []                  # one dict per finished case: entry, label, kind, t_warm_ms, T_ms, slack_A_ms, slack_B_ms
_cycles_per_ms = None


class StreamOrderError(AssertionError):
    """entry: the entry point; variant: "warm", "A" or "B"; condition: "vacuous", "waited", "bytes" or "shrink the case"."""

    def __init__(self, entry, variant, condition, detail=""):
        super().__init__(f"stream order: {entry}, variant {variant}: {condition}" + (f" -- {detail}" if detail else ""))
        self.entry, self.variant, self.condition, self.detail = entry, variant, condition, detail


def cycles_per_ms():
    """Spin cycles of torch.cuda._sleep per millisecond: the median of three short sleeps timed with events, once a session."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        probe = 2_000_000
        torch.cuda._sleep(probe)                                  # (first use: not timed)
        torch.cuda.synchronize()
        rates = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(probe)
            b.record()
            b.synchronize()
            rates.append(probe / max(a.elapsed_time(b), 1e-3))
        _cycles_per_ms = float(sorted(rates)[1])
    return _cycles_per_ms


_beside_default = {}       # cuda_stream -> does the hardware run this stream beside the default stream


def side_stream():
    """A fresh non-blocking stream that the device really runs beside the default stream.  HIP multiplexes its streams onto a
    few hardware queues; a stream that shares its queue with the null stream is serialised behind whatever the null stream
    runs, however non-blocking it is, and variant B could tell nothing on it.  A short probe (a 5 ms stall on the default
    stream, one fill on the candidate) decides, once per stream; a machine without any such stream fails here."""
    probe = torch.zeros(64, dtype=torch.uint8, device="cuda")
    held = []
    for _ in range(32):
        s = torch.cuda.Stream()
        held.append(s)
        ok = _beside_default.get(s.cuda_stream)
        if ok is None:
            with torch.cuda.stream(s):
                probe.fill_(1)                                   # (first use of the stream: not part of the probe)
            torch.cuda.synchronize()
            stall(5.0)
            E = torch.cuda.Event()
            E.record()
            with torch.cuda.stream(s):
                probe.fill_(2)
                s.synchronize()
            ok = _beside_default[s.cuda_stream] = not E.query()
            torch.cuda.synchronize()
        if ok:
            return s
    raise StreamOrderError("harness", "B", "waited", "no side stream runs beside the default stream on this device")


def stall(ms):
    """A spin of `ms` milliseconds on the current stream: one thread of one wave; refused beyond MAX_STALL_MS."""
    ms = float(ms)
    if not 0.0 <= ms <= MAX_STALL_MS:
        raise ValueError(f"a stall of {ms} ms is outside 0 .. {MAX_STALL_MS}")
    if ms > 0.0:
        torch.cuda._sleep(max(1, int(ms * cycles_per_ms())))


_AS_SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def to_device(a):
    """A numpy array as a contiguous CUDA tensor (unsigned 16 / 32 / 64-bit arrays travel as their signed bit patterns); a
    CUDA tensor (a large input that was made on the device) is copied."""
    if isinstance(a, torch.Tensor):
        return a.detach().cuda().contiguous().clone()
    a = np.ascontiguousarray(a)
    if a.dtype in _AS_SIGNED:
        a = a.view(_AS_SIGNED[a.dtype])
    return torch.from_numpy(a.copy()).cuda()


def _bytes(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous().view(torch.uint8).numpy() if x.numel() else np.zeros(0, np.uint8)
    return np.ascontiguousarray(x).reshape(-1).view(np.uint8)


def _differs(a, b):
    a, b = _bytes(a), _bytes(b)
    return a.size != b.size or not np.array_equal(a, b)


class Case:
    """One call under test.

    entry    the entry point the case is about (the name a failure carries)
    inputs   name -> (real, decoy): numpy arrays (or CUDA tensors) of one shape and dtype; they become device tensors at fixed
             addresses
    ref      name -> numpy array: the reference output for the real inputs (from the CPU statements)
    decoy_ref  name -> numpy array: the reference output for the decoy inputs; at least one must differ from `ref` (checked
             on the host).  A case without inputs has none.
    call(inp, outs, state) -> name -> CUDA tensor: runs under `with torch.cuda.stream(s)`; inp: name -> the device tensor in
             place; outs: name -> preallocated output tensors (see `outs`); state: what prepare() returned
    outs     name -> (shape, torch dtype): outputs the harness allocates, fills before every run and hands to call()
    norm(got) -> name -> numpy: got: name -> numpy array of every tensor call() returned; -> what is compared with `ref`
             (default: the arrays themselves; for outputs with unspecified bytes)
    prepare(variant) -> state: host-side set-up before a run ("warm", "A", "B"), with the device idle: a fresh palette for a
             cold case, a reset of a resident object
    kind     "async", "syncs_stream" or "cold"
    T_ms     the stall of a cold case (that of the matching warm case); force_T_ms overrides the rule (controls only)"""

    def __init__(self, entry, inputs, ref, call, decoy_ref=None, outs=None, norm=None, prepare=None, kind="async", T_ms=None,
                 force_T_ms=None, label=""):
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}")
        if kind == "cold" and T_ms is None:
            raise ValueError("a cold case takes the stall of its warm case (T_ms)")
        self.entry, self.inputs, self.ref, self.call, self.decoy_ref = entry, inputs, ref, call, decoy_ref
        self.outs, self.norm, self.prepare, self.kind, self.T_ms, self.force_T_ms, self.label = outs or {}, norm, prepare, kind, T_ms, force_T_ms, label
        for name, (real, decoy) in inputs.items():
            if not isinstance(real, torch.Tensor):
                real, decoy = np.asarray(real), np.asarray(decoy)
            if tuple(real.shape) != tuple(decoy.shape) or real.dtype != decoy.dtype:
                raise ValueError(f"{entry}: decoy of '{name}' is not of the real input's shape and dtype")
        if inputs:
            if not decoy_ref:
                raise ValueError(f"{entry}: a case with inputs needs the reference output of its decoy")
            if not any(_differs(ref[k], decoy_ref[k]) for k in decoy_ref):
                raise ValueError(f"{entry}: the decoy's reference output equals the real one: the case could not fail")


def _compare(case, variant, got, place, real):
    arrays = {k: v.detach().cpu().numpy() if v.numel() else np.zeros(tuple(v.shape), np.uint8) for k, v in got.items()}
    seen = case.norm(arrays) if case.norm else arrays
    for name, want in case.ref.items():
        a, b = _bytes(seen[name]), _bytes(want)
        if a.size != b.size:
            raise StreamOrderError(case.entry, variant, "bytes", f"'{name}' has {a.size} bytes, the reference {b.size} {case.label}")
        if not np.array_equal(a, b):
            bad = np.nonzero(a != b)[0]
            raise StreamOrderError(case.entry, variant, "bytes", f"'{name}': {len(bad)} bytes differ from the reference, first at {int(bad[0])} {case.label}")
    for name in place:
        if not torch.equal(place[name], real[name]):
            raise StreamOrderError(case.entry, variant, "bytes", f"the input '{name}' was changed {case.label}")


def _fill(tensors, byte):
    for t in tensors.values():
        if t.numel():
            t.view(torch.uint8).fill_(byte)


def run_case(case, variants=("A", "B")):
    """Warm run, variant A, variant B (see the module docstring) -> the case's entry in STATS."""
    gc.collect()              # a palette or threshold object that dies inside a stalled window frees device memory, which waits
    s = side_stream()
    real = {k: to_device(v[0]) for k, v in case.inputs.items()}
    decoy = {k: to_device(v[1]) for k, v in case.inputs.items()}
    place = {k: torch.empty_like(v) for k, v in real.items()}
    outs = {k: torch.empty(shape, dtype=dt, device="cuda") for k, (shape, dt) in case.outs.items()}
    res = None
    stat = dict(entry=case.entry, label=case.label, kind=case.kind, t_warm_ms=None, T_ms=None, slack_A_ms=None, slack_B_ms=None)

    def put(src, byte):
        for k in place:
            place[k].copy_(src[k])
        _fill(outs, byte)
        if res is not None:
            _fill(res, byte)

    def poison(got, byte):
        # the tensors a wrapper allocated go back to the stream's pool: the next run's outputs must not find this run's result there
        for k, t in got.items():
            if k not in outs and t.numel() and t.is_contiguous():
                t.view(torch.uint8).fill_(byte)

    # ---- warm run
    if case.kind != "cold":
        state = case.prepare("warm") if case.prepare else None
        put(real, 0x11)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            t0 = time.perf_counter()
            got = case.call(place, outs, state)
            s.synchronize()
            t_warm = (time.perf_counter() - t0) * 1e3
            torch.cuda.synchronize()   # the warm run asks for the values only: work on a wrong stream is for A and B to tell
            _compare(case, "warm", got, place, real)
            res = {k: torch.empty_like(t) for k, t in got.items()}
            poison(got, 0x11)
            s.synchronize()
        del got
        T = max(MIN_STALL_MS, STALL_FACTOR * t_warm) if case.force_T_ms is None else float(case.force_T_ms)
        if T > MAX_STALL_MS:
            raise StreamOrderError(case.entry, "warm", "shrink the case", f"the warm run took {t_warm:.1f} ms {case.label}")
        stat["t_warm_ms"] = t_warm
    else:
        T = float(case.T_ms)
    stat["T_ms"] = T

    # ---- variant A: late input
    if "A" in variants:
        state = case.prepare("A") if case.prepare else None
        put(decoy, 0x33)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            stall(T)
            E = torch.cuda.Event()
            E.record()
            for k in place:
                place[k].copy_(real[k], non_blocking=True)
            got = case.call(place, outs, state)
            done = E.query()
            t_query = time.perf_counter()
            if res is None:
                res = {k: torch.empty_like(t) for k, t in got.items()}
            for k in got:
                res[k].copy_(got[k], non_blocking=True)
        if case.kind == "async":
            if done:
                raise StreamOrderError(case.entry, "A", "vacuous", f"the stall of {T:.1f} ms was over when the call returned {case.label}")
            E.synchronize()
            stat["slack_A_ms"] = (time.perf_counter() - t_query) * 1e3
        s.synchronize()
        _compare(case, "A", res, place, real)
        with torch.cuda.stream(s):
            poison(got, 0x33)
            s.synchronize()
        del got

    # ---- variant B: busy default stream
    if "B" in variants:
        state = case.prepare("B") if case.prepare else None
        put(real, 0x55)
        torch.cuda.synchronize()
        stall(T)
        E = torch.cuda.Event()
        E.record()
        with torch.cuda.stream(s):
            got = case.call(place, outs, state)
            if res is None:
                res = {k: torch.empty_like(t) for k, t in got.items()}
            for k in got:
                res[k].copy_(got[k], non_blocking=True)
            s.synchronize()
        done = E.query()
        t_query = time.perf_counter()
        if case.kind != "cold":
            if done:
                raise StreamOrderError(case.entry, "B", "waited", f"the default stream's stall of {T:.1f} ms was over when the side stream was done {case.label}")
            E.synchronize()
            stat["slack_B_ms"] = (time.perf_counter() - t_query) * 1e3
        _compare(case, "B", res, place, real)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            poison(got, 0x55)
            s.synchronize()
        del got
    torch.cuda.synchronize()
    STATS.append(stat)
    return stat


def summary():
    """-> (smallest slack in ms, its share of that case's T, the case; largest t_warm in ms, its case) over STATS."""
    slacks = [(st[k], st[k] / st["T_ms"], st["entry"] + " " + st["label"]) for st in STATS for k in ("slack_A_ms", "slack_B_ms")
              if st[k] is not None and st["T_ms"]]
    warms = [(st["t_warm_ms"], st["entry"] + " " + st["label"]) for st in STATS if st["t_warm_ms"] is not None]
    return (min(slacks, key=lambda x: x[1]) if slacks else None), (max(warms) if warms else None)
