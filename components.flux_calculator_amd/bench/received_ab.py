"""Received fields declared against the undeclared twin in one process (measurement tool,
fcx_bind_received).

The CCLM step (T = 1, bias) from host arrays through fcx_step: the eight atmosphere inputs are
either exchange-grid arrays the host expanded (undeclared) or model-grid sources the engine
gathers (declared; intersection-grid map, runs of 4-9 exchange cells per atmosphere cell, unit
weights).  For every set and arm a fresh engine is made over the SAME arrays, run and closed
before the next, the arms' order rotating from set to set.  Reported per memory kind (caller
heap arrays, fcx_host_malloc arrays) and arm: the median wall-clock ms per step of every set and
the sets' range, the bytes one step uploads over the host link, fcx_algorithmic_bytes; and for
the declared arm the gather launch alone (sources in device memory, so fcx_receive is the launch
only; HIP events around a block of them): ms per launch and its algorithmic bytes per second
against the 6.29 TB/s float4 copy.
  python received_ab.py [SETS] [CELLS]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "components.flux_calculator_amd", "python"))
import numpy as np
import torch
from fcx import host_alloc
from fcx.basic import PHASE_ALL, PHASE_NORMAL
from fcx.engine import Engine
from fcx.synthetic import build_case

ATMOS = ("PSUR", "PATM", "QATM", "TATM", "UATM", "VATM", "AMOI", "AMOM")
READS = ("TSUR", "FICE") + ATMOS  # what the CCLM step uploads
SETS = int(sys.argv[1]) if len(sys.argv) > 1 else 4
N = int(sys.argv[2]) if len(sys.argv) > 2 else 32_768
WARM, TIMED = (20, 100) if N <= 1_000_000 else (3, 10)
COPY_TBS = 6.29
T_STEP = 3600 * 24 * 45


def intersection_map(n, seed=7):
    r = np.random.Generator(np.random.PCG64([seed, n]))
    runs = r.integers(4, 10, n // 4 + 2)
    owner = np.repeat(np.arange(runs.size, dtype=np.int32), runs)[:n]
    return int(owner[-1]) + 1, owner, np.arange(n, dtype=np.int32), np.ones(n)


def build(memory, arena):
    case = build_case("CCLM", n=N, T=1, bias=True)
    n_src, src, dst, w = intersection_map(N)
    alloc = arena.empty if memory == "library" else (lambda k, dt="float64": np.empty(k, dt))
    sources = {}
    for name in ATMOS:  # the model-grid values, and their expansion in the exchange-grid arrays
        a = case.lf.field[(0, 1, name)]
        s = alloc(n_src)
        s[src] = a
        a[:] = 0.0 + s[src]
        sources[name] = s
    if memory == "library":
        arena.adopt(case.lf)
    return case, (n_src, src, dst, w), sources


def engine(case, links, sources, declared):
    n_src, src, dst, w = links
    rec = [{"grid": 1, "n_src": n_src, "src": src, "dst": dst, "w": w,
            "fields": [(PHASE_NORMAL, 0, 1, name, a) for name, a in sources.items()]}] if declared else None
    return Engine(case.lf, 1, case.methods, corrections=case.corrections, received=rec)


def time_steps(eng):
    for _ in range(WARM):
        eng.step(PHASE_ALL, T_STEP)
    t0 = time.perf_counter()
    for _ in range(TIMED):
        eng.step(PHASE_ALL, T_STEP)
    return (time.perf_counter() - t0) / TIMED * 1e3


def gather_alone(case, links, sources):
    dev = {k: torch.as_tensor(np.asarray(a)).to("cuda:0") for k, a in sources.items()}
    stream = torch.cuda.Stream()
    n_src, src, dst, w = links
    rec = [{"grid": 1, "n_src": n_src, "src": src, "dst": dst, "w": w,
            "fields": [(PHASE_NORMAL, 0, 1, name, a) for name, a in dev.items()]}]
    base = Engine(case.lf, 1, case.methods, corrections=case.corrections, stream=stream.cuda_stream)
    eng = Engine(case.lf, 1, case.methods, corrections=case.corrections, received=rec, stream=stream.cuda_stream)
    try:
        nbytes = eng.algorithmic_bytes(PHASE_ALL) - base.algorithmic_bytes(PHASE_ALL)
        reps = 200 if N <= 1_000_000 else 30
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            for _ in range(10):
                eng.receive(PHASE_ALL)
            e0.record(stream)
            for _ in range(reps):
                eng.receive(PHASE_ALL)
            e1.record(stream)
        e1.synchronize()
        ms = e0.elapsed_time(e1) / reps
    finally:
        eng.close()
        base.close()
    return {"gather_ms": ms, "gather_bytes": nbytes, "gather_tb_s": nbytes / (ms * 1e-3) / 1e12,
            "fraction_of_copy": nbytes / (ms * 1e-3) / 1e12 / COPY_TBS}


def main():
    out = {"cells": N, "sets": SETS, "timed_steps": TIMED}
    for memory in ("heap", "library"):
        with host_alloc.Arena() as arena:
            case, links, sources = build(memory, arena)
            n_src = links[0]
            ms = {"undeclared": [], "declared": []}
            info = {}
            for k in range(SETS):
                arms = ("undeclared", "declared") if k % 2 == 0 else ("declared", "undeclared")
                for arm in arms:
                    eng = engine(case, links, sources, arm == "declared")
                    try:
                        ms[arm].append(time_steps(eng))
                        info[arm] = {"algorithmic_bytes": eng.algorithmic_bytes(PHASE_ALL),
                                     "zero_copy_bytes": eng.zero_copy_bytes(), "staging_bytes": eng.staging_bytes()}
                    finally:
                        eng.close()
            es = 8
            h2d = {"undeclared": len(READS) * N * es, "declared": 2 * N * es + len(ATMOS) * n_src * es}
            res = {"n_src": n_src}
            for arm in ms:
                res[arm] = dict(info[arm], step_ms_sets=ms[arm], step_ms_median=float(np.median(ms[arm])),
                                step_ms_range=[min(ms[arm]), max(ms[arm])], host_link_h2d_bytes=h2d[arm])
            if memory == "heap":
                res["gather"] = gather_alone(case, links, sources)
            out[memory] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
