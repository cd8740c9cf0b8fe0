"""What FCX_OPT_CR_MATH costs: the fp64 engine with the device library's exp / log against the same
engine with the correctly rounded functions, in one process (measurement tool, after
precision_ab.py).

Each case is built once; for every set and arm a fresh set of engines is made over the SAME
arrays, run and closed again before the next, the arms' order alternating from set to set.
  t1_group  the T = 1 three-variant group step (CCLM + MOM5 + RCO, 10M cells, random map, the
            fused accumulation), device-resident
  t2_group  the T = 2 group step, the type-0 averages accumulated in the one group launch
  baltic    the Baltic-size host step (MOM5_BALTIC set-up, 32,768 cells per grid, caller heap
            arrays, early + normal phase through fcx_step); wall clock
The device cases are event-timed fcx_run_group calls over uploaded inputs.  Reported per arm: the
median ms per launch of every set, the sets' range, Mcells/s of the median (cells x engines per
launch), fcx_algorithmic_bytes summed over the engines (the same in both arms: the option
changes arithmetic only), and the ratio cr / default of the medians.
  python cr_math_ab.py [SETS] [CELLS] [CASES, comma-separated: t1_group,t2_group,baltic]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "components.flux_calculator_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import namelists
from fcx.basic import PHASE_ALL, PHASE_EARLY, PHASE_NORMAL
from fcx.engine import Engine, run_group
from fcx.parallel import BlockedRandomAtmosMap
from fcx.setup import setup_from_namelist
from fcx.synthetic import SyntheticCoupler, build_case, corrections, inputs_for_bench

VARIANTS = ("CCLM", "MOM5", "RCO")
FIELDS = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))
SETS = int(sys.argv[1]) if len(sys.argv) > 1 else 4
N = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
KINDS = tuple(sys.argv[3].split(",")) if len(sys.argv) > 3 else ("t1_group", "t2_group", "baltic")
WARM, TIMED = 30, 100
ARMS = ("default", "cr_math")
stream = torch.cuda.current_stream()


def arm_options(arm):
    return {"cr_math": 1 if arm == "cr_math" else 0}


def device_case(kind, la, host):
    T = 2 if kind == "t2_group" else 1
    cases = [build_case(v, n=N, T=T, data=host if T == 1 else None) for v in VARIANTS]
    outs = [{name: np.empty(la.n_atmos) for name, _ in FIELDS} for _ in VARIANTS]

    def run(arm):
        engines = []
        try:
            for c, o in zip(cases, outs):
                engines.append(Engine(c.lf, T, c.methods, corrections=c.corrections, averages=c.averages, device=0,
                                      stream=stream.cuda_stream,
                                      atmos={"local": la, "fields": [(PHASE_NORMAL, 0 if T == 2 else 1, g, name, o[name])
                                                                      for name, g in FIELDS]},
                                      options={"atmos_in_run": 0, "timing": 0, "host_staging": 0, "pipeline_chunks": 1,
                                               **arm_options(arm)}))
            for e in engines:
                e.upload(PHASE_ALL)

            def step(k):
                run_group(engines, PHASE_ALL, 3600 * k)
                for e in engines:
                    e.run_atmos(PHASE_ALL)  # (a no-op where the accumulation rode in the launch)
            for k in range(WARM):
                step(k)
            torch.cuda.synchronize()
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(TIMED)]
            for k, (a, b) in enumerate(evs):
                a.record(stream)
                step(k)
                b.record(stream)
            torch.cuda.synchronize()
            ms = np.array([a.elapsed_time(b) for a, b in evs])
            facts = {"bytes": sum(e.algorithmic_bytes(PHASE_ALL) for e in engines),
                     "group": [e.last_group_size() for e in engines], "cr_math": [e.cr_math() for e in engines],
                     "cells": N * len(engines)}
            return float(np.median(ms)), facts
        finally:
            for e in engines:
                e.close()
            torch.cuda.empty_cache()
    return run


def baltic_case():
    grids = (32768, 32768, 32768)
    regrid = namelists.regrid_matrices(grids)
    corr = (20000101, corrections(grids[0]))
    s = setup_from_namelist(namelists.MOM5_BALTIC, mype=0, grid_size=grids, dtype="float64")
    coupler = SyntheticCoupler.for_setup(s)
    for f in s.input_field:  # one set of received fields; the timed loop is the engine's part of a step
        coupler.get(f.name, 0, s.local_field.field[f.slot])

    def run(arm):
        eng = s.engine(corrections=corr, regrid=regrid, options=arm_options(arm))
        try:
            def step(k):
                eng.step(PHASE_EARLY, 600 * k)
                eng.step(PHASE_NORMAL, 600 * k)
            for k in range(WARM):
                step(k)
            t = []
            for k in range(TIMED):
                t0 = time.perf_counter()
                step(k)
                t.append((time.perf_counter() - t0) * 1e3)
            facts = {"bytes": eng.algorithmic_bytes(PHASE_ALL), "cr_math": [eng.cr_math()],
                     "zero_copy_bytes": eng.zero_copy_bytes(), "staging_bytes": eng.staging_bytes(), "cells": grids[0]}
            return float(np.median(t)), facts
        finally:
            eng.close()
    return run


def main():
    la = BlockedRandomAtmosMap().local(0, N, 0, 1, N)
    host = inputs_for_bench(N)
    report = {"n": N, "sets": SETS, "warm": WARM, "timed": TIMED, "arms": ARMS, "cases": {}}
    for kind in KINDS:
        run = baltic_case() if kind == "baltic" else device_case(kind, la, host)
        ms = {a: [] for a in ARMS}
        facts = {}
        for s in range(SETS):
            r = s % len(ARMS)
            for arm in ARMS[r:] + ARMS[:r]:
                m, facts[arm] = run(arm)
                ms[arm].append(round(m, 4))
                print(f"{kind} set {s} {arm}: median {m:.4f} ms per {'step' if kind == 'baltic' else 'launch'}", flush=True)
        summary = {}
        for arm in ARMS:
            r = ms[arm]
            med = float(np.median(r))
            summary[arm] = {"median_ms": round(med, 4), "min_ms": min(r), "max_ms": max(r),
                            "mcells_per_s": round(facts[arm]["cells"] / med / 1e3, 1)}
            print(f"{kind} {arm}: median of sets {med:.4f} ms, sets {min(r):.4f}..{max(r):.4f}, "
                  f"{summary[arm]['mcells_per_s']} Mcells/s, {facts[arm]}", flush=True)
        ratio = summary["cr_math"]["median_ms"] / summary["default"]["median_ms"]
        print(f"{kind}: cr_math / default = {ratio:.3f}", flush=True)
        report["cases"][kind] = {"ms": ms, "summary": summary, "facts": facts, "ratio": round(ratio, 4)}
        del run
    print(json.dumps(report))


if __name__ == "__main__":
    main()
