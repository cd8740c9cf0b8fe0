"""Declared against undeclared outputs in one process (measurement tool, fcx_set_output_use).

Each case is built once; for every set and arm a fresh set of engines is made over the SAME
arrays, run and closed again before the next, the arms' order rotating from set to set (as
lib_ab.py does with builds).  The arms differ in nothing but the declarations.
  t1_qsur   the T = 1 three-variant group step (CCLM + MOM5 + RCO, 10M cells, random map, the
            fused accumulation), QSUR unread (RCO computes none)
  t1_all    the same with every exchange-grid output unread
  t2_types  the T = 2 group step with the per-type MEVA / HLAT / HSEN / RBBR unread, the type-0
            averages accumulated
  baltic    the Baltic-size host step (MOM5_BALTIC set-up, 32,768 cells per grid, caller heap
            arrays, early + normal phase through fcx_step) with select_outputs; wall clock
The device cases are event-timed group launches over uploaded inputs; reported per arm: the
median ms per launch of every set, the sets' range, fcx_algorithmic_bytes (summed over the
engines) and what fcx_output_info says of the declared slots.
  python outputs_ab.py [SETS] [CELLS]"""
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
from fcx import _lib
from fcx.basic import PHASE_ALL, PHASE_EARLY, PHASE_NORMAL
from fcx.engine import Engine, run_group
from fcx.parallel import BlockedRandomAtmosMap
from fcx.setup import setup_from_namelist
from fcx.synthetic import SyntheticCoupler, build_case, corrections, inputs_for_bench

VARIANTS = ("CCLM", "MOM5", "RCO")
FIELDS = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))
UNREAD = _lib.FCX_OUT_UNREAD
SETS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
N = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
WARM, TIMED = 30, 100
ARMS = ("undeclared", "declared")
stream = torch.cuda.current_stream()


def declarations(kind, case):
    has_q = case.methods["which_spec_vapor_surface_t"][0] != "none"
    if kind == "t1_qsur":
        return {(1, 1, "QSUR"): UNREAD} if has_q else {}
    if kind == "t1_all":
        use = {(1, g, name): UNREAD for name, g in FIELDS}
        if has_q:
            use[(1, 1, "QSUR")] = UNREAD
        return use
    return {(s, 1, name): UNREAD for s in (1, 2) for name in ("MEVA", "HLAT", "HSEN", "RBBR")}


def device_case(kind, la, host):
    T = 2 if kind == "t2_types" else 1
    cases = [build_case(v, n=N, T=T, data=host if T == 1 else None) for v in VARIANTS]
    outs = [{name: np.empty(la.n_atmos) for name, _ in FIELDS} for _ in cases]

    def run(arm):
        engines = []
        for c, o in zip(cases, outs):
            use = declarations(kind, c) if arm == "declared" else None
            engines.append(Engine(c.lf, T, c.methods, corrections=c.corrections, averages=c.averages, device=0,
                                  stream=stream.cuda_stream, output_use=use,
                                  atmos={"local": la, "fields": [(PHASE_NORMAL, 0 if T == 2 else 1, g, name, o[name])
                                                                  for name, g in FIELDS]},
                                  # (pipeline_chunks 1: the engines are only ever run over the whole grid.
                                  # An engine of host arrays that fcx_step could cut into chunks keeps the
                                  # accumulated fields' stores, since chunk launches carry crossing records.)
                                  options={"atmos_in_run": 0, "timing": 0, "host_staging": 0, "pipeline_chunks": 1}))
        try:
            for e in engines:
                e.upload(PHASE_ALL)
            for k in range(WARM):
                run_group(engines, PHASE_ALL, 3600 * k)
            torch.cuda.synchronize()
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(TIMED)]
            for k, (a, b) in enumerate(evs):
                a.record(stream)
                run_group(engines, PHASE_ALL, 3600 * k)
                b.record(stream)
            torch.cuda.synchronize()
            ms = np.array([a.elapsed_time(b) for a, b in evs])
            facts = {"bytes": sum(e.algorithmic_bytes(PHASE_ALL) for e in engines),
                     "group": [e.last_group_size() for e in engines],
                     "kinds": {v: sorted({e.output_info(*k) for k in e.output_use}) for v, e in zip(VARIANTS, engines)}}
            return float(np.median(ms)), facts
        finally:
            for e in engines:
                e.close()
            torch.cuda.empty_cache()
    return run


def baltic_case():
    grids = (32768, 32768, 32768)
    s = setup_from_namelist(namelists.MOM5_BALTIC, mype=0, grid_size=grids)
    regrid = namelists.regrid_matrices(grids)
    corr = (20000101, corrections(grids[0]))
    coupler = SyntheticCoupler.for_setup(s)
    for f in s.input_field:  # one set of received fields; the timed loop is the engine's part of a step
        coupler.get(f.name, 0, s.local_field.field[f.slot])

    def run(arm):
        eng = s.engine(corrections=corr, regrid=regrid, select_outputs=arm == "declared")
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
            facts = {"bytes": eng.algorithmic_bytes(PHASE_ALL), "unsent": len(eng.output_use),
                     "kinds": sorted({eng.output_info(*k) for k in eng.output_use}),
                     "zero_copy_bytes": eng.zero_copy_bytes(), "staging_bytes": eng.staging_bytes()}
            return float(np.median(t)), facts
        finally:
            eng.close()
    return run


def main():
    la = BlockedRandomAtmosMap().local(0, N, 0, 1, N)
    host = inputs_for_bench(N)
    report = {"n": N, "sets": SETS, "warm": WARM, "timed": TIMED, "cases": {}}
    for kind in ("t1_qsur", "t1_all", "t2_types", "baltic"):
        run = baltic_case() if kind == "baltic" else device_case(kind, la, host)
        ms = {a: [] for a in ARMS}
        facts = {}
        for s in range(SETS):
            order = ARMS[s % 2:] + ARMS[: s % 2]
            for arm in order:
                m, facts[arm] = run(arm)
                ms[arm].append(round(m, 4))
                print(f"{kind} set {s} {arm}: median {m:.4f} ms per {'step' if kind == 'baltic' else 'launch'}", flush=True)
        for arm in ARMS:
            r = ms[arm]
            print(f"{kind} {arm}: median of sets {np.median(r):.4f} ms, sets {min(r):.4f}..{max(r):.4f}, "
                  f"algorithmic bytes {facts[arm]['bytes']}, {facts[arm]}", flush=True)
        report["cases"][kind] = {"ms": ms, "facts": facts}
        del run
    print(json.dumps(report))


if __name__ == "__main__":
    main()
