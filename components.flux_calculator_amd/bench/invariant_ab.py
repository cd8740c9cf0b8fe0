"""FCX_OPT_ATMOS_INVARIANT on against off, measured in one process (measurement tool).

One rank has no neighbour, so the boundaries are forced: the engines' first atmosphere cell is
boundary 0 and their last one boundary 1 of a 2-boundary region (left = 0, right = 1,
max_terms = the map's longest segment).  A step is the flux launch (fcx_run_group of the three
T = 1 variants CCLM, MOM5 and RCO; fcx_run of the T = 2 engine), the terms launch the option
adds, and fcx_atmos_finish of every engine -- everything of a step but the all-reduce itself,
whose cost with the wider message needs several GPUs and is NOT measured here.  The arms are two
sets of engines built as bench.py builds them (host arrays, engine-owned mirrors uploaded once,
one stream); sets alternate their order; wall clock per step over REPS steps, medians over the
sets.  Each arm has its own mirrors, and where a 10M-cell engine's mirrors land in HBM moves its
step by more than the option does: run it a second time with `on_first`, which allocates the
"on" arm's engines first, and read the two runs together.  Both arms' atmosphere outputs are
compared bit for bit (one rank: the forced boundary cells are whole, so on and off must agree).
  python invariant_ab.py [SETS] [on_first] [what ...]     what: t1_32768 t1_10000000 t2_10000000"""
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "components.flux_calculator_amd", "python"))
import numpy as np
import torch
from fcx.basic import PHASE_ALL
from fcx.engine import Engine, run_group
from fcx.parallel import BlockedRandomAtmosMap
from fcx.synthetic import build_case, inputs_for_bench

SETS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
ON_FIRST = "on_first" in sys.argv[2:]  # build the "on" arm's engines (and mirrors) first
WHAT = [w for w in sys.argv[2:] if w != "on_first"] or ["t1_32768", "t1_10000000", "t2_10000000"]
FIELDS = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))


# the engines as bench.py builds them (fcx.workload): host arrays, engine-owned mirrors uploaded
# once before any timed region, the atmosphere outputs engine-owned too
OPTS = {"atmos_in_run": 0, "timing": 0, "host_staging": 0}


def arm(cases, la, T, invariant):
    """the engines of one arm over the cases' host arrays, their outputs and adjacent regions"""
    stride = len(FIELDS) * ((1 + la.max_terms) if invariant else 1)
    region = torch.zeros(len(cases) * la.n_boundaries * stride, dtype=torch.float64, device="cuda:0")
    engines, outs = [], []
    for i, case in enumerate(cases):
        o = {f: np.zeros(la.n_atmos) for f, _ in FIELDS}
        atmos = {"local": la, "fields": [(2, 1 if T == 1 else 0, g, f, o[f]) for f, g in FIELDS],
                 "shared": (region[i * la.n_boundaries * stride:], stride), "invariant": invariant}
        e = Engine(case.lf, T, case.methods, corrections=case.corrections, averages=case.averages if T > 1 else (),
                   atmos=atmos, options=OPTS, stream=torch.cuda.current_stream().cuda_stream)  # one stream: fcx_run_group merges
        e.upload(PHASE_ALL)
        engines.append(e)
        outs.append(o)
    return engines, outs


def step_of(engines, t):
    def fn():
        if len(engines) > 1:
            run_group(engines, PHASE_ALL, t)
        else:
            engines[0].run(PHASE_ALL, t)
        for e in engines:
            e.atmos_finish()
    return fn


def measure(what):
    kind, n = what.split("_")
    n, T = int(n), 1 if kind == "t1" else 2
    if T == 1:
        data = inputs_for_bench(n)
        cases = [build_case(v, n=n, T=1, bias=False, data=data) for v in ("CCLM", "MOM5", "RCO")]
    else:
        cases = [build_case("CCLM", n=n, T=2, bias=False)]
    la = BlockedRandomAtmosMap().local(0, n, 0, 1, n)  # bench.py's default map: runs of 3..5 in random order
    k = int(np.bincount(la.atmos_index).max())
    la = dataclasses.replace(la, left=0, right=1, n_boundaries=2, max_terms=k, left_pos=0)
    arms = {name: arm(cases, la, T, name == "on") for name in (("on", "off") if ON_FIRST else ("off", "on"))}
    reps = 200 if n <= 1_000_000 else 30
    ms = {name: [] for name in arms}
    try:
        for s in range(SETS):
            for name in (list(arms) if s % 2 == 0 else list(arms)[::-1]):
                fn = step_of(arms[name][0], 3600)
                for _ in range(10):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) / reps * 1e3)
        for engines, _ in arms.values():
            for e in engines:
                e.download(PHASE_ALL)
                e.synchronize()
        same = all(np.array_equal(a[f].view(np.uint64), b[f].view(np.uint64))
                   for a, b in zip(arms["off"][1], arms["on"][1]) for f, _ in FIELDS)
        fused = [bool(e.fused_accumulation(PHASE_ALL)) for e in arms["on"][0]]
        groups = [e.last_group_size() for e in arms["on"][0]]
        terms = [e.last_terms_group() for e in arms["on"][0]]  # engines per terms launch (one launch: 3, 3, 3)
        assert terms == [len(cases)] * len(cases) and all(e.last_terms_group() == 0 for e in arms["off"][0]), terms
    finally:
        for engines, _ in arms.values():
            for e in engines:
                e.close()
    med = {name: float(np.median(v)) for name, v in ms.items()}
    return {"what": what, "on_first": ON_FIRST, "cells": n, "types": T, "engines": len(cases), "max_terms": k, "reps": reps,
            "group_sizes": groups, "terms_group": terms, "fused_accumulation": fused, "outputs_bit_identical": bool(same),
            "ms_sets": ms, "ms_median": med, "ms_range": {name: [min(v), max(v)] for name, v in ms.items()},
            "on_minus_off_us": (med["on"] - med["off"]) * 1e3, "on_over_off": med["on"] / med["off"],
            "slot_doubles": {"off": len(cases) * 2 * len(FIELDS), "on": len(cases) * 2 * len(FIELDS) * (1 + k)}}


def main():
    out = {"sets": SETS, "results": []}
    for what in WHAT:
        out["results"].append(measure(what))
        print(json.dumps(out["results"][-1]), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
