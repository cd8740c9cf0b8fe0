"""Exact field integrals, measured in one process (measurement tool, fcx_field_integrals).

calls: fcx_field_integrals of 1, 7 and 16 fp64 fields and 7 fp32 fields of a device-resident CCLM
engine after a step -- its seven computed fields first (QSUR, MEVA, HLAT, HSEN, RBBR, UMOM, VMOM),
then received fields, leaving out FICE (mostly zeros, which cost no digit work) and FARE (all
ones) --, weighted and unweighted -- the streaming launch, the finishing launch, the 576 B per field
copy and the wait -- as wall-clock per call, with its algorithmic bytes per second (the fields,
plus 8 B of area per cell and field when weighted: the range call reads half of that in fp64);
beside it fcx_field_ranges over the same slots in the same process.  Sets alternate the arms.
window: the lanes' register windows against the all-LDS baseline (FCX_OPT_SUM_BASELINE), the same
arrays, on a physical field (HSEN after a step: both signs) and on the full-exponent-range
pattern, where no window helps.
Every arm's result is compared byte for byte with the other's.
  python integrals_ab.py [SETS] [CELLS]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "components.flux_calculator_amd", "python"))
import numpy as np
import torch
from fcx.basic import PHASE_ALL
from fcx.engine import Engine
from fcx.local_field import LocalFields
from fcx.synthetic import as_dtype, build_case

SETS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
SIZES = [int(sys.argv[2])] if len(sys.argv) > 2 else [32_768, 10_000_000]


def device_case(n, dtype):
    case = build_case("CCLM", n=n, T=1)
    if dtype == "float32":
        case = as_dtype(case, "float32")
    lf = LocalFields(case.lf.grid_size, device="cuda:0", dtype=dtype)
    moved = {}
    for key, a in case.lf.field.items():
        if id(a) not in moved:
            moved[id(a)] = torch.from_numpy(np.nan_to_num(a)).to("cuda:0")
        lf.field[key] = moved[id(a)]
    lf.allocated, lf.put_to = set(case.lf.allocated), dict(case.lf.put_to)
    case.lf = lf
    return case


def distinct_slots(case, k):
    """k distinct arrays: the step's outputs first, then inputs that hold varying non-zero values"""
    seen, out = set(), []
    keys = sorted(set(case.outputs)) + [key for key in case.lf.field if key[2] not in ("FICE", "FARE")]
    for key in keys:
        a = case.lf.field[key]
        if id(a) not in seen:
            seen.add(id(a))
            out.append(key)
    assert len(out) >= k, (len(out), k)
    return out[:k]


def time_arms(arms, reps):
    """{name: [ms per call of every set]}, the arms' order alternating from set to set"""
    ms = {name: [] for name, _ in arms}
    for k in range(SETS):
        for name, fn in (arms if k % 2 == 0 else arms[::-1]):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            ms[name].append((time.perf_counter() - t0) / reps * 1e3)
    return ms


def summary(ms, nbytes):
    med = float(np.median(ms))
    return {"ms_sets": ms, "ms_median": med, "ms_range": [min(ms), max(ms)], "tb_s": nbytes / (med * 1e-3) / 1e12}


def calls(n, dtype, nf):
    case = device_case(n, dtype)
    eng = Engine(case.lf, 1, case.methods)
    reps = 200 if n <= 1_000_000 else 20
    try:
        eng.step(PHASE_ALL, 3600)
        slots = distinct_slots(case, nf)
        es = case.lf.field[slots[0]].element_size()
        for g in (1, 2, 3):
            eng.set_areas(g, np.random.default_rng(g).uniform(0.5, 2.0, n))
        arms = [("weighted", lambda: eng.field_integrals(slots, weighted=True)),
                ("unweighted", lambda: eng.field_integrals(slots, weighted=False)),
                ("ranges", lambda: eng.field_ranges(slots))]
        ms = time_arms(arms, reps)
        nbytes = {"weighted": nf * n * (es + 8), "unweighted": nf * n * es, "ranges": nf * n * es}
        res = {"cells": n, "dtype": dtype, "fields": nf}
        for name, v in ms.items():
            res[name] = dict(summary(v, nbytes[name]), bytes=nbytes[name])
        return res
    finally:
        eng.close()


def window(n, what):
    case = device_case(n, "float64")
    rng = np.random.default_rng(3)
    eng = Engine(case.lf, 1, case.methods)
    reps = 200 if n <= 1_000_000 else 20
    try:
        eng.step(PHASE_ALL, 3600)
        if what == "exponents":  # every exponent of the double range: the window cannot help
            x = np.ldexp(rng.uniform(-1.0, 1.0, n), rng.integers(-1074, 1024, n))
            case.lf.field[(1, 1, "HSEN")].copy_(torch.from_numpy(x))
            torch.cuda.synchronize()
        eng.set_areas(1, rng.uniform(0.5, 2.0, n))
        slot = [(1, 1, "HSEN")]
        got = {}

        def arm(baseline, weighted):
            def fn():
                eng.set_option("sum_baseline", baseline)
                got[(baseline, weighted)] = eng.field_integrals(slot, weighted=weighted)[0]
            return fn

        res = {"cells": n, "field": what}
        for weighted in (False, True):
            ms = time_arms([("window", arm(0, weighted)), ("baseline", arm(1, weighted))], reps)
            assert bytes(got[(0, weighted)]) == bytes(got[(1, weighted)])
            nbytes = n * (16 if weighted else 8)
            key = "weighted" if weighted else "unweighted"
            res[key] = {name: summary(v, nbytes) for name, v in ms.items()}
            res[key]["window_over_baseline"] = res[key]["window"]["ms_median"] / res[key]["baseline"]["ms_median"]
        return res
    finally:
        eng.close()


def main():
    out = {"sets": SETS, "calls": [], "window": []}
    for n in SIZES:
        for dtype, nf in (("float64", 1), ("float64", 7), ("float64", 16), ("float32", 7)):
            out["calls"].append(calls(n, dtype, nf))
        for what in ("physical", "exponents"):
            out["window"].append(window(n, what))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
