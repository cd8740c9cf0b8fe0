"""Field ranges and the non-finite guard, measured in one process (measurement tool,
fcx_field_ranges / FCX_OPT_CHECK_FINITE).

launch: fcx_field_ranges of 1, 7 and 16 fp64 fields and 7 fp32 fields of a device-resident CCLM
engine -- the range launch, the finishing launch, the 40 B per field copy and the wait -- as
wall-clock per call, with its bytes read per second; beside it a read-only stream of the same
bytes in the same process timed the same way (torch.amax of each array, one launch per array,
then one wait).  Sets alternate the two.
guard: what FCX_OPT_CHECK_FINITE costs a step: the CCLM + MOM5 + RCO group step device-resident
(fcx.workload, fcx_run_group) and the Baltic-size host step (MOM5, two surface types, fcx_step
from heap arrays), with the check off, with bit 0 and with bits 0 + 1.  A fresh engine set per
arm and set, the arms' order rotating from set to set; median wall-clock ms per step of every
set and the sets' range.
  python ranges_ab.py [SETS] [CELLS] [GROUP_CELLS]"""
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
from fcx.workload import Workload

SETS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
SIZES = [int(sys.argv[2])] if len(sys.argv) > 2 else [32_768, 10_000_000]
GROUP_N = int(sys.argv[3]) if len(sys.argv) > 3 else 10_000_000
BALTIC_N = 32_768
T_STEP = 3600 * 24 * 45


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


def distinct_slots(lf, k):
    seen, out = set(), []
    for key, a in lf.field.items():
        if id(a) not in seen:
            seen.add(id(a))
            out.append(key)
    assert len(out) >= k, (len(out), k)
    return out[:k]


def launch_alone(n, dtype, nf):
    case = device_case(n, dtype)
    eng = Engine(case.lf, 1, case.methods)
    reps = 200 if n <= 1_000_000 else 20
    try:
        slots = distinct_slots(case.lf, nf)
        arrays = [case.lf.field[k] for k in slots]
        nbytes = nf * n * arrays[0].element_size()

        def ranges():
            eng.field_ranges(slots)

        def stream():
            for a in arrays:
                torch.amax(a)
            torch.cuda.synchronize()

        ms = {"ranges": [], "stream": []}
        for k in range(SETS):
            for name, fn in ((("ranges", ranges), ("stream", stream)) if k % 2 == 0 else
                             (("stream", stream), ("ranges", ranges))):
                for _ in range(5):
                    fn()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                ms[name].append((time.perf_counter() - t0) / reps * 1e3)
        res = {"cells": n, "dtype": dtype, "fields": nf, "bytes": nbytes}
        for name, v in ms.items():
            med = float(np.median(v))
            res[name] = {"ms_sets": v, "ms_median": med, "ms_range": [min(v), max(v)],
                         "tb_s": nbytes / (med * 1e-3) / 1e12}
        return res
    finally:
        eng.close()


def timed(step, steps, warm):
    for k in range(warm):
        step(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        step(warm + k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def group_step(check):
    wl = Workload(GROUP_N, 0, 1, ("CCLM", "MOM5", "RCO"), atmos=True, engine_options={"check_finite": check})
    try:
        steps, warm = (20, 5) if GROUP_N > 1_000_000 else (200, 20)
        ms = timed(lambda k: wl.run_group(3600 * k), steps, warm)
        return ms, [e.last_group_size() for e in wl.engines], len(wl.engines[0].check_fields(PHASE_ALL))
    finally:
        wl.close()


def baltic_step(check):
    case = build_case("MOM5", n=BALTIC_N, T=2, bias=True)
    eng = Engine(case.lf, 2, case.methods, corrections=case.corrections, averages=case.averages,
                 options={"check_finite": check})
    try:
        ms = timed(lambda k: eng.step(PHASE_ALL, T_STEP), 200, 20)
        return ms, eng.zero_copy_active(), len(eng.check_fields(PHASE_ALL))
    finally:
        eng.close()


def guard(fn):
    ms, info = {0: [], 1: [], 3: []}, {}
    for k in range(SETS):
        arms = [0, 1, 3]
        arms = arms[k % 3:] + arms[: k % 3]
        for check in arms:
            t, *rest = fn(check)
            ms[check].append(t)
            info[check] = rest
    return {f"check_{c}": {"step_ms_sets": v, "step_ms_median": float(np.median(v)), "step_ms_range": [min(v), max(v)],
                           "info": info[c]} for c, v in ms.items()}


def main():
    out = {"sets": SETS, "launch": []}
    for n in SIZES:
        for dtype, nf in (("float64", 1), ("float64", 7), ("float64", 16), ("float32", 7)):
            out["launch"].append(launch_alone(n, dtype, nf))
    out["guard_group_cells"] = GROUP_N
    out["guard_group"] = guard(group_step)
    out["guard_baltic_cells"] = BALTIC_N
    out["guard_baltic"] = guard(baltic_step)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
