"""Builds of libfcx against each other in one process (measurement tool): the bench workload
(CCLM + MOM5 + RCO in one group launch over 10M cells, host arrays with engine-owned
tile-blocked mirrors, random map) built afresh for every set and arm and freed again before the
next, the arms' order rotating from set to set; 60 warm-up and 100 event-timed launches each.
Like records_ab.py, with a library per arm.  (inproc_ab.py --host keeps every build's mirrors
allocated side by side, in the same order in every process: the builds then differ by their
placement the same way every time.)
  python lib_ab.py SETS NAME=PATH ...   (PATH 'ref': the product build)"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python"))
import numpy as np
import torch
from fcx import _lib
from fcx.basic import PHASE_ALL, PHASE_NORMAL
from fcx.engine import Engine, run_group
from fcx.parallel import BlockedRandomAtmosMap
from fcx.synthetic import build_case, inputs_for_bench

VARIANTS = ("CCLM", "MOM5", "RCO")
FIELDS = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))
sets = int(sys.argv[1])
arms = {}
for spec in sys.argv[2:]:
    name, path = spec.split("=", 1)
    arms[name] = None if path == "ref" else _lib.load_path(path)
n = 10_000_000
host = inputs_for_bench(n)
la = BlockedRandomAtmosMap().local(0, n, 0, 1, n)
stream = torch.cuda.current_stream()
names = list(arms)
res = {k: [] for k in names}
for s in range(sets):
    order = names[s % len(names):] + names[: s % len(names)]
    for arm in order:
        engines, keep = [], []
        for v in VARIANTS:
            c = build_case(v, n=n, T=1, data=host)
            o = {name: np.empty(la.n_atmos) for name, _ in FIELDS}
            engines.append(Engine(c.lf, 1, c.methods, corrections=c.corrections, averages=c.averages, device=0,
                                  stream=stream.cuda_stream,
                                  atmos={"local": la, "fields": [(PHASE_NORMAL, 1, g, name, o[name]) for name, g in FIELDS]},
                                  options={"atmos_in_run": 0, "timing": 0, "host_staging": 0}, lib=arms[arm]))
            keep.append((c, o))
        for e in engines:
            e.upload(PHASE_ALL)
        for k in range(60):
            run_group(engines, PHASE_ALL, 3600 * k)
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(100)]
        for k, (a, b) in enumerate(evs):
            a.record(stream)
            run_group(engines, PHASE_ALL, 3600 * k)
            b.record(stream)
        torch.cuda.synchronize()
        ms = np.array([a.elapsed_time(b) for a, b in evs])
        res[arm].append(round(float(np.median(ms)), 4))
        print(f"set {s} {arm}: median {np.median(ms):.4f} ms, mean {ms.mean():.4f}, p10 {np.percentile(ms, 10):.4f}, "
              f"p90 {np.percentile(ms, 90):.4f}, group {[e.last_group_size() for e in engines]}", flush=True)
        for e in engines:
            e.close()
        del engines, keep
        torch.cuda.empty_cache()
for arm in names:
    r = res[arm]
    print(f"{arm}: median of sets {np.median(r):.4f} ms, sets {min(r):.4f}..{max(r):.4f}")
print(json.dumps({"n": n, "map": "random", "launches_per_set": 100, "ms": res}))
