"""FCX_OPT_ATM_RECORDS 0 against 1 in one process: the bench workload (CCLM + MOM5 + RCO in one
group launch over n cells) built afresh for every set and arm, the arms interleaved, 60 warm-up
and 100 event-timed launches each; prints every set's median and the arms' spread.
  python records_ab.py [cells = 10000000] [sets = 4] [random | periodic]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python"))
import numpy as np
import torch

from fcx.workload import Workload

n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
sets = int(sys.argv[2]) if len(sys.argv) > 2 else 4
amap = sys.argv[3] if len(sys.argv) > 3 else "random"
res = {0: [], 1: []}
for s in range(sets):
    for opt in ((0, 1) if s % 2 == 0 else (1, 0)):
        wl = Workload(n, 0, 1, atmos_map=amap, engine_options={"atm_records": opt})
        on = [e.atm_records() for e in wl.engines]
        for k in range(60):
            wl.run_group(3600 * k)
        torch.cuda.synchronize()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(100)]
        for k, ev in enumerate(evs):
            wl.run_group(3600 * k, event=ev)
        torch.cuda.synchronize()
        ms = np.array([a.elapsed_time(b) for a, b in evs])
        res[opt].append(float(np.median(ms)))
        print(f"set {s} atm_records {opt} (on={on}): median {np.median(ms):.4f} ms, mean {ms.mean():.4f}, "
              f"p10 {np.percentile(ms, 10):.4f}, p90 {np.percentile(ms, 90):.4f}", flush=True)
        wl.close()
        del wl
        torch.cuda.empty_cache()
for opt in (0, 1):
    r = res[opt]
    print(f"atm_records {opt}: median of sets {np.median(r):.4f} ms, sets {min(r):.4f}..{max(r):.4f}")
print(json.dumps({"n": n, "map": amap, "ms": res, "gain_pct": 100 * (1 - np.median(res[1]) / np.median(res[0]))}))
