"""ms per launch of each variant's own fused launch, per precision (measurement tool).

One engine per run (Workload of one variant, device-resident inputs, random map), fcx_run +
fcx_run_atmos timed with events.  Prints one line per (types, variant, precision).
  python per_variant.py [--cells N] [--types 1,2] [--variants CCLM,MOM5,RCO]
                        [--precisions f64,f32,f32w] [--warm 20] [--launches 60]
With a few launches and one variant it is also the program for a counter run of one kernel."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "components.flux_calculator_amd", "python"))
import numpy as np
import torch
from fcx.basic import PHASE_ALL
from fcx.workload import Workload

p = argparse.ArgumentParser()
p.add_argument("--cells", type=int, default=10_000_000)
p.add_argument("--types", default="1,2")
p.add_argument("--variants", default="CCLM,MOM5,RCO")
p.add_argument("--precisions", default="f64,f32,f32w")
p.add_argument("--warm", type=int, default=20)
p.add_argument("--launches", type=int, default=60)
args = p.parse_args()

for T in (int(t) for t in args.types.split(",")):
    for v in args.variants.split(","):
        for prec in args.precisions.split(","):
            wl = Workload(args.cells, 0, 1, (v,), types=T, precision=prec, bias=False, atmos_map="random")
            try:
                for k in range(args.warm):
                    wl.run(3600 * k)
                torch.cuda.synchronize()
                evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                       for _ in range(args.launches)]
                for k, (a, b) in enumerate(evs):
                    a.record(wl.stream)
                    wl.run(3600 * k)
                    b.record(wl.stream)
                torch.cuda.synchronize()
                ms = np.array([a.elapsed_time(b) for a, b in evs])
                fused = wl.engines[0].fused_accumulation(PHASE_ALL) if hasattr(wl.engines[0].lib, "fcx_fused_accumulation") else None
                print(f"T={T} {v} {prec}: median {np.median(ms):.4f} ms (min {ms.min():.4f}), fused {fused}", flush=True)
            finally:
                wl.close()
            torch.cuda.empty_cache()
