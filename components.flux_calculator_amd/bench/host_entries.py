"""The 32,768-cell host-array entries of `bench.py --full` alone, through bench.py's own
functions (bench.py has no switch that selects them): caller heap arrays one variant after
another (e2e_host), fcx_step_async (e2e_async), library memory by zero-copy and by spans
(e2e_library_memory).  One JSON line of us_per_step_median figures; FCX_LIBRARY selects the
build, so two commits can be run in alternating processes (profiles/r12/pairs/)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

args = argparse.Namespace(types=1, bias=False)
variants = list(bench.VARIANTS)
heap = bench.e2e_host(args, variants, sizes=(32_768,))["sizes"]["32768"]
out = {"heap_" + v: x["us_per_step_median"] for v, x in heap["variants"].items()}
out["step_async"] = bench.e2e_async(args, variants)["us_per_step_median"]
lib = bench.e2e_library_memory(args, variants)
for tr in ("zero_copy", "spans"):
    for mode in ("sequential", "async"):
        out[f"lib_{tr}_{mode}"] = lib[tr][f"{mode}_us_per_step_median"]
print(json.dumps(out))
