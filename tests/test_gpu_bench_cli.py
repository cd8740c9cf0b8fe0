"""bench.py's command line: a plain run (the headline figure only) and --dump-outputs.

One small run of the benchmark itself (300,007 cells: more than one block per variant, no
multiple of the 128-cell wave tile, above the dump's sample size so the flux arrays are
sampled and the atmosphere arrays are not), then the same workload stepped in this process:
the dumped arrays must be bit-identical to what the timed path's caller holds after the
last step (same seeded inputs, same launch)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from fcx.workload import ATM_FIELDS, VARIANTS, Workload  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS, STEPS = 300_007, 3
FULL_ONLY = ("cold_step_ms", "kernels", "multi_gpu_check", "other_map", "config5_fp32", "config4", "e2e",
             "cpu_baseline", "baltic_size")


def test_plain_run_and_dump_outputs(tmp_path):
    import bench

    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "2",
           "--cells", str(CELLS), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["metric"] == bench.METRIC and line["unit"] == "Mcells/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["steps"] == STEPS
    assert line["ms_per_step"] > 0
    # the line rounds ms_per_step to 1e-4, timed_ms to 1e-3 and value to 0.1
    assert abs(line["ms_per_step"] * STEPS - line["timed_ms"]) <= 0.5e-4 * STEPS + 0.5e-3 + 1e-9
    assert abs(line["value"] - CELLS * len(VARIANTS) / line["ms_per_step"] / 1e3) \
        <= 1.01 * line["value"] * 0.5e-4 / (line["ms_per_step"] - 0.5e-4) + 0.05 + 1e-9
    assert not [k for k in FULL_ONLY if k in line], sorted(line)

    files = sorted(os.listdir(out))
    assert sum(os.path.getsize(out / f) for f in files) <= 64e6
    wl = Workload(CELLS, variants=VARIANTS, atmos_map="random")
    try:
        wl.run_group((STEPS - 1) * 3600)  # the last timed step (no bias: the time selects nothing)
        wl.download()
        want = {}
        for v, case, outs in zip(wl.variants, wl.cases, wl.atm_outs):
            for s, g, name in dict.fromkeys(case.outputs):
                want[f"{v}.flux.s{s}.g{g}.{name}.npy"] = np.asarray(case.lf.field[(s, g, name)])
            for name, _ in ATM_FIELDS:
                want[f"{v}.atmos.{name}.npy"] = np.asarray(outs[name][: wl.la.n_atmos])
        assert files == sorted(want)
        per = min(bench.DUMP_SAMPLE, int(bench.DUMP_BYTES // (8 * len(want))))
        assert wl.la.n_atmos <= per < CELLS  # both branches of the sampling are exercised
        for f, w in want.items():
            got = np.load(out / f)
            assert got.dtype == np.float64 and np.isfinite(got).all(), f
            n = w.shape[0]
            if n > per:
                w = w[np.unique(np.random.default_rng([bench.DUMP_SEED, n]).integers(0, n, per))]
            np.testing.assert_array_equal(got, w, err_msg=f)
            assert np.any(got != 0), f
    finally:
        wl.close()
