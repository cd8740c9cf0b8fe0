"""Rank-invariant atmosphere sums through the Fortran drop-in module (fcx_define_atmos_terms,
fcx_engine_handle, the fcx_c_api interfaces fcx_set_atmos_terms / fcx_atmos_columns /
fcx_atmos_invariant; components.flux_calculator_amd/fortran/).

A Fortran host (tests/fortran/invariant_host.F90) whose local_field is the reference's own
flux_calculator_basic runs, in ONE process, a global case and its two shards, cut inside an
atmosphere cell.  It works out max_terms and left_pos with the table loop of INTEGRATION.md
section 3, keeps the boundary slots in library host memory, adds the two shards' slots itself
(the all-reduce) and lets fcx_atmos_finish add the terms in link order.  Every atmosphere cell of
both shards must have the bits of the global run, the shared cell included; the numbers the host
reports are those of fcx.parallel.boundary_terms.
Skipped like tests/test_fortran.py when the host program is not built (no flang, or no reference
module to hold local_field)."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_fortran import write_manifest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "oracle", "_ref", "fcx_invariant_host")
SHIM_O = os.path.join(ROOT, "components.flux_calculator_amd", "lib", "fortran", "flux_calculator_calculate.o")
FIELDS = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))


@pytest.mark.skipif(not os.path.exists(SHIM_O), reason="Fortran shim not built (needs flang + reference module)")
def test_dropin_module_exports_the_terms_routines():
    out = subprocess.run(["nm", SHIM_O], capture_output=True, text=True, check=True).stdout.lower()
    for name in ("fcx_define_atmos_terms", "fcx_engine_handle"):
        assert f"_qmflux_calculator_calculatep{name}" in out, name
    assert " u fcx_set_atmos_terms" in out


def shard(full, lo, hi, variant, T, seed):
    from fcx.synthetic import build_case

    case = build_case(variant, n=hi - lo, T=T, bias=True, seed=seed)
    moved = {}
    for key, a in full.lf.field.items():
        if id(a) not in moved:
            moved[id(a)] = np.array(np.asarray(a)[lo:hi], copy=True)
        case.lf.field[key] = moved[id(a)]
    init_date, corr = full.corrections
    case.corrections = (init_date, np.ascontiguousarray(corr[lo:hi]))
    return case


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(HOST), reason="Fortran invariant host not built")
@pytest.mark.parametrize("variant,T", [("CCLM", 1), ("MOM5", 2)])
def test_fortran_host_two_shards_bit_identical_to_the_global_run(tmp_path, variant, T):
    from fcx.basic import IDX
    from fcx.parallel import boundary_terms, local_atmos, synthetic_atmos_map
    from fcx.synthetic import build_case

    n, seed = 4099, 77
    amap = synthetic_atmos_map(n)
    idx = amap.atmos_index
    # a cut with two exchange cells of the atmosphere cell on either side
    cut = next(i for i in range(n // 2, n - 2) if idx[i - 2] == idx[i - 1] == idx[i] == idx[i + 1])
    ranges = [(0, cut), (cut, n - cut)]
    full = build_case(variant, n=n, T=T, bias=True, seed=seed)
    s0 = 1 if T == 1 else 0  # the type-0 fields: the averages with several surface types
    dirs, las = [], []
    for r in (0, 1, None):
        d = str(tmp_path / ("global" if r is None else f"shard{r}"))
        os.makedirs(d)
        if r is None:
            case, la = full, local_atmos(amap, 0, 1)
        else:
            off, size = ranges[r]
            case, la = shard(full, off, off + size, variant, T, seed), local_atmos(amap, r, 2, ranges=ranges)
        write_manifest(case, d, 3600 * 24 * 45)
        np.concatenate([la.atmos_index.astype(np.float64), la.weight]).tofile(os.path.join(d, "map.bin"))
        lines = [f"T {la.n_atmos} {la.atmos_offset} map.bin"]
        lines += [f"F {s0} {g} {IDX[name]} f{i}.bin" for i, (name, g) in enumerate(FIELDS)]
        with open(os.path.join(d, "manifest.txt"), "a") as f:
            f.write("\n".join(lines) + "\n")
        dirs.append(d)
        las.append(la)
    k, pos = boundary_terms(ranges, lambda x: idx[x])
    assert las[0].right == las[1].left == 0 and pos[1] >= 2 and k >= 4
    r = subprocess.run([HOST, dirs[2], dirs[0], dirs[1]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"INVARIANT_HOST OK max_terms (\d+) left_pos (\d+) columns (\d+)", r.stdout)
    assert m, r.stdout
    # the Fortran table loop against fcx.parallel.boundary_terms; fcx_atmos_columns
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (k, pos[1], len(FIELDS) * (1 + k))
    for i, (name, _) in enumerate(FIELDS):
        want = np.fromfile(os.path.join(dirs[2], f"f{i}.bin"), dtype=np.float64)
        assert want.shape[0] == amap.n_atmos and np.isfinite(want).all() and np.any(want != 0.0), name
        for la, d in zip(las[:2], dirs[:2]):
            got = np.fromfile(os.path.join(d, f"f{i}.bin"), dtype=np.float64)
            w = want[la.atmos_offset: la.atmos_offset + la.n_atmos]
            assert got.shape == w.shape
            assert np.array_equal(got.view(np.uint64), w.view(np.uint64)), (name, la.offset)
