"""The non-finite guard and the range lines through the Fortran drop-in module (fcx_check_finite,
fcx_field_range_of, components.flux_calculator_amd/fortran/flux_calculator_calculate.F90).

A Fortran host (tests/fortran/ranges_host.F90) whose local_field is the reference's own
flux_calculator_basic registers its abort routine, turns the guard on (3) and runs the two fused
phases on one manifest.  Clean inputs: it prints fcx_field_range_of of every sent field, which
must equal numpy on the output files.  One NaN in an input: the registered abort routine receives
the message naming the field and the cell, and the program ends through it.
Skipped like tests/test_fortran.py when the host program is not built (no flang, or no
reference module to hold local_field)."""
import os
import subprocess

import numpy as np
import pytest

from ranges import expect, same_value
from test_fortran import write_manifest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "oracle", "_ref", "fcx_ranges_host")
SHIM_O = os.path.join(ROOT, "components.flux_calculator_amd", "lib", "fortran", "flux_calculator_calculate.o")
STEP_T = 3600 * 24 * 45


@pytest.mark.skipif(not os.path.exists(SHIM_O), reason="Fortran shim not built (needs flang + reference module)")
def test_dropin_module_exports_the_guard_routines():
    out = subprocess.run(["nm", SHIM_O], capture_output=True, text=True, check=True).stdout.lower()
    for name in ("fcx_check_finite", "fcx_field_range_of"):
        assert f"_qmflux_calculator_calculatep{name}" in out, name
    for c in ("fcx_field_ranges", "fcx_set_option"):
        assert f" u {c}" in out, c


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(HOST), reason="Fortran ranges host not built")
@pytest.mark.parametrize("variant,T", [("CCLM", 1), ("MOM5", 2)])
def test_fortran_host_prints_the_ranges_of_its_sent_fields(tmp_path, variant, T):
    from fcx.basic import IDX
    from fcx.synthetic import build_case

    case = build_case(variant, n=8200, T=T, bias=True)
    d = str(tmp_path)
    outs = write_manifest(case, d, STEP_T)
    r = subprocess.run([HOST, d], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "RANGES_HOST OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("RANGE ")]
    assert len(lines) == len(outs)
    for i, ((s, g, name), ln) in enumerate(zip(outs, lines)):
        assert [int(x) for x in ln[1:4]] == [s, g, IDX[name]]
        want = expect(np.fromfile(os.path.join(d, f"o{i}.bin")), case.grid_size[g - 1])
        assert same_value(float(ln[4]), want.min) and same_value(float(ln[5]), want.max), (name, ln, want)
        assert int(ln[6]) == want.n_nan + want.n_inf == 0


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(HOST), reason="Fortran ranges host not built")
def test_fortran_host_ends_through_its_abort_routine_on_a_nan(tmp_path):
    from fcx.synthetic import build_case

    case = build_case("CCLM", n=8200, T=1, bias=True)
    case.lf.field[(1, 1, "TATM")][4097] = np.nan
    write_manifest(case, str(tmp_path), STEP_T)
    r = subprocess.run([HOST, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 3 and "RANGES_HOST OK" not in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    got = [ln for ln in r.stdout.splitlines() if ln.startswith("HOST ABORT ROUTINE: ")]
    assert len(got) == 1
    assert "fcx_step: phase 2: TATM(0,t) cell 4097 = nan (1 NaN, 0 Inf of 8200 cells)" in got[0], got[0]
