"""The receive side through the Fortran drop-in module (fcx_define_receive_map /
fcx_declare_received, components.flux_calculator_amd/fortran/flux_calculator_calculate.F90).

A Fortran host (tests/fortran/received_host.F90) whose local_field is the reference's own
flux_calculator_basic runs the two fused phases twice on one manifest: `declared` receives the
atmosphere fields, TSUR and FICE on the models' grids and declares them through the module (the
exchange-grid arrays are overwritten with NaN after the commit), `plain` uses the exchange-grid
arrays the numpy restatement expanded on the host.  The outputs are equal bit for bit.
Skipped like tests/test_fortran.py when the host program is not built (no flang, or no
reference module to hold local_field)."""
import os
import subprocess

import numpy as np
import pytest

import received
from parity import bits_equal
from test_fortran import write_manifest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "oracle", "_ref", "fcx_received_host")
SHIM_O = os.path.join(ROOT, "components.flux_calculator_amd", "lib", "fortran", "flux_calculator_calculate.o")


@pytest.mark.skipif(not os.path.exists(SHIM_O), reason="Fortran shim not built (needs flang + reference module)")
def test_dropin_module_exports_the_receive_routines():
    out = subprocess.run(["nm", SHIM_O], capture_output=True, text=True, check=True).stdout.lower()
    for name in ("fcx_define_receive_map", "fcx_declare_received"):
        assert f"_qmflux_calculator_calculatep{name}" in out, name
    for c in ("fcx_add_receive_map", "fcx_bind_received"):
        assert f" u {c}" in out, c


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(HOST), reason="Fortran receive host not built")
@pytest.mark.parametrize("variant,T", [("CCLM", 1), ("MOM5", 2)])
def test_fortran_host_declares_received_fields(tmp_path, variant, T):
    from fcx.basic import IDX
    from fcx.synthetic import build_case

    n, atm, oce = received.geometric(12)
    case = build_case(variant, n=n, T=T, bias=True)
    decl = received.standard(case, atm, oce)
    decl.fill_exchange(case)
    d = str(tmp_path)
    outs = write_manifest(case, d, 3600 * 24 * 45)
    lines, ids = [], {}
    for mkey, (grid, (n_src, src, dst, w)) in decl.maps.items():
        ids[mkey] = len(ids) + 1
        np.concatenate([src + 1.0, dst + 1.0, w]).astype(np.float64).tofile(os.path.join(d, f"p{ids[mkey]}.bin"))
        lines.append(f"P {ids[mkey]} {grid} {n_src} {len(src)} p{ids[mkey]}.bin")
    for i, ((s, g, name), (mkey, phase)) in enumerate(decl.fields.items()):
        decl.sources[(s, g, name)].astype(np.float64).tofile(os.path.join(d, f"x{i}.bin"))
        lines.append(f"X {s} {g} {IDX[name]} {ids[mkey]} {phase} x{i}.bin")
    with open(os.path.join(d, "manifest.txt"), "a") as f:
        f.write("\n".join(lines) + "\n")
    got = {}
    for mode in ("declared", "plain"):
        r = subprocess.run([HOST, d, mode], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "RECEIVED_HOST OK" in r.stdout, r.stdout
        got[mode] = {key: np.fromfile(os.path.join(d, f"o{i}.bin"), dtype=np.float64) for i, key in enumerate(outs)}
    for key in outs:
        assert np.all(np.isfinite(got["declared"][key])), key
        assert bits_equal(got["declared"][key], got["plain"][key]).all(), key
