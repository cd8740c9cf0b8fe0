"""No sub-dword vector load in any cells_* kernel of the built library.  The wave-uniform
method bytes of the parameter block (TypeParams::m_*, bias_adds, Params::rec_pos) are read
as aligned words through the scalar unit (fcx_kernels.hip type_methods); a byte member read
directly is a global_load_ubyte / sbyte, a wait for the wave's loads and stores in flight
and a v_readfirstlane in the middle of the flux pass (gfx950 has no byte-sized scalar load).
The disassembly of lib/libfcx.so is read with tools/isa_waits.py; no GPU is needed."""
import importlib.util
import os

import pytest

from fcx import _lib

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "components.flux_calculator_amd",
                    "tools", "isa_waits.py")


def test_cells_kernels_have_no_subdword_vector_loads():
    spec = importlib.util.spec_from_file_location("isa_waits", TOOL)
    isa = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa)
    if not isa.have_disassembler():
        pytest.skip("no llvm-objdump")
    rows = isa.report(isa.disassemble(_lib.LIB_PATH), "cells_")
    assert len(rows) > 50, f"only {len(rows)} cells_* kernels found in {_lib.LIB_PATH}"
    assert any(name.startswith("fcx::cells_atmos_group_kernel") for name in rows)
    bad = {name: r["subdword_loads"] for name, r in rows.items() if r["subdword_loads"]}
    assert not bad, f"sub-dword vector loads (global_load_[us]byte/short): {bad}"
