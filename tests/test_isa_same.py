"""tools/isa_waits.py same(): two disassemblies, {kernel: [instructions]}, compared instruction
for instruction -- what `isa_waits.py --same LIB_A LIB_B` reports of two builds of the library.
Hand-made dictionaries; neither a library nor a GPU is needed."""
import importlib.util
import os

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "components.flux_calculator_amd",
                    "tools", "isa_waits.py")
spec = importlib.util.spec_from_file_location("isa_waits", TOOL)
isa = importlib.util.module_from_spec(spec)
spec.loader.exec_module(isa)

A = {"cells_a": ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "s_waitcnt lgkmcnt(0)", "s_endpgm"],
     "cells_b": ["v_add_f64 v[0:1], v[2:3], v[4:5]", "s_endpgm"]}


def copy(funcs):
    return {k: list(v) for k, v in funcs.items()}


def test_equal():
    assert isa.same(A, copy(A)) == ([], [], {})
    assert isa.same({}, {}) == ([], [], {})


def test_one_instruction_changed():
    b = copy(A)
    b["cells_a"][1] = "s_waitcnt vmcnt(0) lgkmcnt(0)"
    only_a, only_b, differ = isa.same(A, b)
    assert (only_a, only_b) == ([], [])
    assert differ == {"cells_a": (1, "s_waitcnt lgkmcnt(0)", "s_waitcnt vmcnt(0) lgkmcnt(0)")}


def test_one_list_is_a_prefix_of_the_other():
    b = copy(A)
    b["cells_b"].append("s_nop 0")
    assert isa.same(A, b) == ([], [], {"cells_b": (2, None, "s_nop 0")})
    assert isa.same(b, A) == ([], [], {"cells_b": (2, "s_nop 0", None)})


def test_kernel_missing_on_each_side():
    b = copy(A)
    del b["cells_b"]
    b["cells_c"] = ["s_endpgm"]
    assert isa.same(A, b) == (["cells_b"], ["cells_c"], {})
    assert isa.same(b, A) == (["cells_c"], ["cells_b"], {})
