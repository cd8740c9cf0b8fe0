"""FCX_OPT_F32_MATH on the host (no GPU): the option's values and state rules, the default from
the environment variable FCX_F32_MATH, one number in the header, the Python and the Fortran
bindings, and the plans of an fp32 engine with the option on (every launch family it can take
has a wide kernel, so fcx_plan_check passes as it does without the option)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from fcx import _lib
from fcx.engine import Engine
from fcx.synthetic import as_dtype, build_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "components.flux_calculator_amd")
E_ARG, E_STATE = 1, 2
OPT = 22


def new_engine(lib, precision):
    h = ctypes.c_void_p()
    gs = (ctypes.c_int32 * 3)(64, 64, 64)
    assert lib.fcx_create(0, 1, gs, ctypes.byref(h)) == 0
    assert lib.fcx_set_precision(h, precision) == 0
    return h


def is_on(lib, h):
    on = ctypes.c_int32(-1)
    assert lib.fcx_f32_math(h, ctypes.byref(on)) == 0
    return on.value


@pytest.mark.parametrize("precision", [_lib.FCX_PRECISION_F64, _lib.FCX_PRECISION_F32])
def test_option_values(precision):
    """0 and 1 on an uncommitted engine of either precision; 2 and -1 are FCX_E_ARG.  On an fp64
    engine the option is accepted and changes nothing."""
    lib = _lib.load()
    h = new_engine(lib, precision)
    try:
        f32 = precision == _lib.FCX_PRECISION_F32
        assert is_on(lib, h) == (1 if f32 and os.environ.get("FCX_F32_MATH") == "1" else 0)
        assert lib.fcx_set_option(h, OPT, 1) == 0
        assert is_on(lib, h) == (1 if f32 else 0)
        assert lib.fcx_set_option(h, OPT, 0) == 0
        assert is_on(lib, h) == 0
        for bad in (2, -1):
            assert lib.fcx_set_option(h, OPT, bad) == E_ARG
            assert b"f32_math" in lib.fcx_last_error()
        assert is_on(lib, h) == 0
    finally:
        lib.fcx_destroy(h)


CHILD = """
import ctypes, sys
from fcx import _lib
lib = _lib.load()
h = ctypes.c_void_p()
gs = (ctypes.c_int32 * 3)(8, 8, 8)
assert lib.fcx_create(0, 1, gs, ctypes.byref(h)) == 0
assert lib.fcx_set_precision(h, _lib.FCX_PRECISION_F32) == 0
on = ctypes.c_int32(-1)
assert lib.fcx_f32_math(h, ctypes.byref(on)) == 0
first = on.value
assert lib.fcx_set_option(h, 22, int(sys.argv[1])) == 0
assert lib.fcx_f32_math(h, ctypes.byref(on)) == 0
print(first, on.value)
"""


@pytest.mark.parametrize("env,explicit,want", [("1", 0, (1, 0)), ("1", 1, (1, 1)), ("0", 1, (0, 1)), (None, 0, (0, 0)),
                                               ("2", 0, (0, 0))])
def test_environment_sets_the_default(env, explicit, want):
    """FCX_F32_MATH in the environment of a fresh process is the default of engines created in
    it (0 or 1; anything else is ignored); an explicit option wins."""
    environ = {k: v for k, v in os.environ.items() if k != "FCX_F32_MATH"}
    if env is not None:
        environ["FCX_F32_MATH"] = env
    environ["FCX_NO_TORCH"] = "1"
    environ["PYTHONPATH"] = os.pathsep.join([os.path.join(PKG, "python")] + sys.path)
    out = subprocess.run([sys.executable, "-c", CHILD, str(explicit)], env=environ, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert tuple(int(x) for x in out.stdout.split()) == want


def test_one_number_everywhere():
    header = open(os.path.join(ROOT, "include", "fcx.h")).read()
    m = re.search(r"FCX_OPT_F32_MATH\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == OPT
    assert _lib.FCX_OPT_F32_MATH == OPT
    assert Engine.OPTIONS["f32_math"] == OPT
    f90 = open(os.path.join(PKG, "fortran", "fcx_c_api.F90")).read()
    m = re.search(r"FCX_OPT_F32_MATH\s*=\s*(\d+)", f90)
    assert m and int(m.group(1)) == OPT
    assert sorted(Engine.OPTIONS.values()).count(OPT) == 1


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("variant", ["CCLM", "MOM5", "RCO"])
def test_plan_check_with_the_option_on(variant, T):
    c32 = as_dtype(build_case(variant, n=257, T=T, bias=True), "float32")
    eng = Engine(c32.lf, c32.num_surface_types, c32.methods, corrections=c32.corrections, averages=c32.averages,
                 options={"f32_math": 1}, commit=False)
    try:
        assert eng.f32_math()
        eng.plan_check()
    finally:
        eng.close()
