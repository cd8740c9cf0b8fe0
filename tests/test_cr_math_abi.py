"""FCX_OPT_CR_MATH through the C ABI: the option's values and state rules, the default from the
environment variable FCX_CR_MATH, one number in the header, the Python and the Fortran
bindings, the query before and after fcx_commit, and the plans of an fp64 engine with the
option on (every launch family has its sibling, so fcx_plan_check passes as without it).
The tests that commit an engine are marked gpu; the others run without one."""
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
OPT = 24


def new_engine(lib, precision):
    h = ctypes.c_void_p()
    gs = (ctypes.c_int32 * 3)(64, 64, 64)
    assert lib.fcx_create(0, 1, gs, ctypes.byref(h)) == 0
    assert lib.fcx_set_precision(h, precision) == 0
    return h


def is_on(lib, h):
    on = ctypes.c_int32(-1)
    assert lib.fcx_cr_math(h, ctypes.byref(on)) == 0
    return on.value


@pytest.mark.parametrize("precision", [_lib.FCX_PRECISION_F64, _lib.FCX_PRECISION_F32])
def test_option_values(precision):
    """0 and 1 on an uncommitted engine of either precision; 2 and -1 are FCX_E_ARG.  The query
    answers 0 before fcx_commit whatever the option says."""
    lib = _lib.load()
    h = new_engine(lib, precision)
    try:
        assert is_on(lib, h) == 0
        assert lib.fcx_set_option(h, OPT, 1) == 0
        assert is_on(lib, h) == 0  # not committed
        assert lib.fcx_set_option(h, OPT, 0) == 0
        for bad in (2, -1):
            assert lib.fcx_set_option(h, OPT, bad) == E_ARG
            assert b"cr_math" in lib.fcx_last_error()
        assert is_on(lib, h) == 0
        assert lib.fcx_cr_math(h, None) == E_ARG
    finally:
        lib.fcx_destroy(h)


def test_one_number_everywhere():
    header = open(os.path.join(ROOT, "include", "fcx.h")).read()
    m = re.search(r"FCX_OPT_CR_MATH\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == OPT
    assert "int fcx_cr_math(const fcx_engine *e, int32_t *on);" in header
    assert _lib.FCX_OPT_CR_MATH == OPT
    assert Engine.OPTIONS["cr_math"] == OPT
    assert sorted(Engine.OPTIONS.values()).count(OPT) == 1
    f90 = open(os.path.join(PKG, "fortran", "fcx_c_api.F90")).read()
    m = re.search(r"FCX_OPT_CR_MATH\s*=\s*(\d+)", f90)
    assert m and int(m.group(1)) == OPT
    assert "BIND(C, name='fcx_cr_math')" in f90


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("variant", ["CCLM", "MOM5", "RCO"])
def test_plan_check_with_the_option_on(variant, T):
    """no plan is refused for the option (an uncommitted engine: fcx_plan_check needs no GPU)"""
    c = build_case(variant, n=257, T=T, bias=True)
    eng = Engine(c.lf, c.num_surface_types, c.methods, corrections=c.corrections, averages=c.averages,
                 options={"cr_math": 1}, commit=False)
    try:
        assert not eng.cr_math()  # before commit
        eng.plan_check()
    finally:
        eng.close()


CHILD = """
import sys
import numpy as np
from fcx.engine import Engine
from fcx.synthetic import as_dtype, build_case
explicit, precision = sys.argv[1], sys.argv[2]
c = build_case("CCLM", n=64, T=1)
if precision == "f32":
    c = as_dtype(c, "float32")
options = {} if explicit == "none" else {"cr_math": int(explicit)}
eng = Engine(c.lf, 1, c.methods, options=options, commit=False)
before = int(eng.cr_math())
eng.commit()
print(before, int(eng.cr_math()))
eng.close()
"""


def child(env, explicit, precision):
    environ = {k: v for k, v in os.environ.items() if k != "FCX_CR_MATH"}
    if env is not None:
        environ["FCX_CR_MATH"] = env
    environ["PYTHONPATH"] = os.pathsep.join([os.path.join(PKG, "python")] + sys.path)
    out = subprocess.run([sys.executable, "-c", CHILD, str(explicit), precision], env=environ, capture_output=True,
                         text=True)
    assert out.returncode == 0, out.stderr
    return tuple(int(x) for x in out.stdout.split())


@pytest.mark.gpu
@pytest.mark.parametrize("env,explicit,want", [("1", "none", 1), ("1", 0, 0), ("1", 1, 1), ("0", 1, 1), (None, "none", 0),
                                               (None, 1, 1), ("2", "none", 0)])
def test_environment_sets_the_default(env, explicit, want):
    """FCX_CR_MATH in the environment of a fresh process is the default of the engines created in
    it (0 or 1; anything else is ignored); an explicit option wins.  The query is 0 before
    fcx_commit and tells what the committed fp64 engine runs."""
    assert child(env, explicit, "f64") == (0, want)


@pytest.mark.gpu
@pytest.mark.parametrize("env,explicit", [("1", "none"), (None, 1)])
def test_fp32_engines_accept_and_ignore_it(env, explicit):
    assert child(env, explicit, "f32") == (0, 0)


@pytest.mark.gpu
def test_applied_at_commit():
    """after fcx_commit the option is FCX_E_STATE; with FCX_OPT_F32_MATH on an fp32 engine it is
    accepted and the engine still reports the wide kernels, not these"""
    c = build_case("RCO", n=64, T=1)
    eng = Engine(c.lf, 1, c.methods, options={"cr_math": 1})
    try:
        assert eng.cr_math() and not eng.f32_math()
        assert eng.lib.fcx_set_option(eng.h, OPT, 0) == E_STATE
        assert eng.cr_math()
    finally:
        eng.close()
    c32 = as_dtype(build_case("RCO", n=64, T=1), "float32")
    eng = Engine(c32.lf, 1, c32.methods, options={"cr_math": 1, "f32_math": 1})
    try:
        assert eng.f32_math() and not eng.cr_math()
    finally:
        eng.close()
