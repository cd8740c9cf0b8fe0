"""fcx_fused_accumulation, the query beside fcx_atm_records / fcx_f32_math: whether a phase's
exchange -> atmosphere accumulation rides inside the flux launch.  Its argument checks need no
GPU: the answer itself is only known after fcx_commit (tests/test_gpu_f32_multitype.py)."""
import ctypes

import pytest

from fcx import _lib

E_ARG, E_STATE = 1, 2


@pytest.fixture()
def uncommitted():
    lib = _lib.load()
    h = ctypes.c_void_p()
    gs = (ctypes.c_int32 * 3)(10, 10, 10)
    _lib.check(lib.fcx_create(0, 2, gs, ctypes.byref(h)))
    yield lib, h
    lib.fcx_destroy(h)


def test_uncommitted_engine_is_a_state_error(uncommitted):
    lib, h = uncommitted
    on = ctypes.c_int32(7)
    for phase in (1, 2, 3):
        assert lib.fcx_fused_accumulation(h, phase, ctypes.byref(on)) == E_STATE
    assert b"fcx_commit" in lib.fcx_last_error()
    assert on.value == 7  # nothing is answered


def test_null_pointer_is_an_argument_error(uncommitted):
    lib, h = uncommitted
    assert lib.fcx_fused_accumulation(h, 3, None) == E_ARG
    on = ctypes.c_int32()
    assert lib.fcx_fused_accumulation(None, 3, ctypes.byref(on)) == E_ARG


@pytest.mark.parametrize("phase", [0, 4])
def test_phase_outside_1_to_3_is_an_argument_error(uncommitted, phase):
    lib, h = uncommitted
    on = ctypes.c_int32()
    assert lib.fcx_fused_accumulation(h, phase, ctypes.byref(on)) == E_ARG
    assert b"phase" in lib.fcx_last_error()
