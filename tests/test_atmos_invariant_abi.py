"""FCX_OPT_ATMOS_INVARIANT through the C ABI, without a GPU: the new entry points exported and
bound in Python and Fortran, one option number everywhere, option and getter round trip,
fcx_atmos_columns, and the named FCX_E_ARG errors fcx_plan_check raises on the host (the same
fcx_commit raises): left_pos + own cells > max_terms, a caller stride that is too small, an
unsorted atmosphere map, max_terms over the cap, boundary slots without fcx_set_atmos_terms."""
import ctypes
import os
import re

import numpy as np
import pytest

from fcx import _lib
from fcx.engine import Engine
from fcx.parallel import LocalAtmos, local_atmos, synthetic_atmos_map
from fcx.synthetic import build_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "components.flux_calculator_amd")
E_ARG, E_STATE = 1, 2
OPT = 26
CAP = 4096
FIELDS = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))
NEW = ("fcx_set_atmos_terms", "fcx_atmos_columns", "fcx_atmos_invariant")


def test_symbols_exported_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "fcx.h")).read()
    f90 = open(os.path.join(PKG, "fortran", "fcx_c_api.F90")).read()
    dropin = open(os.path.join(PKG, "fortran", "flux_calculator_calculate.F90")).read()
    for name in NEW:
        assert getattr(lib, name) is not None
        assert re.search(rf"\bint {name}\(", header), name
        assert f"BIND(C, name='{name}')" in f90, name
    assert "int fcx_set_atmos_terms(fcx_engine *e, int32_t max_terms, int32_t left_pos);" in header
    assert "int fcx_atmos_columns(const fcx_engine *e, int32_t *columns);" in header
    assert "SUBROUTINE fcx_define_atmos_terms(max_terms, left_pos)" in dropin
    assert re.search(r"PUBLIC[^\n]*fcx_define_atmos_terms", dropin)


def test_one_number_everywhere():
    header = open(os.path.join(ROOT, "include", "fcx.h")).read()
    m = re.search(r"FCX_OPT_ATMOS_INVARIANT\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == OPT
    assert _lib.FCX_OPT_ATMOS_INVARIANT == OPT and Engine.OPTIONS["atmos_invariant"] == OPT
    assert sorted(Engine.OPTIONS.values()).count(OPT) == 1
    f90 = open(os.path.join(PKG, "fortran", "fcx_c_api.F90")).read()
    m = re.search(r"FCX_OPT_ATMOS_INVARIANT\s*=\s*(\d+)", f90)
    assert m and int(m.group(1)) == OPT
    assert len(re.findall(rf"=\s*{OPT}\b", header[header.index("enum fcx_option"):])) == 1


def test_option_and_getter_round_trip():
    lib = _lib.load()
    h = ctypes.c_void_p()
    gs = (ctypes.c_int32 * 3)(64, 64, 64)
    assert lib.fcx_create(0, 1, gs, ctypes.byref(h)) == 0
    try:
        on, cols = ctypes.c_int32(-1), ctypes.c_int32(-1)
        assert lib.fcx_atmos_invariant(h, ctypes.byref(on)) == 0 and on.value == 0  # off by default
        assert lib.fcx_set_option(h, OPT, 1) == 0
        assert lib.fcx_atmos_invariant(h, ctypes.byref(on)) == 0 and on.value == 1
        assert lib.fcx_set_option(h, OPT, 0) == 0
        assert lib.fcx_atmos_invariant(h, ctypes.byref(on)) == 0 and on.value == 0
        for bad in (2, -1):
            assert lib.fcx_set_option(h, OPT, bad) == E_ARG
            assert b"atmos_invariant" in lib.fcx_last_error()
        assert lib.fcx_atmos_invariant(h, None) == E_ARG
        assert lib.fcx_atmos_columns(h, None) == E_ARG
        assert lib.fcx_set_atmos_terms(None, 4, 0) == E_ARG
        assert lib.fcx_atmos_columns(h, ctypes.byref(cols)) == 0 and cols.value == 0  # no fields yet
    finally:
        lib.fcx_destroy(h)


def engine(la, invariant=True, shared_stride=None, options=None):
    """an uncommitted engine over la (no GPU touched); shared_stride: caller slots of that stride"""
    c = build_case("CCLM", n=la.size, T=1, bias=True)
    outs = [np.zeros(max(la.n_atmos, 1)) for _ in FIELDS]
    atmos = {"local": la, "fields": [(2, 1, g, name, o) for (name, g), o in zip(FIELDS, outs)], "invariant": invariant}
    if shared_stride is not None:
        atmos["shared"] = (np.zeros(max(la.n_boundaries * shared_stride, 1)), shared_stride)
    else:
        atmos["own_boundaries"] = True
    return Engine(c.lf, 1, c.methods, corrections=c.corrections, atmos=atmos, options=options, commit=False)


def shard(rank=1, n=257):
    """one of two shards of a 3..5-cell map cut inside an atmosphere cell, two or more of whose
    exchange cells lie on the lower shard"""
    amap = synthetic_atmos_map(3 * n)
    k = next(i for i in range(n, 2 * n) if amap.atmos_index[i - 2] == amap.atmos_index[i])
    la = local_atmos(amap, rank, 2, ranges=[(0, k), (k, n)])
    assert (la.left >= 0 and la.left_pos >= 2) if rank else (la.right >= 0 and la.left < 0)
    return la


def refused(eng, *words):
    try:
        with pytest.raises(_lib.FcxError) as ex:
            eng.plan_check()
        assert ex.value.status == E_ARG, str(ex.value)
        for w in words:
            assert w in str(ex.value), str(ex.value)
    finally:
        eng.close()


def test_columns_follow_the_option():
    la = shard()
    eng = engine(la, invariant=False)
    try:
        assert not eng.atmos_invariant() and eng.atmos_columns() == len(FIELDS)
        eng.plan_check()
    finally:
        eng.close()
    eng = engine(la)
    try:
        assert eng.atmos_invariant() and eng.atmos_columns() == len(FIELDS) * (1 + la.max_terms)
        eng.plan_check()  # the well-formed case passes
    finally:
        eng.close()
    eng = engine(la, shared_stride=len(FIELDS) * (1 + la.max_terms))
    try:
        eng.plan_check()  # a caller stride of exactly the width
    finally:
        eng.close()


def test_left_pos_plus_own_over_max_terms():
    import dataclasses

    la = shard()
    own = int(np.count_nonzero(la.atmos_index == 0))
    small = dataclasses.replace(la, max_terms=la.left_pos + own - 1)
    refused(engine(small), f"left_pos {la.left_pos}", f"{own} exchange cells", f"max_terms {small.max_terms}")
    # the last cell of the lower shard
    lo = shard(rank=0)
    own = int(np.count_nonzero(lo.atmos_index == lo.n_atmos - 1))
    assert lo.right >= 0 and lo.left < 0
    refused(engine(dataclasses.replace(lo, max_terms=own - 1)), "last local atmosphere cell", f"max_terms {own - 1}")


def test_caller_stride_too_small():
    la = shard()
    need = len(FIELDS) * (1 + la.max_terms)
    refused(engine(la, shared_stride=need - 1), f"stride {need - 1}", str(need), f"max_terms {la.max_terms}")
    refused(engine(la, shared_stride=len(FIELDS)), f"stride {len(FIELDS)}")


def test_unsorted_map():
    n = 257
    amap = synthetic_atmos_map(n)
    perm = np.random.default_rng(5).permutation(amap.n_atmos).astype(np.int32)
    la = LocalAtmos(0, n, 0, amap.n_atmos, perm[amap.atmos_index], amap.weight, -1, -1, 0, 0, 4)
    refused(engine(la), "sorted atmosphere map", "unsorted")
    eng = engine(la, invariant=False)  # the same map without the option: the CSR path, as ever
    try:
        eng.plan_check()
    finally:
        eng.close()


def test_max_terms_over_the_cap_and_missing_terms():
    import dataclasses

    la = shard()
    refused(engine(dataclasses.replace(la, max_terms=CAP + 1)), f"max_terms {CAP + 1}", str(CAP))
    refused(engine(dataclasses.replace(la, max_terms=0)), "max_terms 0")
    eng = engine(dataclasses.replace(la, max_terms=CAP, left_pos=1))  # the cap itself is taken
    try:
        eng.plan_check()
    finally:
        eng.close()
    # the option through fcx_set_option alone, boundary slots, no fcx_set_atmos_terms
    refused(engine(la, invariant=False, options={"atmos_invariant": 1}), "fcx_set_atmos_terms")
    header = open(os.path.join(ROOT, "include", "fcx.h")).read()
    assert f"1 .. {CAP}" in header  # the documented cap
