"""Received fields (fcx_bind_received) inside the guard-band arena.

Every array of the case and every model-grid source is carved out of ONE allocation with
sentinel bands on both sides (tests/guards.py); a source is bound longer than the map's n_src,
its tail holding sentinels.  After a step:
  * no band element differs from its sentinel: no byte outside an output is written, and
    nothing outside a source's n_src cells is read and used (a sentinel is a NaN: it would
    poison a result, and every output is finite and equal to the twin's);
  * no source and no other input changed;
  * the released exchange-grid host arrays, overwritten with NaN after the commit, hold those
    bits still (never written) and reach no result (never read);
  * the cells of a destination device array past its grid size, set to a pattern before the
    step, are untouched.
The twin is the same case in an arena of its own with the exchange-grid arrays expanded on the
host (tests/received.py)."""
import ctypes

import numpy as np
import pytest

import received
from guards import GuardedArena
from parity import bits_equal

pytestmark = pytest.mark.gpu

from fcx import _lib  # noqa: E402
from fcx.basic import PHASE_ALL  # noqa: E402
from fcx.engine import Engine  # noqa: E402
from fcx.synthetic import as_dtype, build_case  # noqa: E402

T_STEP = 3600 * 24 * 45
SRC_TAIL = 5  # sentinel cells a source is bound longer than n_src
PAST = 4      # cells of a destination past its grid that are watched


def past_cells(eng, key, n, dtype, write=None):
    """cells [n, n + PAST) of the device array behind slot `key`: written, or read back"""
    tile, stride = eng.device_layout()
    es = np.dtype(dtype).itemsize
    assert n % tile + PAST <= tile
    addr = eng.device_ptr(*key) + ((n // tile) * stride + n % tile) * es
    buf = np.array(write, dtype=dtype) if write is not None else np.empty(PAST, dtype=dtype)
    _lib.check(eng.lib.fcx_memcpy(ctypes.c_void_p(addr) if write is not None else ctypes.c_void_p(buf.ctypes.data),
                                  ctypes.c_void_p(buf.ctypes.data) if write is not None else ctypes.c_void_p(addr),
                                  buf.nbytes, 1 if write is not None else 2))
    return buf


def guarded_pair(make, declare, backend, options=None, label=""):
    res = []
    for recv in (True, False):
        case = make()
        dtype = case.lf.dtype
        decl = declare(case)
        decl.fill_exchange(case)
        n_srcs = {k: a.shape[0] for k, a in decl.sources.items()}
        arena = GuardedArena.for_case(case, backend, extra=[n + SRC_TAIL for n in n_srcs.values()])
        eng = None
        try:
            if recv:  # the sources: inputs with a sentinel tail, inside the arena
                for k, a in list(decl.sources.items()):
                    view = arena.empty(n_srcs[k], ("src",) + k, output=False, tail=SRC_TAIL)
                    if backend == "torch":
                        import torch

                        view[:n_srcs[k]].copy_(torch.from_numpy(a))
                    else:
                        view[:n_srcs[k]] = a
                    decl.sources[k] = view
                released = {id(case.lf.field[k]) for k in decl.fields}
                for r in arena.regions:  # the released host arrays: regions no run may write
                    if r.key in case.lf.field and id(case.lf.field[r.key]) in released:
                        r.output = False
            eng = Engine(case.lf, case.num_surface_types, case.methods, corrections=case.corrections,
                         averages=case.averages, options=options or {}, received=decl.engine_arg() if recv else None)
            watched = {}
            if recv:
                decl.poison(case)
                for k in decl.fields:
                    n = case.lf.grid_size[k[1] - 1]
                    watched[k] = past_cells(eng, k, n, dtype, write=[-7.0, 1e30, -0.0, 12345.0])
            arena.snapshot()
            eng.step(PHASE_ALL, T_STEP)
            eng.step(PHASE_ALL, T_STEP)
            violations = arena.check()
            assert violations == [], f"{label} recv={recv}: {violations[:5]}"
            for k, want in watched.items():
                got = past_cells(eng, k, case.lf.grid_size[k[1] - 1], dtype)
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (label, k, got)
            res.append(arena.outputs(case))
        finally:
            if eng is not None:
                eng.close()
            arena.close()
    got, twin = res
    assert got and got.keys() == twin.keys(), label
    for k in got:
        assert np.all(np.isfinite(got[k])), f"{label}: {k} not finite"
        assert bits_equal(got[k], twin[k]).all(), f"{label}: {k} differs from the twin"


@pytest.mark.parametrize("backend,options", [("numpy", {}), ("numpy", {"zero_copy": 0}),
                                             ("numpy", {"zero_copy": 0, "tiled_layout": 0}), ("lib", {}),
                                             ("lib", {"zero_copy": 0}), ("lib", {"zero_copy": 0, "lib_spans": 0}),
                                             ("torch", {})])
def test_intersection_grid_in_the_arena(backend, options):
    """CCLM on geometric_maps(12): the atmosphere fields through the transposed atmosphere map,
    TSUR and FICE through the transposed ocean map, in every kind of memory and transport."""
    n, atm, oce = received.geometric(12)
    guarded_pair(lambda: build_case("CCLM", n=n, T=1, bias=True), lambda c: received.standard(c, atm, oce),
                 backend, options=options, label=f"CCLM {backend} {options}")


@pytest.mark.parametrize("kind", ["weighted", "general", "empty"])
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_map_forms_and_the_partial_vector_in_the_arena(dtype, kind):
    """n = 301: the last vector of a destination is partial in both precisions; the weighted
    injection form, the general form, and a map with cells without a link."""
    m = received.links(kind, 301)
    fields = ("UATM", "VATM") if kind == "empty" else received.ATMOS

    def make():
        case = build_case("MOM5", n=301, T=1, bias=True)
        return as_dtype(case, dtype) if dtype == "float32" else case

    guarded_pair(make, lambda c: received.standard(c, m, None if kind == "empty" else m, atmos=fields), "numpy",
                 options={"zero_copy": 0}, label=f"{kind} {dtype}")
