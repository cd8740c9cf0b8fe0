"""Outputs the host never takes (fcx_set_output_use) inside the guard-band arena.

Every array of the case is carved out of ONE allocation with sentinel bands on both sides
(tests/guards.py).  The kernels now run flux blocks whose store pointer is null and guard only
the store, on grids with a partial last vector; the transports leave the declared arrays out.
After a step: no band element differs from its sentinel (no byte outside an output is written,
before or after any array), no pure input changed, and the host arrays of the declared outputs
-- counted as never-written regions, like inputs -- hold the bits they held before the commit.
The outputs still read are the twin's (the same case in an arena of its own, nothing declared).
Cases 1, 2 and 5 of tests/test_gpu_output_use.py, once each per memory kind."""
import numpy as np
import pytest

from guards import GuardedArena
from parity import bits_equal

pytestmark = pytest.mark.gpu

from fcx import _lib  # noqa: E402
from fcx.basic import PHASE_ALL, PHASE_NORMAL  # noqa: E402
from fcx.engine import Engine  # noqa: E402
from fcx.parallel import BlockedRandomAtmosMap  # noqa: E402
from fcx.synthetic import build_case  # noqa: E402

T_STEP = 3600 * 24 * 45
N = 4096 + 128 + 3
SEP = (4099, 4225)
DEVICE, UNREAD = _lib.FCX_OUT_DEVICE, _lib.FCX_OUT_UNREAD
ATM_FIELDS = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))
ALL_SEVEN = {(1, 1, "QSUR"): UNREAD, (1, 1, "MEVA"): UNREAD, (1, 1, "HLAT"): UNREAD, (1, 1, "HSEN"): UNREAD,
             (1, 1, "RBBR"): UNREAD, (1, 2, "UMOM"): UNREAD, (1, 3, "VMOM"): UNREAD}


def guarded_pair(make, use, backend, atmos=False, options=None, kinds=None, label=""):
    res = []
    for declare in (True, False):
        case = make()
        n = case.lf.grid_size[0]
        la = BlockedRandomAtmosMap().local(0, n, 0, 1, n, ranges=[(0, n)]) if atmos else None
        arena = GuardedArena.for_case(case, backend, extra=[la.n_atmos] * len(ATM_FIELDS) if atmos else ())
        eng = None
        try:
            kw, outs = {}, {}
            if atmos:
                outs = {name: arena.empty(la.n_atmos, ("atm", name), tail=0) for name, _ in ATM_FIELDS}
                kw["atmos"] = {"local": la, "fields": [(PHASE_NORMAL, 1, g, name, outs[name]) for name, g in ATM_FIELDS]}
            declared = set()
            if declare:  # the declared host arrays: regions no run may write
                for r in arena.regions:
                    if r.key in case.lf.field and any(case.lf.field[r.key] is case.lf.field[k] for k in use):
                        r.output = False
                        declared.add(id(case.lf.field[r.key]))
                assert len(declared) == len({id(case.lf.field[k]) for k in use})
            arena.snapshot()
            eng = Engine(case.lf, case.num_surface_types, case.methods, corrections=case.corrections,
                         averages=case.averages, output_use=use if declare else None, options=options or {}, **kw)
            eng.step(PHASE_ALL, T_STEP)
            if declare and kinds:
                for k, want in kinds.items():
                    assert eng.output_info(*k) == want, (label, k, eng.output_info(*k))
            violations = arena.check()
            assert violations == [], f"{label} declare={declare}: {violations[:5]}"
            got = {k: v for k, v in arena.outputs(case).items() if id(case.lf.field[k]) not in declared}
            got.update({("atm", name): arena.host(a) for name, a in outs.items()})
            res.append(got)
        finally:
            if eng is not None:
                eng.close()
            arena.close()
    got, twin = res
    assert got and got.keys() <= twin.keys(), label
    for k in got:
        assert np.all(np.isfinite(got[k])), f"{label}: {k} not finite"
        assert bits_equal(got[k], twin[k]).all(), f"{label}: {k} differs from the twin"


@pytest.mark.parametrize("backend", ["numpy", "lib"])
@pytest.mark.parametrize("variant,sep", [("CCLM", None), ("MOM5", SEP)])
def test_one_unread_output_in_the_arena(variant, sep, backend):
    """Case 1: QSUR unread, not stored (kind 2); with separate grids QSUR of u and v too, whose
    blocks run with null pointers for the grids' momentum."""
    use = {(1, 1, "QSUR"): UNREAD}
    if sep:
        use.update({(1, 2, "QSUR"): UNREAD, (1, 3, "QSUR"): UNREAD})
    guarded_pair(lambda: build_case(variant, n=N, T=1, bias=True, sep_grids=sep), use, backend,
                 kinds={k: 2 for k in use}, label=f"{variant} sep={sep} {backend}")


@pytest.mark.parametrize("backend,options", [("numpy", {"zero_copy": 0}), ("lib", {})])
def test_fused_accumulation_with_every_flux_unread_in_the_arena(backend, options):
    """Case 2: the MOM5 halo launch stores none of its seven exchange-grid outputs."""
    guarded_pair(lambda: build_case("MOM5", n=N, T=1, bias=True), ALL_SEVEN, backend, atmos=True, options=options,
                 kinds={k: 2 for k in ALL_SEVEN}, label=f"fused {backend}")


@pytest.mark.parametrize("backend,options", [("numpy", {}), ("numpy", {"zero_copy": 0}), ("lib", {}),
                                             ("lib", {"zero_copy": 0})])
def test_kept_outputs_in_the_arena(backend, options):
    """Case 5: QSUR and HSEN kept on the device through the mapped arena, the staged mirrors,
    library arrays in place and as spans."""
    use = {(1, 1, "QSUR"): DEVICE, (1, 1, "HSEN"): DEVICE}
    guarded_pair(lambda: build_case("MOM5", n=N, T=1, bias=True), use, backend, options=options,
                 kinds={k: 1 for k in use}, label=f"kept {backend} {options}")
