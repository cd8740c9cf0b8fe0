"""fp32 engines with several surface types: the exchange -> atmosphere accumulation of the
type-0 averages rides inside the flux launch (fused register-average kernels for float and for
FCX_OPT_F32_MATH), and fcx_run_group merges such engines into one launch.

No new rule, only the existing ones:
  - plain fp32: every per-type flux and every type-0 average is the bits of the same engine
    without an atmosphere map (cells_kernel with register averages, the path before);
  - FCX_OPT_F32_MATH: every output is np.float32(fp64 twin), each average formed in the launch
    from unrounded values (tests/test_gpu_f32_math.py);
  - an atmosphere output is np.float32 of the sequential fp64 sum, in link order, of
    w * float64(the engine's own stored fp32 average): exact, no tolerance.
Shapes: a single cell, one 256-cell tile minus and plus one cell, a ragged last lane of four,
and 70,001 cells (several blocks) on maps with crossings, segments at the half-tile limit of
both tile sizes (64 cells) and empty atmosphere cells, with and without a grid cap."""
import numpy as np
import pytest

import oracle_lib

pytestmark = pytest.mark.gpu

from fcx import _lib  # noqa: E402
from fcx.basic import PHASE_ALL, PHASE_NORMAL  # noqa: E402
from fcx.engine import Engine, run_group  # noqa: E402
from fcx.parallel import local_atmos  # noqa: E402
from fcx.synthetic import as_dtype, build_case  # noqa: E402
from test_gpu_f32_math import ATM_FIELDS, STEP_T, WIDE, bits32, engine_of, run_wide_and_twin  # noqa: E402
from test_gpu_multirank import random_run_map  # noqa: E402

VARIANTS = ("CCLM", "MOM5", "RCO")
LENGTHS = [(1, 5), (1, 10), (40, 64), (0, 5)]
MODES = {"default": {}, "capped": {"max_blocks": 64}}
SMALL = [1, 255, 257, 4099]
# (n, run lengths, mode): the small shapes on short runs, the large one over lengths x modes
SHAPES = [(n, (1, 5), "default") for n in SMALL] + [(70_001, ln, m) for m in MODES for ln in LENGTHS]


def shape_id(shape):
    n, lengths, mode = shape
    return f"n{n}-runs{lengths[0]}_{lengths[1]}-{mode}"


def variant_and_types(shape):
    """T alternates between 2 and 3, the variant rotates over the cross, so that each of the
    three kernels meets every mode"""
    i = SHAPES.index(shape)
    n, lengths, mode = shape
    rot = i if n != 70_001 else list(MODES).index(mode) + LENGTHS.index(lengths)
    return VARIANTS[rot % 3], 2 + i % 2


def map_of(n, lengths):
    amap = random_run_map(n, lengths, seed=lengths[1] + 5)
    return amap, local_atmos(amap, 0, 1)


def atmos_kw(la, outs, s=0, fields=ATM_FIELDS):
    """the six type-0 fields (s = 0) registered as Workload does"""
    return {"atmos": {"local": la, "fields": [(PHASE_NORMAL, s, g, k, outs[k]) for k, g in fields]}}


def new_outs(la, dtype=np.float32, fields=ATM_FIELDS):
    return {k: np.full(max(la.n_atmos, 1), np.nan, dtype) for k, _ in fields}


def check_atmosphere(case32, amap, outs, label):
    """each atmosphere output: the sequential fp64 sum of the engine's own stored fp32 averages"""
    for k, g in ATM_FIELDS:
        avg = np.asarray(case32.lf.field[(0, g, k)], dtype=np.float64)
        want = np.float32(oracle_lib.atmos_accumulate(amap.atmos_index, amap.weight, avg, amap.n_atmos))
        np.testing.assert_array_equal(bits32(outs[k][:amap.n_atmos]), bits32(want), err_msg=f"{label}: atmosphere {k}")


# ---------------------------------------------------------------- 1: the path is taken
@pytest.mark.parametrize("options", [{}, WIDE], ids=["f32", "f32w"])
@pytest.mark.parametrize("T", [2, 3])
def test_fused_path_is_taken(T, options):
    c32 = as_dtype(build_case("MOM5", n=4099, T=T, bias=True), "float32")
    _, la = map_of(4099, (1, 5))
    eng = engine_of(c32, dict(options), **atmos_kw(la, new_outs(la)))
    try:
        assert eng.f32_math() == bool(options)
        assert eng.fused_accumulation(PHASE_ALL) is True
    finally:
        eng.close()


def test_not_fused_when_a_segment_exceeds_half_a_tile():
    c32 = as_dtype(build_case("MOM5", n=4099, T=2, bias=True), "float32")
    _, la = map_of(4099, (130, 140))
    eng = engine_of(c32, **atmos_kw(la, new_outs(la)))
    try:
        assert eng.fused_accumulation(PHASE_ALL) is False
    finally:
        eng.close()


def test_not_fused_when_a_field_is_not_a_register_average():
    """T = 2 with a type-1 flux registered: only the type-0 averages ride in a multi-type launch"""
    c32 = as_dtype(build_case("MOM5", n=4099, T=2, bias=True), "float32")
    _, la = map_of(4099, (1, 5))
    eng = engine_of(c32, **atmos_kw(la, new_outs(la), s=1, fields=(("MEVA", 1),)))
    try:
        assert eng.fused_accumulation(PHASE_ALL) is False
    finally:
        eng.close()


def test_fp64_single_type_reports_its_fused_path():
    case = build_case("CCLM", n=4099, T=1, bias=True)
    _, la = map_of(4099, (1, 5))
    eng = engine_of(case, **atmos_kw(la, new_outs(la, np.float64), s=1))
    try:
        assert eng.fused_accumulation(PHASE_ALL) is True
        with pytest.raises(_lib.FcxError) as ex:
            eng.fused_accumulation(4)
        assert ex.value.status == 1
    finally:
        eng.close()


# ---------------------------------------------------------------- 2: plain fp32, bits
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_plain_fp32_bits(shape):
    """The engine with the map against the same case on an engine without one: every per-type
    flux and every type-0 average identical as uint32; the atmosphere outputs by the float rule."""
    n, lengths, mode = shape
    variant, T = variant_and_types(shape)
    label = f"{variant} T={T} {shape_id(shape)}"
    amap, la = map_of(n, lengths)
    outs = new_outs(la)
    runs = []
    for with_map in (True, False):
        c32 = as_dtype(build_case(variant, n=n, T=T, bias=True, seed=23), "float32")
        eng = engine_of(c32, dict(MODES[mode]), **(atmos_kw(la, outs) if with_map else {}))
        try:
            if with_map:
                assert eng.fused_accumulation(PHASE_ALL), label
            eng.step(PHASE_ALL, STEP_T)
        finally:
            eng.close()
        runs.append(c32)
    fused, plain = runs
    assert fused.outputs == plain.outputs and any(k[0] == 0 for k in fused.outputs)
    for k in fused.outputs:
        a, b = fused.lf.field[k], plain.lf.field[k]
        assert a.dtype == np.float32 and np.isfinite(b).all(), (label, k)
        np.testing.assert_array_equal(bits32(a), bits32(b), err_msg=f"{label}: {k}")
    check_atmosphere(fused, amap, outs, label)


# ---------------------------------------------------------------- 3: wide, twin rule
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_wide_twin_rule(shape):
    n, lengths, mode = shape
    variant, T = variant_and_types(shape)
    label = f"f32w {variant} T={T} {shape_id(shape)}"
    amap, la = map_of(n, lengths)
    outs = new_outs(la)
    c32, got, _, _, averages = run_wide_and_twin(build_case(variant, n=n, T=T, bias=True, seed=23), MODES[mode], label,
                                                 atmos=lambda c: atmos_kw(la, outs))
    assert averages and set(averages) == {k for k in got if k[0] == 0}
    for k, rule in averages.items():
        assert rule.startswith("np.float32(twin)"), (label, k, rule)
    check_atmosphere(c32, amap, outs, label)
    # the path itself, for this shape and mode (run_wide_and_twin keeps its engine to itself: an
    # engine of the same case, options and map; a fall-back to atmos_kernel would meet the rules too)
    eng = engine_of(c32, {**MODES[mode], **WIDE}, **atmos_kw(la, new_outs(la)))
    try:
        assert eng.f32_math() and eng.fused_accumulation(PHASE_ALL), label
    finally:
        eng.close()


# ---------------------------------------------------------------- 4: group launch
def workload_outputs(wl):
    got = {}
    for i, (case, outs) in enumerate(zip(wl.cases, wl.atm_outs)):
        got.update({(i,) + k: np.array(case.lf.field[k], copy=True) for k in case.outputs})
        got.update({(i, "atm", name): np.array(outs[name], copy=True) for name, _ in ATM_FIELDS})
    return got


def same_bits(a, b, label):
    assert a.keys() == b.keys() and a, label
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all(), (label, k)
        np.testing.assert_array_equal(bits32(a[k]), bits32(b[k]), err_msg=f"{label}: {k}")


def grouped_against_single(types, precision, atmos_map):
    import torch

    from fcx.workload import Workload

    res = []
    for grouped in (False, True):
        wl = Workload(50_021, 0, 1, VARIANTS, types=types, precision=precision, bias=True, atmos=True,
                      atmos_map=atmos_map)
        try:
            assert all(e.fused_accumulation(PHASE_ALL) for e in wl.engines)
            for k in range(2):
                (wl.run_group if grouped else wl.run)(3600 * k)
            torch.cuda.synchronize()
            assert [e.last_group_size() for e in wl.engines] == [3 if grouped else 0] * 3
            wl.download()
            res.append(workload_outputs(wl))
        finally:
            wl.close()
    same_bits(res[0], res[1], f"group T={types} {precision} {atmos_map}")


@pytest.mark.parametrize("precision", ["f32", "f32w"])
@pytest.mark.parametrize("types", [2, 3])
def test_group_launch(types, precision):
    """CCLM + MOM5 + RCO as one launch against the engines run singly, two steps, on the random
    map (segments cross the tiles: crossing records and the group fix-up)."""
    grouped_against_single(types, precision, "random")


def test_group_launch_periodic_map():
    """a map without crossings: no records, no fix-up launch"""
    grouped_against_single(2, "f32", "periodic")


def test_group_does_not_merge_multi_type_with_single_type():
    """one fp32 T = 2 engine and one fp32 T = 1 engine in a list: two launches, the same bits"""
    import torch

    from fcx.workload import Workload

    res = []
    for grouped in (False, True):
        wls = [Workload(20_011, 0, 1, ("MOM5",), types=2, precision="f32", bias=True, atmos_map="random"),
               Workload(20_011, 0, 1, ("CCLM",), types=1, precision="f32", bias=True, atmos_map="random")]
        try:
            engines = [wl.engines[0] for wl in wls]
            assert all(e.fused_accumulation(PHASE_ALL) for e in engines)
            for k in range(2):
                if grouped:
                    run_group(engines, PHASE_ALL, 3600 * k)
                    for e in engines:
                        e.run_atmos(PHASE_ALL)
                else:
                    for wl in wls:
                        wl.run(3600 * k)
            torch.cuda.synchronize()
            assert [e.last_group_size() for e in engines] == [0, 0]
            got = {}
            for j, wl in enumerate(wls):
                wl.download()
                got.update({(j,) + k: v for k, v in workload_outputs(wl).items()})
            res.append(got)
        finally:
            for wl in wls:
                wl.close()
    same_bits(res[0], res[1], "T=2 + T=1 list")


# ---------------------------------------------------------------- 5: shard boundaries
def test_shared_boundary_slots_of_a_two_way_split():
    """Ranks 0 and 1 of a 2-way APPLE split in one process, an atmosphere cell straddling the cut:
    each rank's shared slots hold the fp64 link-order partial sum of w * float64(avg32) over its
    own cells of the boundary cell, exactly."""
    import torch

    from fcx.workload import Workload

    for rank in (0, 1):
        wl = Workload(20_011, rank, 2, ("MOM5",), types=2, precision="f32", bias=True, atmos_map="random")
        try:
            la = wl.la
            slot, cell = (la.right, la.n_atmos - 1) if rank == 0 else (la.left, 0)
            assert slot == 0 and (la.left if rank == 0 else la.right) == -1, "the cut must straddle an atmosphere cell"
            assert wl.engines[0].fused_accumulation(PHASE_ALL)
            wl.shared.fill_(float("nan"))  # (the launch writes its slots: one left out stays NaN)
            wl.run(0)
            torch.cuda.synchronize()
            shared = wl.shared.cpu().numpy()[:wl.stride].copy()
            wl.download()
            for col, (name, g) in enumerate(ATM_FIELDS):
                avg = np.asarray(wl.cases[0].lf.field[(0, g, name)], dtype=np.float64)
                want = 0.0
                for x in np.nonzero(la.atmos_index == cell)[0]:
                    want = want + la.weight[x] * avg[x]
                assert shared[col] == want, (rank, name, shared[col], want)
        finally:
            wl.close()


# ---------------------------------------------------------------- 6: declared fields
def test_declared_constant_and_unread_outputs():
    """T = 2 MOM5 with the ice type's FICE a namelist constant and select_outputs on: the unsent
    outputs are the set-up's own unsent_outputs() rule (the one Setup.engine(select_outputs=True)
    declares) applied to this case with the six type-0 averages as the host's output fields --
    every computed output of types 1..T and the TSUR average.  (The namelist set-ups themselves
    regrid and keep u / v arrays of their own, so their phase is never one fused launch.)  The
    register-average kernels take neither wave-uniform inputs nor the unstored path, so the
    constant is an engine-filled array and an output an average consumes keeps a device array;
    every output still read -- the sent averages and the atmosphere outputs -- is the bits of the
    undeclared engine."""
    from types import SimpleNamespace

    from fcx.setup import FluxCalculatorSetup
    from test_gpu_constant_fields import declare

    n = 4096 + 256 + 5
    amap, la = map_of(n, (1, 10))
    res = []
    for declared in (True, False):
        c32 = as_dtype(build_case("MOM5", n=n, T=2, bias=True), "float32")
        declare(c32, {(2, "FICE"): 0.3})
        host = SimpleNamespace(local_field=c32.lf, averages=lambda: c32.averages,
                               output_field=[SimpleNamespace(slot=(0, g, k)) for k, g in ATM_FIELDS])
        host.computed_slots = lambda: FluxCalculatorSetup.computed_slots(host)
        unsent = FluxCalculatorSetup.unsent_outputs(host)
        assert {k for k in unsent if k[0] == 0} == {(0, 1, "TSUR")}
        assert {k for k in c32.outputs if k[0] >= 1} <= set(unsent) and len(unsent) == 19  # (+ the QSUR(u / v) slots)
        unread = {slot: _lib.FCX_OUT_UNREAD for slot in unsent}  # (Setup.engine's select_outputs)
        outs = new_outs(la)
        eng = Engine(c32.lf, 2, c32.methods, corrections=c32.corrections, averages=c32.averages,
                     use_constants=declared, output_use=unread if declared else None, **atmos_kw(la, outs))
        try:
            assert eng.fused_accumulation(PHASE_ALL)
            if declared:
                assert {k[2] for k in eng.constants} == {"FICE"}
            eng.step(PHASE_ALL, STEP_T)
            if declared:
                assert eng.constant_info(2, 1, "FICE") == 2  # an array the engine filled
                assert {eng.output_info(*k) for k in unread} <= {1, 2}
        finally:
            eng.close()
        got = {k: np.array(c32.lf.field[k], copy=True) for k in c32.outputs if k[0] == 0 and k not in unread}
        got.update({("atm", k): outs[k].copy() for k, _ in ATM_FIELDS})
        res.append(got)
        if not declared:
            check_atmosphere(c32, amap, outs, "undeclared")
    same_bits(res[0], res[1], "declared against undeclared")
