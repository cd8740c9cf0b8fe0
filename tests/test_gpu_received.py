"""Received fields on the GPU (fcx_bind_received): model-grid sources gathered to the exchange
grid by the engine.

The expected value everywhere is a TWIN engine (tests/received.py): the same case with the
exchange-grid arrays bound as ordinary arrays that the numpy restatement of the map expanded on
the host.  Every output of the receiving engine equals the twin's bit for bit.  In the receiving
engine the released exchange-grid host arrays are overwritten with NaN once the engine is
committed: finite outputs equal to the twin's show they are never read again.

Grids: geometric_maps(12) (784 exchange cells, 144 atmosphere and 289 ocean cells, runs of 4-9;
not a multiple of the 128- or 256-cell wave tile), geometric_maps(28) (4,225 cells: one 4,096-cell
layout tile and a bit) and n = 301 for the partial vector."""
import ctypes

import numpy as np
import pytest

import namelists
import received
from received import ATMOS, Declared, geometric, links, pair, same, snapshot, standard

pytestmark = pytest.mark.gpu

from fcx import _lib, driver, host_alloc  # noqa: E402
from fcx.basic import IDX, PHASE_ALL, PHASE_EARLY, PHASE_NORMAL  # noqa: E402
from fcx.engine import Engine, run_group  # noqa: E402
from fcx.parallel import geometric_maps, local_atmos  # noqa: E402
from fcx.setup import setup_from_namelist  # noqa: E402
from fcx.synthetic import SyntheticCoupler, as_dtype, build_case, build_regrid_case, corrections  # noqa: E402

T_STEP = 3600 * 24 * 45
FLUXES = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))


def step_all(eng, case, decl):
    eng.step(PHASE_ALL, T_STEP)


def geo_declare(side):
    n, atm, oce = geometric(side)
    return n, (lambda case: standard(case, atm, oce))


# ---------------------------------------------------------------- the variants, T = 1
@pytest.mark.parametrize("specialize", [1, 0])
@pytest.mark.parametrize("variant", ["CCLM", "MOM5", "RCO"])
def test_variants_t1(variant, specialize):
    """Atmosphere inputs through the transposed atmosphere map, TSUR and FICE through the
    transposed ocean map; aliases of the declared type-0 slots report received too."""
    n, declare = geo_declare(12)
    assert n == 784

    def check(eng, case, decl):
        for v in ("PSUR", "UATM"):
            if (1, 1, v) in case.lf.field:
                assert eng.received_info(1, 1, v) == (1, eng.received_info(0, 1, v)[1])
                assert eng.received_info(1, 3, v)[0] == 1  # the v grid IS the t grid
        assert eng.received_info(1, 1, "MEVA") == (0, -1)
        with pytest.raises(_lib.FcxError) as ex:  # set-up calls after the commit
            eng.add_receive_map(1, 1, [0], [0], [1.0])
        assert ex.value.status == 2
        with pytest.raises(_lib.FcxError) as ex:
            eng.bind_received(0, PHASE_NORMAL, 0, 1, "PSUR", decl.sources[(0, 1, "PSUR")])
        assert ex.value.status == 2

    for cpt in (2, 1):
        pair(lambda: build_case(variant, n=n, T=1, bias=True), declare, step_all, check=check,
             engine_kw={"options": {"specialize": specialize, "cells_per_thread": cpt}},
             label=f"{variant} spec={specialize} cpt={cpt}")


# ---------------------------------------------------------------- T = 2, the Baltic shape
def atmos_of(case, amap, s0, fields=FLUXES, phase=PHASE_NORMAL):
    la = local_atmos(amap, 0, 1)
    dtype = np.dtype(case.lf.dtype)
    outs = {name: np.full(max(la.n_atmos, 1), np.nan, dtype=dtype) for name, _ in fields}
    kw = {"atmos": {"local": la, "fields": [(phase, s0, g, name, outs[name]) for name, g in fields]}}
    return kw, {("atm", name): a for name, a in outs.items()}


def test_baltic_shape_t2_fused_accumulation():
    """MOM5 water + ice with bias, register averages and the accumulation fused into the flux
    launch, on the 4,225-cell grid."""
    amap, _ = geometric_maps(28)
    n, declare = geo_declare(28)
    assert n == 4225

    def check(eng, case, decl):
        assert eng.fused_accumulation(PHASE_ALL)

    pair(lambda: build_case("MOM5", n=n, T=2, bias=True), declare, step_all,
         extra=lambda c: atmos_of(c, amap, 0), check=check, label="Baltic T=2")


# ---------------------------------------------------------------- separate u / v grids
@pytest.mark.parametrize("variant", ["CCLM", "MOM5"])
def test_separate_uv_grids_each_with_its_own_map(variant):
    sizes = (301, 310, 290)
    maps = {g: links("unit" if g != 2 else "weighted", sizes[g - 1], seed=g) for g in (1, 2, 3)}
    pair(lambda: build_case(variant, n=301, T=1, bias=True, sep_grids=(310, 290)),
         lambda case: standard(case, maps, None), step_all, label=f"{variant} sep grids")


# ---------------------------------------------------------------- the forms of a map
@pytest.mark.parametrize("n", [301, 4225])
@pytest.mark.parametrize("kind", ["unit", "weighted", "general", "empty"])
def test_map_forms(kind, n):
    """Injection with unit weights, injection with weights, the general form (two links per
    cell in a shuffled order) and a map with cells without a link (0.0 there: FICE, UATM and
    VATM only, where a zero is a physical value)."""
    m = links(kind, n)
    if kind == "empty":
        plain = links("unit", n)

        def declare(case):
            d = standard(case, plain, None)
            d.maps[("hole", 1)] = (1, m)
            for v in ("UATM", "VATM"):
                d.fields[(0, 1, v)] = (("hole", 1), PHASE_NORMAL)
            return Declared(case, d.maps, d.fields)
    else:
        def declare(case):
            return standard(case, m, m)
    pair(lambda: build_case("CCLM", n=n, T=1, bias=True), declare, step_all, label=f"{kind} n={n}")


# ---------------------------------------------------------------- fp32 engines
@pytest.mark.parametrize("f32_math", [0, 1])
@pytest.mark.parametrize("kind,n", [("unit", 784), ("weighted", 301), ("general", 4225), ("empty", 301)])
def test_fp32_engines(kind, n, f32_math):
    m = links(kind, n)
    fields = ("UATM", "VATM") if kind == "empty" else ATMOS

    def declare(case):
        return standard(case, m, None if kind == "empty" else m, atmos=fields)

    pair(lambda: as_dtype(build_case("MOM5", n=n, T=1, bias=True), "float32"), declare, step_all,
         engine_kw={"options": {"f32_math": f32_math}}, label=f"fp32 {kind} n={n} math={f32_math}")


# ---------------------------------------------------------------- two launches of one map
def test_more_than_16_fields_on_one_map():
    n = 784
    m = links("weighted", n)
    bottom = ("TSUR", "FICE", "CMOI", "CHEA", "CMOM", "FARE")
    decls = []

    def declare(case):
        d = standard(case, m, m, bottom=bottom)
        d.maps = {("atm", 1): d.maps[("atm", 1)]}  # ONE map for every field
        d.fields = {k: (("atm", 1), ph) for k, (_, ph) in d.fields.items()}
        decls.append(d)
        return d

    pair(lambda: build_case("MOM5", n=n, T=3, bias=True), declare, step_all, label="26 fields")
    assert len(decls[0].fields) == 8 + 3 * 6 > 16


# ---------------------------------------------------------------- regridding and other readers
def test_received_field_as_regrid_source():
    """The t grid's atmosphere fields and TSUR(1, t) are received; UATM(1, t) is regridded to the
    u grid, whose fields are ordinary arrays (do_regridding reads the device array as last
    gathered: fcx_receive first); the step then runs the regridding engine's staged sequence on
    300 / 310 / 290 cells."""
    sizes = (300, 310, 290)
    maps = {g: links("unit", sizes[g - 1], seed=g) for g in (1, 2, 3)}
    oce = links("weighted", 300, seed=9)

    def make():
        case = build_regrid_case("CCLM", n=300, sep_grids=(310, 290), T=2, bias=True)
        case.lf.put_to[(1, 1, "UATM")] = 2
        return case

    def declare(case):
        d = standard(case, maps, None)
        fields = {k: v for k, v in d.fields.items() if k[1] == 1}
        fields[(1, 1, "TSUR")] = (("oce", 1), PHASE_EARLY)
        return Declared(case, {("atm", 1): d.maps[("atm", 1)], ("oce", 1): (1, oce)}, fields)

    def run(eng, case, decl):
        eng.receive(PHASE_ALL)
        eng.do_regridding("UATM", 1)
        eng.step(PHASE_ALL, T_STEP)

    def extra(case):
        return {}, {("host", "UATM_u"): case.lf.field[(1, 2, "UATM")]}

    pair(make, declare, run, extra=extra, label="regrid source")


def test_received_tsur_accumulated_and_remapped():
    amap, omap = geometric_maps(12)
    n, declare = geo_declare(12)

    def extra(case):
        kw, arrays = atmos_of(case, amap, 1, fields=(("TSUR", 1), ("MEVA", 1)), phase=PHASE_NORMAL)
        outs = {name: np.full(omap.n_model, np.nan) for name in ("TSUR", "HSEN")}
        kw["remaps"] = [{"n_dst": omap.n_model, "src": omap.src, "dst": omap.dst, "w": omap.weight,
                         "fields": [(PHASE_NORMAL, 1, 1, name, outs[name]) for name in outs]}]
        arrays.update({("remap", k): a for k, a in outs.items()})
        return kw, arrays

    pair(lambda: build_case("CCLM", n=n, T=1, bias=True), declare, step_all, extra=extra, label="TSUR readers")


# ---------------------------------------------------------------- phases and time
def test_early_and_normal_phases_in_a_time_loop():
    """Three coupling steps, each the early phase then the normal phase, the sources renewed
    before every step: every step's outputs equal the twin's (no stale gather)."""
    n, declare = geo_declare(12)
    traces = []

    def run(eng, case, decl):
        trace = []
        for k in range(3):
            for key, a in decl.sources.items():
                a[:] = received.source_values(key[2], a.shape[0], a.dtype, step=k + 1)
            if not eng.receive_maps:
                decl.fill_exchange(case)
            eng.step(PHASE_EARLY, 600 * k)
            eng.step(PHASE_NORMAL, 600 * k)
            trace.append(snapshot(case))
        traces.append(trace)

    pair(lambda: build_case("MOM5", n=n, T=2, bias=True), declare, run, label="time loop")
    for k in range(3):
        same(traces[0][k], traces[1][k], f"time loop step {k}")
    assert any(not np.array_equal(traces[0][0][key], traces[0][2][key]) for key in traces[0][0])


def test_per_call_subroutines_after_receive():
    n, declare = geo_declare(12)

    def run(eng, case, decl):
        lib, h = eng.lib, eng.h
        eng.receive(PHASE_ALL)
        _lib.check(lib.fcx_calc_flux_radiation_blackbody(h))
        for g in (1, 2, 3):
            _lib.check(lib.fcx_calc_spec_vapor_surface(h, g))
        _lib.check(lib.fcx_calc_flux_mass_evap(h, T_STEP))
        _lib.check(lib.fcx_calc_flux_heat_latent(h))
        _lib.check(lib.fcx_calc_flux_heat_sensible(h))
        _lib.check(lib.fcx_calc_flux_momentum_east(h, 2))
        _lib.check(lib.fcx_calc_flux_momentum_north(h, 3))
        for _, g, name in case.averages:
            _lib.check(lib.fcx_average_across_surface_types(h, g, IDX[name]))

    pair(lambda: build_case("CCLM", n=n, T=2, bias=True), declare, run, label="per call")


# ---------------------------------------------------------------- every transport of the source
def test_step_async_and_upload_field():
    n, declare = geo_declare(12)

    def run_async(eng, case, decl):
        eng.step_async(PHASE_ALL, T_STEP)
        for a in decl.sources.values():  # in the engine's hands: the host may overwrite them
            a[:] = np.nan
        eng.synchronize()

    def run_handed(eng, case, decl):
        for (s, g, name) in list(decl.fields)[::2]:  # half the fields handed over, one by one
            eng.upload_field(s, g, name)
        eng.upload_field(1, 1, "PSUR")  # an alias of a field already handed over
        eng.step(PHASE_ALL, T_STEP)

    pair(lambda: build_case("CCLM", n=n, T=1, bias=True), declare, run_async, label="step_async")
    pair(lambda: build_case("MOM5", n=n, T=1, bias=True), declare, run_handed, label="upload_field")


@pytest.mark.parametrize("zero_copy", [1, 0])
@pytest.mark.parametrize("lib_spans", [1, 0])
def test_library_memory(zero_copy, lib_spans):
    """Fields and sources in fcx_host_malloc memory: used in place, as spans, or by direct DMA."""
    n, atm, oce = geometric(12)
    with host_alloc.Arena() as arena:
        def make():
            case = build_case("CCLM", n=n, T=1, bias=True)
            arena.adopt(case.lf)
            return case

        def check(eng, case, decl):
            assert (eng.zero_copy_bytes() > 0) == bool(zero_copy)
            if zero_copy:  # in place: the sources are counted, the released arrays are not
                arrays = {id(a): a.nbytes for k, a in case.lf.field.items() if k not in released(case, decl)}
                arrays.update({id(a): a.nbytes for a in decl.sources.values()})
                assert eng.zero_copy_bytes() == sum(arrays.values())
            elif lib_spans:
                up, down = eng.span_runs(PHASE_ALL)
                assert up >= 1 and down >= 1

        pair(make, lambda case: standard(case, atm, oce, alloc=arena.empty), step_all, check=check,
             engine_kw={"options": {"zero_copy": zero_copy, "lib_spans": lib_spans}},
             label=f"library memory zc={zero_copy} spans={lib_spans}")


def released(case, decl):
    """every slot whose array a declaration released (the declared slots and their aliases)"""
    ids = {id(case.lf.field[k]) for k in decl.fields}
    return {k for k, a in case.lf.field.items() if id(a) in ids}


def test_device_memory_sources():
    import torch

    n, atm, oce = geometric(12)

    def declare(case):
        d = standard(case, atm, oce)
        d.host_sources = dict(d.sources)
        d.sources = {k: torch.as_tensor(a).to("cuda:0") for k, a in d.sources.items()}
        return d

    def declare_fill(case):
        d = declare(case)
        fill = d.fill_exchange

        def fill_exchange(c):
            dev, d.sources = d.sources, d.host_sources
            fill(c)
            d.sources = dev
        d.fill_exchange = fill_exchange
        return d

    def check(eng, case, decl):
        lay = eng.device_layout()
        assert lay[1] > lay[0], "device sources leave the field mirrors tile-blocked"

    pair(lambda: build_case("CCLM", n=n, T=1, bias=True), declare_fill, step_all, check=check,
         engine_kw={"options": {"zero_copy": 0}}, label="device sources")
    # ... and in an engine whose fields are device memory too (nothing moves over the link)
    def make_dev():
        return build_case("MOM5", n=n, T=1, bias=True, device="cuda:0")

    out = []
    for recv in (True, False):
        case = make_dev()
        host = build_case("MOM5", n=n, T=1, bias=True)
        d = standard(host, atm, oce)
        d.fill_exchange(host)
        for key in d.fields:
            case.lf.field[key].copy_(torch.as_tensor(host.lf.field[key]))
        kw = {}
        if recv:
            d.sources = {k: torch.as_tensor(a).to("cuda:0") for k, a in d.sources.items()}
            kw["received"] = d.engine_arg()
        eng = Engine(case.lf, 1, case.methods, corrections=case.corrections, **kw)
        try:
            if recv:
                for key in d.fields:
                    case.lf.field[key].fill_(float("nan"))
            eng.step(PHASE_ALL, T_STEP)
            out.append({k: case.lf.to_numpy(*k).copy() for k in case.outputs})
        finally:
            eng.close()
    same(out[0], out[1], "device fields and sources")


# ---------------------------------------------------------------- the chunked step
def test_pipelined_step_gathers_before_the_first_chunk():
    n, declare = geo_declare(28)
    amap, _ = geometric_maps(28)
    for tiled in (1, 0):
        pair(lambda: build_case("CCLM", n=n, T=1, bias=True), declare, step_all,
             extra=lambda c: atmos_of(c, amap, 1),
             engine_kw={"options": {"pipeline_min_chunk": 1024, "pipeline_chunks": 4, "zero_copy": 0,
                                    "tiled_layout": tiled}},
             label=f"chunked tiled={tiled}")


# ---------------------------------------------------------------- the group launch
def test_run_group_of_three_variants():
    import torch

    amap, _ = geometric_maps(28)
    n, atm, oce = geometric(28)
    la = local_atmos(amap, 0, 1)
    results = []
    for recv in (True, False):
        stream = torch.cuda.Stream()
        cases, engines, outs = [], [], []
        try:
            for v in ("CCLM", "MOM5", "RCO"):
                c = build_case(v, n=n, T=1, bias=True, seed=5)
                d = standard(c, atm, oce)
                d.fill_exchange(c)
                o = {name: np.full(la.n_atmos, np.nan) for name, _ in FLUXES}
                kw = {"atmos": {"local": la, "fields": [(PHASE_NORMAL, 1, g, name, o[name]) for name, g in FLUXES]}}
                if recv:
                    kw["received"] = d.engine_arg()
                engines.append(Engine(c.lf, 1, c.methods, corrections=c.corrections, stream=stream.cuda_stream,
                                      options={"zero_copy": 0}, **kw))
                if recv:
                    d.poison(c)
                cases.append(c)
                outs.append(o)
            for e in engines:
                e.upload(PHASE_ALL)
            run_group(engines, PHASE_ALL, T_STEP)
            for e in engines:
                e.download(PHASE_ALL)
                e.synchronize()
            sizes = [e.last_group_size() for e in engines]
            results.append((sizes, [snapshot(c, {("atm", k): a for k, a in o.items()}) for c, o in zip(cases, outs)]))
        finally:
            for e in engines:
                e.close()
    assert results[0][0] == results[1][0] == [3, 3, 3], (results[0][0], results[1][0])
    for k in range(3):
        same(results[0][1][k], results[1][1][k], f"group member {k}")


# ---------------------------------------------------------------- queries
def read_device(eng, ptr, n, dtype):
    tile, stride = eng.device_layout()
    rows = (n + tile - 1) // tile
    flat = np.empty((rows - 1) * stride + (n - (rows - 1) * tile), dtype=dtype)
    _lib.check(eng.lib.fcx_memcpy(ctypes.c_void_p(flat.ctypes.data), ctypes.c_void_p(ptr), flat.nbytes, 2))
    return np.concatenate([flat[r * stride: r * stride + min(tile, n - r * tile)] for r in range(rows)])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_device_ptr_holds_the_expanded_values(dtype):
    n, declare = geo_declare(28)

    def check(eng, case, decl):
        eng.synchronize()
        for key in ((0, 1, "TATM"), (1, 1, "FICE"), (1, 2, "UATM")):
            mkey, _ = decl.fields[key if key in decl.fields else (0, 1, key[2])]
            src_key = key if key in decl.fields else (0, 1, key[2])
            grid, (n_src, src, dst, w) = decl.maps[mkey]
            want = received.expand(src, dst, w, decl.sources[src_key], n, np.dtype(dtype))
            got = read_device(eng, eng.device_ptr(*key), n, np.dtype(dtype))
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), key

    pair(lambda: as_dtype(build_case("CCLM", n=n, T=1, bias=True), dtype), declare, step_all, check=check,
         label=f"device_ptr {dtype}")


@pytest.mark.parametrize("kind", ["unit", "weighted", "general"])
def test_algorithmic_and_staging_bytes(kind):
    """fcx_algorithmic_bytes: the twin's bytes plus, per gather launch, the map (injection: 4 B
    per exchange cell, + 8 B with weights; general: 4 (n + 1) + 12 links) and per field n_src
    elements read and n written.  fcx_staging_bytes (the mapped arena of a small grid's heap
    arrays, and the plain pool's image with zero-copy off): one 256-B rounded image per distinct
    heap array -- the sources, not the exchange-grid arrays they replace."""
    n = 784
    m = links(kind, n)
    n_src, n_links = m[0], m[1].size
    map_bytes = {"unit": 4 * n, "weighted": 12 * n, "general": 4 * (n + 1) + 12 * n_links}[kind]
    seen = {}

    def r256(b):
        return (b + 255) // 256 * 256

    def image(case, decl, recv):
        arrays = {id(a): a.nbytes for k, a in case.lf.field.items() if not (recv and k in released(case, decl))}
        if recv:
            arrays.update({id(a): a.nbytes for a in decl.sources.values()})
        return sum(r256(b) for b in arrays.values())

    for opts in ({}, {"zero_copy": 0, "tiled_layout": 0}):
        for recv in (True, False):
            case = build_case("MOM5", n=n, T=1, bias=True)
            decl = standard(case, m, m)
            decl.fill_exchange(case)
            eng = Engine(case.lf, 1, case.methods, corrections=case.corrections, options=opts,
                         received=decl.engine_arg() if recv else None)
            try:
                eng.step(PHASE_ALL, T_STEP)
                seen[recv] = (eng.algorithmic_bytes(PHASE_ALL), eng.algorithmic_bytes(PHASE_EARLY),
                              eng.algorithmic_bytes(PHASE_NORMAL))
                assert eng.staging_bytes() == image(case, decl, recv), (opts, recv)
            finally:
                eng.close()
        # two maps (atmosphere, ocean).  Early: the ocean map's launch of TSUR.  Normal: the
        # atmosphere map's launch of 8 fields and the ocean map's of FICE.  Both phases: two launches.
        assert len(decl.fields) == 10
        per_field = (n_src + n) * 8
        assert seen[True][1] - seen[False][1] == map_bytes + per_field
        assert seen[True][2] - seen[False][2] == 2 * map_bytes + 9 * per_field
        assert seen[True][0] - seen[False][0] == 2 * map_bytes + 10 * per_field


# ---------------------------------------------------------------- the Python time loop
class ModelGridCoupler(SyntheticCoupler):
    """get() of a field received on its model's grid fills the model-grid array; for the twin
    it fills the exchange-grid array with the host-side expansion of the same values."""

    def __init__(self, setup, maps):
        super().__init__(setup.grid_size, setup.num_surface_types)
        self.grid_of = {f.name: f.which_grid for f in setup.input_field}
        self.maps = maps

    def get(self, name, time, out, which_grid=None):
        n_src, src, dst, w = self.maps[name[1]]
        vals = received.source_values(name[2:6], n_src, out.dtype, step=1 + time // 60 + int(name[6:8]))
        out[:] = vals if out.shape[0] == n_src else received.expand(src, dst, w, vals, out.shape[0], out.dtype)


@pytest.mark.parametrize("which, mype, letter", [("MOM5_BALTIC", 0, "M"), ("CCLM_REGRID", 1, "M")])
def test_python_time_loop_with_receive_maps(which, mype, letter):
    n, atm, oce = geometric(12)
    grids = (n, n - 5, n + 3)
    assert atm[0] != n and oce[0] != n and atm[0] != oce[0]
    regrid = namelists.regrid_matrices(grids)
    corr = (20000101, corrections(grids[0])) if which == "MOM5_BALTIC" else None
    maps = {"A": atm, letter: oce}
    sent = []
    for recv in (True, False):
        setup = setup_from_namelist(getattr(namelists, which), mype=mype, grid_size=grids)
        kw = {"receive_maps": {k: {1: m} for k, m in maps.items()}} if recv else {}
        eng = setup.engine(corrections=corr, regrid=regrid, **kw)
        coupler = ModelGridCoupler(setup, maps)
        try:
            if recv:
                assert set(setup.source_field) == {f.name for f in setup.input_field}
                for f in setup.input_field:
                    assert eng.received_info(*f.slot)[0] == 1
                    setup.local_field.field[f.slot][:] = np.nan
            driver.run(setup, eng, coupler)
        finally:
            eng.close()
        sent.append(coupler.sent)
    assert sent[0].keys() == sent[1].keys() and sent[0]
    same(sent[0], sent[1], which)
