"""Device-side field ranges (fcx_field_ranges, fcx_atmos_ranges) and the non-finite guard
(FCX_OPT_CHECK_FINITE) against the numpy restatement of tests/ranges.py.  The shapes are the
smallest at which the kernel can go wrong: the partial 16-B vector, the 128-cell wave tile and the
4096-cell layout tile on either side, two blocks, the tile-blocked mirrors at 8200 cells."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import received  # noqa: E402
from ranges import assert_range, expect  # noqa: E402
from fcx import _lib  # noqa: E402
from fcx.basic import PHASE_ALL, PHASE_EARLY, PHASE_NORMAL  # noqa: E402
from fcx.engine import Engine  # noqa: E402
from fcx.local_field import LocalFields  # noqa: E402
from fcx.parallel import AtmosMap, local_atmos, synthetic_atmos_map  # noqa: E402
from fcx.synthetic import as_dtype, build_case  # noqa: E402

STEP_T = 3600
TAIL = 64
SIZES = (1, 3, 127, 128, 129, 4095, 4096, 4097, 8200)
MIRRORS = {"zero_copy": 0}  # device mirrors of the host arrays (tile-blocked from two tiles on)


def engine_of(case, **kw):
    return Engine(case.lf, case.num_surface_types, case.methods, corrections=case.corrections,
                  averages=case.averages, **kw)


def on_device(case, tail=TAIL):
    """The case with every distinct array in device memory (FCX_MEM_DEVICE), `tail` cells longer
    than its grid, the tail holding NaN and +-1e300 so that a read past the grid shows."""
    import torch

    src = case.lf
    lf = LocalFields(src.grid_size, device="cuda:0", dtype=src.dtype)
    with np.errstate(over="ignore"):  # (fp32: the tail is NaN and +-Inf)
        junk = np.resize(np.array([np.nan, 1e300, -1e300, np.nan]), tail).astype(src.dtype)
    moved = {}
    for key, a in src.field.items():
        if id(a) not in moved:
            moved[id(a)] = torch.from_numpy(np.concatenate([a, junk])).to("cuda:0")
        lf.field[key] = moved[id(a)]
    lf.allocated, lf.put_to = set(src.allocated), dict(src.put_to)
    new = type(case)(**{**case.__dict__, "lf": lf})
    return new


def set_cells(t, values):
    import torch

    t[: values.shape[0]] = torch.from_numpy(values).to(t.device)


def patterns(n, dtype, rng):
    """(label, values[n]): the extremes and one NaN, one +Inf and one -Inf in turn at the first
    cell, the last cell, cells 4095 and 4096 and inside the partial last vector; the all-NaN,
    the all-equal and the signed-zeros field."""
    per = 16 // np.dtype(dtype).itemsize
    spots = sorted({p for p in (0, n - 1, 4095, 4096, (n // per) * per, n - 2) if 0 <= p < n})
    base = rng.uniform(-5.0, 5.0, n).astype(dtype)
    for p in spots:
        for label, v in (("max", 77.0), ("min", -77.0), ("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
            x = base.copy()
            x[p] = v
            yield f"{label}@{p}", x
    x = base.copy()
    x[spots[0]], x[spots[-1]] = np.nan, -np.inf  # first_bad is the lowest of several
    yield "nan+inf", x
    yield "all-nan", np.full(n, np.nan, dtype)
    yield "all-equal", np.full(n, 3.25, dtype)
    z = np.zeros(n, dtype)
    z[::2] = -0.0
    yield "zeros", z
    yield "plain", base


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_numpy(n, dtype):
    """Device-bound fields 64 cells longer than their grid; every pattern in TSUR, with 16 more
    slots in the same request (17 fields: two launches), answered in request order."""
    case = build_case("CCLM", n=n, T=1)
    if dtype == "float32":
        case = as_dtype(case, "float32")
    dev = on_device(case)
    rng = np.random.default_rng(n)
    eng = engine_of(dev)
    try:
        others = [k for k in dev.lf.field if k[2] != "TSUR" and k not in case.outputs][:16]
        assert len(others) == 16
        slots = [(1, 1, "TSUR")] + others
        for k in others:  # a pattern of its own per distinct array (aliases share it)
            x = rng.uniform(-1.0, 1.0, n).astype(dtype)
            x[rng.integers(0, n)] = rng.choice([np.nan, np.inf, 9.0])
            set_cells(dev.lf.field[k], x)
        want_others = [expect(dev.lf.field[k].cpu().numpy(), n) for k in others]
        for label, x in patterns(n, dtype, rng):
            set_cells(dev.lf.field[(1, 1, "TSUR")], x)
            got = eng.field_ranges(slots)
            assert_range(got[0], expect(x), (n, dtype, label))
            for k, g, w in zip(others, got[1:], want_others):
                assert_range(g, w, (n, dtype, label, k))
        assert eng.field_ranges([]) == []
    finally:
        eng.close()


def _after_step(case, options, arena=False):
    """ranges of every input and output of the step (fcx_check_fields names them; an array no
    plan reads is never uploaded) == numpy on the host arrays the step downloaded"""
    keep = None
    if arena:
        from fcx.host_alloc import Arena

        keep = Arena()
        keep.adopt(case.lf)
    eng = engine_of(case, options={**options, "check_finite": 3})
    try:
        eng.step(PHASE_ALL, STEP_T)
        slots = eng.check_fields(PHASE_ALL)
        assert set(case.outputs) <= set(slots) and len(slots) > len(case.outputs) + 8
        got = eng.field_ranges(slots)
        for k, g in zip(slots, got):
            assert_range(g, expect(case.lf.field[k], case.lf.grid_size[k[1] - 1]), (options, k))
        assert all(g.n_nan + g.n_inf == 0 for k, g in zip(slots, got) if k in case.outputs)
        return eng.device_layout(), eng.zero_copy_active()
    finally:
        eng.close()
        if keep is not None:
            keep.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_tile_blocked_mirrors_zero_copy_and_library_memory(dtype):
    def case():
        c = build_case("MOM5", n=8200, T=2, bias=True)
        return as_dtype(c, "float32") if dtype == "float32" else c

    (tile, stride), zc = _after_step(case(), MIRRORS)
    assert stride > tile and not zc  # the mirrors are tile-blocked
    _after_step(case(), {"zero_copy": 1})  # heap arrays through the mapped staging arena
    (tile, stride), zc = _after_step(case(), {"zero_copy": 1}, arena=True)
    assert stride == tile and zc  # the arrays in place, through the link
    _after_step(case(), {"zero_copy": 0}, arena=True)  # spans


def test_separate_grids_use_each_grids_size():
    case = build_case("CCLM", n=4100, T=1, sep_grids=(4097, 130))
    _after_step(case, MIRRORS)


def test_received_field_reports_the_exchange_grid_array():
    n = 8200
    n_src, src, dst, w = received.links("weighted", n)
    case = build_case("CCLM", n=n, T=1)
    source = received.source_values("TATM", n_src, np.float64)
    twin = received.expand(src, dst, w, source, n)
    rm = {"grid": 1, "n_src": n_src, "src": src, "dst": dst, "w": w,
          "fields": [(PHASE_NORMAL, 1, 1, "TATM", source)]}
    case.lf.field[(1, 1, "TATM")][:] = -1.0  # the engine no longer reads the exchange-grid array
    eng = engine_of(case, received=[rm], options=MIRRORS)
    try:
        eng.step(PHASE_ALL, STEP_T)
        got = eng.field_ranges([(1, 1, "TATM"), (0, 1, "TATM")])
        assert_range(got[0], expect(twin), "TATM(1,t)")
        assert_range(got[1], expect(twin), "TATM(0,t)")
    finally:
        eng.close()


def test_outputs_the_host_cannot_see():
    n = 4097
    plain = build_case("MOM5", n=n, T=1, bias=True)
    eng = engine_of(plain, options=MIRRORS)
    eng.step(PHASE_ALL, STEP_T)
    eng.close()
    qsur = plain.lf.field[(1, 1, "QSUR")].copy()

    case = build_case("MOM5", n=n, T=1, bias=True)
    eng = engine_of(case, options=MIRRORS, output_use={(1, 1, "QSUR"): "device"})
    try:
        eng.step(PHASE_ALL, STEP_T)
        assert_range(eng.field_ranges([(1, 1, "QSUR")])[0], expect(qsur), "FCX_OUT_DEVICE QSUR")
    finally:
        eng.close()

    case = build_case("MOM5", n=n, T=1, bias=True)
    eng = engine_of(case, options=MIRRORS, output_use={(1, 1, "QSUR"): "unread"})
    try:
        eng.step(PHASE_ALL, STEP_T)
        assert eng.output_info(1, 1, "QSUR") == 2  # the store was left out: the array is stale
        with pytest.raises(_lib.FcxError) as ex:
            eng.field_ranges([(1, 1, "TSUR"), (1, 1, "QSUR")])
        assert ex.value.status == 2 and "QSUR(1,t)" in str(ex.value) and "stale" in str(ex.value)
        with pytest.raises(_lib.FcxError) as ex:
            eng.field_ranges([(2, 1, "HLAT")])
        assert ex.value.status == 1 and "HLAT(2,t)" in str(ex.value) and "not bound" in str(ex.value)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_uniform_constant_is_answered_from_its_value(dtype):
    case = build_case("CCLM", n=4097, T=1)
    if dtype == "float32":
        case = as_dtype(case, "float32")
    value = 280.1  # (not a float)
    case.lf.set_constant("TATM", 1, 1, value)
    eng = engine_of(case, options=MIRRORS)
    try:
        eng.step(PHASE_ALL, STEP_T)
        kind = eng.constant_info(1, 1, "TATM")
        r = eng.field_ranges([(1, 1, "TATM")])[0]
        seen = float(np.float32(value)) if dtype == "float32" else value
        assert (r.min, r.max, r.n_nan, r.n_inf, r.first_bad) == (seen, seen, 0, 0, -1)
        assert eng.constant_info(1, 1, "TATM") == kind  # (1 in the fp64 CCLM launch: it stays a value)
        assert kind == (1 if dtype == "float64" else 2)
    finally:
        eng.close()


def holey_map(n, every=5):
    """synthetic_atmos_map with every `every`-th atmosphere cell left without an exchange cell"""
    m = synthetic_atmos_map(n)
    idx = (m.atmos_index + m.atmos_index // (every - 1)).astype(np.int32)
    return AtmosMap(idx, m.weight, int(idx[-1]) + 2)


ATM = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))


def atmos_rig(n, dtype, options, amap=None, variant="MOM5", weight_scale=None):
    case = build_case(variant, n=n, T=1, bias=True)
    if dtype == "float32":
        case = as_dtype(case, "float32")
    amap = holey_map(n) if amap is None else amap
    if weight_scale is not None:
        amap = AtmosMap(amap.atmos_index, amap.weight * weight_scale, amap.n_atmos)
    la = local_atmos(amap, 0, 1)
    outs = {name: np.full(la.n_atmos, np.nan, dtype) for name, _ in ATM}
    atm = {"local": la, "fields": [(PHASE_EARLY if name == "RBBR" else PHASE_NORMAL, 1, g, name, outs[name])
                                   for name, g in ATM]}
    return case, outs, engine_of(case, atmos=atm, options=options)


@pytest.mark.parametrize("dtype, records", [("float64", 0), ("float64", 1), ("float32", 0)])
def test_atmosphere_outputs(dtype, records):
    """Plain (tile-blocked) arrays, per-cell records forced at a small grid, an fp32 engine; the
    map has atmosphere cells without exchange cells, whose zero sums count.  With records the
    ranges are right before any download has happened."""
    n = 8200 * 4  # > 4096 atmosphere cells: two tiles of the atmosphere pool
    case, outs, eng = atmos_rig(n, dtype, {**MIRRORS, "atm_records": records})
    try:
        assert eng.atm_records() == bool(records)
        eng.upload(PHASE_ALL)
        eng.run(PHASE_ALL, STEP_T)
        early, normal = eng.atmos_ranges(PHASE_EARLY), eng.atmos_ranges(PHASE_NORMAL)
        both = eng.atmos_ranges(PHASE_ALL)
        assert (len(early), len(normal), len(both)) == (1, 5, 6)
        eng.download(PHASE_ALL)
        eng.synchronize()
        for (name, _), r in zip(ATM, both):
            assert_range(r, expect(outs[name]), (dtype, records, name))
            assert r.min <= 0.0 <= r.max and r.n_nan == 0  # the empty cells' zeros take part
        assert_range(early[0], expect(outs["RBBR"]), "early")
        for r, (name, _) in zip(normal, [a for a in ATM if a[0] != "RBBR"]):
            assert_range(r, expect(outs[name]), ("normal", name))
        assert both == eng.atmos_ranges(PHASE_ALL)  # ... and after the download too
    finally:
        eng.close()


# ---- the guard

def _outputs(case, outs=None):
    got = {k: np.array(case.lf.field[k], copy=True) for k in case.outputs}
    for name, a in (outs or {}).items():
        got[("atm", name)] = a.copy()
    return got


def _same_bytes(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("T", [1, 2])
def test_clean_steps_are_bit_identical_with_the_guard(T, dtype):
    """fcx_step and fcx_step_async + fcx_synchronize with option 3 return FCX_OK and every output
    is the bytes of an engine without the option (T = 1 with the atmosphere accumulation; T = 2:
    the Baltic set-up's two types and their type-0 averages)."""
    n = 8200
    res = {}
    for check in (0, 3):
        for how in ("step", "async"):
            options = {**MIRRORS, "check_finite": check}
            if T == 1:
                case, outs, eng = atmos_rig(n, dtype, options)
            else:
                case = build_case("MOM5", n=n, T=2, bias=True)
                case = as_dtype(case, "float32") if dtype == "float32" else case
                outs, eng = None, engine_of(case, options=options)
            try:
                if how == "step":
                    eng.step(PHASE_ALL, STEP_T)
                else:
                    eng.step_async(PHASE_ALL, STEP_T)
                    eng.synchronize()
                assert eng.check_result() is None
                res[(check, how)] = _outputs(case, outs)
            finally:
                eng.close()
    for how in ("step", "async"):
        _same_bytes(res[(3, how)], res[(0, how)])


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_clean_group_run_is_bit_identical_and_keeps_its_members(precision):
    """CCLM + MOM5 + RCO device-resident on one stream (fcx.workload): the merged launch has its
    three members with and without the option, and every output is the same bytes."""
    import torch
    from test_gpu_group import outputs
    from fcx.workload import Workload

    res, sizes = {}, {}
    for check in (0, 3):
        wl = Workload(70_001, 0, 1, ("CCLM", "MOM5", "RCO"), precision=precision, atmos=True, atmos_map="random",
                      engine_options={"check_finite": check})
        try:
            wl.run_group(0)
            wl.run_group(3600)
            torch.cuda.synchronize()
            sizes[check] = [e.last_group_size() for e in wl.engines]
            assert all(e.check_result() is None for e in wl.engines)
            res[check] = outputs(wl)
        finally:
            wl.close()
    assert sizes[3] == sizes[0] == [3, 3, 3]
    _same_bytes(res[3], res[0])


def _first_hit(case, keys, n_of):
    """the first of `keys` (slot order) holding a non-finite value on the host, with numpy's answer"""
    for k in sorted(keys, key=lambda k: (k[0], k[1], _lib_idx(k[2]))):
        r = expect(case.lf.field[k], n_of(k))
        if r.first_bad >= 0:
            return k, r
    return None, None


def _lib_idx(name):
    from fcx.basic import IDX

    return IDX[name]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_a_nan_in_tatm_is_named_then_repaired(dtype):
    n, cell = 8200, 4097
    for check in (3, 1):
        case = build_case("CCLM", n=n, T=1)
        case = as_dtype(case, "float32") if dtype == "float32" else case
        tatm = case.lf.field[(1, 1, "TATM")]
        good = tatm[cell]
        tatm[cell] = np.nan
        twin = build_case("CCLM", n=n, T=1)
        twin = as_dtype(twin, "float32") if dtype == "float32" else twin
        twin.lf.field[(1, 1, "TATM")][cell] = np.nan
        te = engine_of(twin, options=MIRRORS)
        te.step(PHASE_ALL, STEP_T)
        te.close()
        eng = engine_of(case, options={**MIRRORS, "check_finite": check})
        try:
            with pytest.raises(_lib.NonFiniteError) as ex:
                eng.step(PHASE_ALL, STEP_T)
            err = ex.value
            assert err.status == 7 and not err.is_atmos
            _same_bytes(_outputs(case), _outputs(twin))  # fcx_step still downloaded
            if check & 2:
                assert (err.name, err.surface_type, err.grid, err.cell) == ("TATM", 0, 1, cell)
                assert np.isnan(err.value)
                assert f"TATM(0,t) cell {cell} = nan (1 NaN, 0 Inf of {n} cells)" in str(err), str(err)
                assert "phase 3" in str(err)
            else:
                # outputs only: the first output in slot order that the NaN reaches, by numpy
                k, r = _first_hit(twin, twin.outputs, lambda k: n)
                assert k is not None
                assert (err.surface_type, err.grid, err.name, err.cell) == (k[0], k[1], k[2], r.first_bad)
                stored = twin.lf.field[k][r.first_bad]
                assert (np.isnan(err.value) and np.isnan(stored)) or err.value == stored
                assert f"{r.n_nan} NaN, {r.n_inf} Inf" in str(err)
            assert eng.check_result()["cell"] == err.cell
            tatm[cell] = good
            eng.step(PHASE_ALL, STEP_T)  # repaired: FCX_OK
            assert eng.check_result() is None
            # ... and fcx_step_async defers the verdict to fcx_synchronize
            tatm[cell] = np.inf
            eng.step_async(PHASE_ALL, STEP_T)
            with pytest.raises(_lib.NonFiniteError):
                eng.synchronize()
            eng.synchronize()  # reported once
        finally:
            eng.close()


def test_an_overflow_in_an_atmosphere_output_only():
    """A finite sensible heat flux of the order of 1e300 (CHEA scales it linearly; the surface is
    warmer than the air everywhere, so it has one sign) and map weights of 1e10: the flux array is
    finite, the weighted sums overflow, and the report names the atmosphere output."""
    n = 4097
    case, outs, eng = atmos_rig(n, "float64", {**MIRRORS, "check_finite": 1}, weight_scale=1e10,
                                amap=synthetic_atmos_map(n))
    try:
        case.lf.field[(1, 1, "CHEA")][:] = 1e296
        case.lf.field[(1, 1, "TATM")][:] = 250.0
        with pytest.raises(_lib.NonFiniteError) as ex:
            eng.step(PHASE_ALL, STEP_T)
        err = ex.value
        hsen = case.lf.field[(1, 1, "HSEN")]
        # (calm cells have a smaller flux: one sign, finite, and of the order of 1e300 where it blows)
        assert np.isfinite(hsen).all() and 0.0 < hsen.min() and 1e300 < hsen.max() < 1e305, (hsen.min(), hsen.max())
        want = expect(outs["HSEN"])
        assert want.n_inf > 0 and want.n_nan == 0
        assert err.is_atmos and (err.name, err.surface_type, err.grid) == ("HSEN", 1, 1)
        assert err.cell == want.first_bad and err.value == np.inf
        assert f"atmosphere output HSEN(1,t) cell {want.first_bad} = inf (0 NaN, {want.n_inf} Inf" in str(err), str(err)
    finally:
        eng.close()


def test_a_chunked_host_step_checks_once_and_finds_the_last_chunk():
    n = 8200
    case = build_case("CCLM", n=n, T=1)
    case.lf.field[(1, 1, "TATM")][n - 3] = np.nan
    eng = engine_of(case, options={"zero_copy": 0, "pipeline_min_chunk": 1024, "pipeline_chunks": 4,
                                   "check_finite": 3})
    try:
        with pytest.raises(_lib.NonFiniteError) as ex:
            eng.step(PHASE_ALL, STEP_T)
        assert (ex.value.name, ex.value.cell) == ("TATM", n - 3) and f"of {n} cells" in str(ex.value)
        assert np.isnan(case.lf.field[(1, 1, "HSEN")][n - 3])  # the step completed its downloads
        assert np.isfinite(case.lf.field[(1, 1, "HSEN")][: n - 3]).all()
    finally:
        eng.close()
