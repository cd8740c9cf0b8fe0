"""Outputs the host never takes (fcx_set_output_use) on the GPU.

The oracle is a TWIN: the same deterministic case run by an engine with the declarations and by
one without.  A declaration changes where an output goes (a device array of the engine's own,
or nowhere), never what is computed, so every output the host still reads is bit-identical to
the twin's (parity.bits_equal, no tolerance).  The host arrays of the declared outputs are
filled with a sentinel bit pattern before the commit and must hold it, bit for bit, after the
run: the engine neither writes nor stages them.

fcx_output_info after the run says what became of a declared output: 1 kept in a device array,
2 the whole-phase plan left its store out (the array is then stale: fcx_device_ptr refuses it).
Sizes: 4096 + 128 + 3 cells (one layout tile, one more wave tile and an odd tail, so the
partial-vector path runs); 4099 / 4225 where u and v are grids of their own; fp32 4096 + 256 + 5.
RCO computes no QSUR (its method is 'none', so a declaration of it is the plan check's error):
its single-type case declares MEVA, which HLAT consumes in the launch."""
import ctypes

import numpy as np
import pytest

import namelists
import oracle_lib
from parity import assert_tight, bits_equal

pytestmark = pytest.mark.gpu

from fcx import _lib, driver, host_alloc  # noqa: E402
from fcx.basic import IDX, PHASE_ALL, PHASE_EARLY, PHASE_NORMAL  # noqa: E402
from fcx.engine import Engine, run_group  # noqa: E402
from fcx.parallel import BlockedRandomAtmosMap, LocalAtmos  # noqa: E402
from fcx.setup import setup_from_namelist  # noqa: E402
from fcx.synthetic import SyntheticCoupler, as_dtype, build_case, corrections  # noqa: E402

T_STEP = 3600 * 24 * 45
N = 4096 + 128 + 3
N32 = 4096 + 256 + 5
SEP = (4099, 4225)
E_STATE = 2
HOST, DEVICE, UNREAD = _lib.FCX_OUT_HOST, _lib.FCX_OUT_DEVICE, _lib.FCX_OUT_UNREAD
ATM_FIELDS = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))
ALL_SEVEN = {(1, 1, "QSUR"): UNREAD, (1, 1, "MEVA"): UNREAD, (1, 1, "HLAT"): UNREAD, (1, 1, "HSEN"): UNREAD,
             (1, 1, "RBBR"): UNREAD, (1, 2, "UMOM"): UNREAD, (1, 3, "VMOM"): UNREAD}


def sentinel(a):
    """the bit pattern a declared host array is filled with: quiet NaNs numbered by cell"""
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    base = 0x7FF8_5E17_0000_0000 if a.dtype == np.float64 else 0x7FC5_0000
    return (np.arange(a.shape[0], dtype=np.uint64) + np.uint64(base)).astype(u)


def fill_sentinels(case, use):
    arrays = {}
    for key in use:
        a = case.lf.field[key]
        a.view(sentinel(a).dtype)[:] = sentinel(a)
        arrays[id(a)] = a
    return arrays


def sentinels_intact(arrays, label):
    for a in arrays.values():
        assert np.array_equal(a.view(sentinel(a).dtype), sentinel(a)), f"{label}: a declared host array was written"


def snapshot(case, declared, extra=None):
    got = {k: np.array(case.lf.field[k], copy=True) for k in case.outputs if id(case.lf.field[k]) not in declared}
    for k, a in (extra or {}).items():
        got[k] = np.array(a, copy=True)
    return got


def same(got, twin, label):
    assert got.keys() <= twin.keys() and got, label
    for k in got:
        assert np.all(np.isfinite(got[k])), f"{label}: {k} not finite"
        bad = ~bits_equal(got[k], twin[k])
        assert not bad.any(), f"{label}: {k} differs from the twin in {int(bad.sum())} cells, first {int(np.argmax(bad))}"


def step_once(eng):
    eng.step(PHASE_ALL, T_STEP)


def read_device(eng, key, n, dtype=np.float64):
    """cells [0, n) of the device array behind a slot (fcx_device_ptr + fcx_memcpy), tiles undone"""
    tile, stride = eng.device_layout()
    tiles = (n + tile - 1) // tile
    raw = np.empty(tiles * stride, dtype=dtype)
    p = eng.device_ptr(*key)
    count = (tiles - 1) * stride + (n - (tiles - 1) * tile)
    _lib.check(eng.lib.fcx_memcpy(ctypes.c_void_p(raw.ctypes.data), ctypes.c_void_p(p), count * raw.itemsize, 2))
    return np.concatenate([raw[t * stride: t * stride + tile] for t in range(tiles)])[:n]


def pair(make, use, run=step_once, engine_kw=None, extra=None, check=None, label=""):
    """The declaring engine, then its twin, over two builds of the same case.  make() -> case;
    extra(case) -> (engine keywords, {key: further output array}); check(eng, case, twin_case=None)
    runs on the declaring engine after the run.  Returns ((got, case, facts), (twin, twin case, facts))
    with facts = the engine's algorithmic bytes, staging bytes, zero-copy bytes, span runs."""
    out = []
    for declare in (True, False):
        case = make()
        declared = fill_sentinels(case, use) if declare else {}
        kw, arrays = extra(case) if extra else ({}, {})
        kw = dict(kw, **(engine_kw or {}))
        eng = Engine(case.lf, case.num_surface_types, case.methods, corrections=case.corrections,
                     averages=case.averages, output_use=use if declare else None, **kw)
        try:
            run(eng)
            sentinels_intact(declared, label)
            facts = {"bytes": eng.algorithmic_bytes(PHASE_ALL), "staging": eng.staging_bytes(),
                     "zero_copy": eng.zero_copy_bytes(), "spans": eng.span_runs(PHASE_ALL)}
            if declare and check:
                check(eng, case)
            out.append((snapshot(case, declared, arrays), case, facts))
        finally:
            eng.close()
    same(out[0][0], out[1][0], label)
    return out[0], out[1]


def stale(eng, key):
    with pytest.raises(_lib.FcxError) as ex:
        eng.device_ptr(*key)
    assert ex.value.status == E_STATE and f"{key[2]}({key[0]}," in str(ex.value) and "stale" in str(ex.value), str(ex.value)


def atmos_of(case, n, s0, fields=ATM_FIELDS, dtype=np.float64, la=None):
    la = la or BlockedRandomAtmosMap().local(0, n, 0, 1, n, ranges=[(0, n)])
    outs = {name: np.full(max(la.n_atmos, 1), np.nan, dtype=dtype) for name, _ in fields}
    kw = {"atmos": {"local": la, "fields": [(PHASE_NORMAL, s0, g, name, outs[name]) for name, g in fields]}}
    return kw, {("atm", name): a for name, a in outs.items()}


def long_runs(n, run=7):
    """atmosphere cells of `run` exchange cells: heads of up to run - 1 > kRecHead cells cross the tiles"""
    idx = (np.arange(n) // run).astype(np.int32)
    area = 1.0 + 0.25 * np.cos(np.arange(n) * 0.37)
    w = area / np.bincount(idx, weights=area)[idx]
    return LocalAtmos(0, n, 0, int(idx[-1]) + 1, idx, w, -1, -1, 0)


# ---------------------------------------------------------------- 1: T = 1, one output unread
@pytest.mark.parametrize("variant,specialize,sep,key", [
    ("CCLM", 1, None, (1, 1, "QSUR")), ("MOM5", 1, None, (1, 1, "QSUR")), ("RCO", 1, None, (1, 1, "MEVA")),
    ("CCLM", 0, None, (1, 1, "QSUR")), ("MOM5", 0, SEP, (1, 1, "QSUR"))])
def test_t1_one_unread_output(variant, specialize, sep, key):
    def check(eng, case):
        assert eng.output_info(*key) == 2
        stale(eng, key)

    (_, _, f), (_, _, ft) = pair(lambda: build_case(variant, n=N, T=1, bias=True, sep_grids=sep), {key: UNREAD},
                                 engine_kw={"options": {"specialize": specialize}}, check=check,
                                 label=f"{variant} spec={specialize} sep={sep} {key}")
    assert ft["bytes"] - f["bytes"] == 8 * N  # one store of n cells less, nothing else


def test_t1_separate_grids_qsur_of_every_grid():
    """u and v grids of their own: QSUR(u) and QSUR(v) feed the grid's momentum in the launch
    (the uv_grid pass computes them though their pointers are null)."""
    use = {(1, 1, "QSUR"): UNREAD, (1, 2, "QSUR"): UNREAD, (1, 3, "QSUR"): UNREAD}

    def check(eng, case):
        for k in use:
            assert eng.output_info(*k) == 2, k
            stale(eng, k)

    for variant in ("CCLM", "MOM5"):
        (_, _, f), (_, _, ft) = pair(lambda: build_case(variant, n=N, T=1, bias=True, sep_grids=SEP), use,
                                     check=check, label=f"{variant} separate grids")
        assert ft["bytes"] - f["bytes"] == 8 * (N + SEP[0] + SEP[1])


# ---------------------------------------------------------------- 2: fused accumulation
@pytest.mark.parametrize("records", [0, 1])
@pytest.mark.parametrize("variant", ["CCLM", "MOM5", "RCO"])
def test_fused_accumulation_with_every_flux_unread(variant, records):
    """The halo launch on the random map (runs of 3-5 cells): the six atmosphere outputs are the
    twin's with all seven exchange-grid outputs declared unread; as plain arrays and as records."""
    use = {k: v for k, v in ALL_SEVEN.items() if not (variant == "RCO" and k[2] == "QSUR")}

    def check(eng, case):
        assert eng.atm_records() == bool(records)
        kinds = {k: eng.output_info(*k) for k in use}
        assert set(kinds.values()) <= {1, 2} and kinds[(1, 1, "MEVA")] == 2, kinds
        # the fp64 CCLM halo kernel takes no unstored path: its accumulated
        # fluxes keep a stored device array; MOM5 and RCO store none of the seven
        want = 1 if variant == "CCLM" else 2
        assert all(kinds[k] == want for k in use if k[2] not in ("QSUR", "MEVA")), kinds

    pair(lambda: build_case(variant, n=N, T=1, bias=True), use, extra=lambda c: atmos_of(c, N, 1),
         engine_kw={"options": {"atm_records": records, "zero_copy": 0}}, check=check,  # (tiled mirrors: records apply)
         label=f"{variant} fused records={records}")


def test_crossing_records_keep_the_accumulated_fields():
    """FCX_OPT_ATMOS_HALO = 0 on a map of 7-cell runs: the fix-up launch re-reads the stored fluxes
    for heads longer than kRecHead, so the accumulated fields stay device arrays (kind 1); QSUR,
    which nothing accumulates, is still not stored (kind 2)."""
    def check(eng, case):
        kinds = {k: eng.output_info(*k) for k in ALL_SEVEN}
        assert kinds.pop((1, 1, "QSUR")) == 2 and set(kinds.values()) == {1}, kinds

    for variant in ("CCLM", "MOM5"):
        pair(lambda: build_case(variant, n=N, T=1, bias=True), ALL_SEVEN,
             extra=lambda c: atmos_of(c, N, 1, la=long_runs(N)), engine_kw={"options": {"atmos_halo": 0}},
             check=check, label=f"{variant} crossing records")


# ---------------------------------------------------------------- 3: T = 2 / T = 3
@pytest.mark.parametrize("variant", ["MOM5", "CCLM"])
def test_t2_register_averages_with_the_per_type_fluxes_unread(variant):
    """The register-average kernels do not take the unstored path (the T = 2
    bench step was slower with it): HLAT, HSEN and RBBR, whose blocks would need a want bit, keep a
    stored device array (kind 1, off the host link all the same); MEVA, whose block computes
    whatever its pointer says, is not stored (kind 2)."""
    use = {(s, 1, name): UNREAD for s in (1, 2) for name in ("MEVA", "HLAT", "HSEN", "RBBR")}

    def check(eng, case):
        for k in use:
            assert eng.output_info(*k) == (2 if k[2] == "MEVA" else 1), (k, eng.output_info(*k))
        assert all(eng.output_info(0, 1, name) == 0 for name in ("MEVA", "HLAT", "HSEN", "RBBR"))

    (got, _, f), (_, case, ft) = pair(lambda: build_case(variant, n=N, T=2, bias=True), use,
                                      extra=lambda c: atmos_of(c, N, 0), check=check, label=f"{variant} T=2")
    assert ft["bytes"] - f["bytes"] == 8 * N * 2  # the two MEVA stores
    assert all((0, 1, name) in got for name in ("MEVA", "HLAT", "HSEN", "RBBR"))
    if variant == "MOM5":  # (the twin's case: its host arrays hold every output for the comparison)
        ref = oracle_lib.run_case(case, "c", current_step_time=T_STEP)
        mine = {k: np.array(case.lf.field[k], copy=True) for k in case.outputs}
        mine.update({k: got[k] for k in got if k in mine})
        assert_tight(case, mine, ref, T_STEP, "per-type fluxes unread, T=2", report=False)


def test_t3_without_register_averages_keeps_the_arrays():
    """Separate u and v grids at T = 3: the averages of UMOM and VMOM re-read x[s] from the arrays the
    launch stored, so those stay (kind 1); MEVA on the t grid goes through a register average and is
    not stored (kind 2)."""
    use = {(s, g, name): UNREAD for s in (1, 2, 3) for g, name in ((1, "MEVA"), (2, "UMOM"), (3, "VMOM"))}

    def make():
        case = build_case("MOM5", n=N, T=3, bias=True, sep_grids=SEP)
        for g, name in ((2, "UMOM"), (3, "VMOM")):  # FARE exists on u and v: the averages apply
            if (0, g, name) not in case.lf.field:
                case.lf.allocate_localvar(name, 0, g, value=np.nan)
                case.averages.append((PHASE_NORMAL, g, name))
                case.outputs.append((0, g, name))
        return case

    def check(eng, case):
        for k in use:
            assert eng.output_info(*k) == (2 if k[1] == 1 else 1), (k, eng.output_info(*k))

    pair(make, use, check=check, label="T=3 re-read averages")


# ---------------------------------------------------------------- 4: group launch
def test_group_of_three_with_declarations_on_two():
    torch = pytest.importorskip("torch")
    stream = torch.cuda.current_stream(torch.device("cuda", 0))  # one stream: the members merge
    n = 3 * 4096 + 128 + 3
    uses = {"CCLM": {(1, 1, "QSUR"): UNREAD}, "MOM5": dict(ALL_SEVEN), "RCO": {}}
    res = []
    for declare in (True, False):
        cases, engines, arrays, declared = [], [], {}, {}
        try:
            for v in ("CCLM", "MOM5", "RCO"):
                c = build_case(v, n=n, T=1, bias=True)
                if declare:
                    declared.update(fill_sentinels(c, uses[v]))
                kw, outs = atmos_of(c, n, 1)
                e = Engine(c.lf, 1, c.methods, corrections=c.corrections, stream=stream.cuda_stream,
                           output_use=uses[v] if declare else None,
                           options={"atmos_in_run": 0, "host_staging": 0, "atm_records": 1}, **kw)
                e.upload(PHASE_ALL)
                cases.append(c)
                engines.append(e)
                arrays.update({(v,) + k: a for k, a in outs.items()})
            run_group(engines, PHASE_ALL, T_STEP)
            assert [e.last_group_size() for e in engines] == [3, 3, 3]
            if declare:
                assert engines[0].output_info(1, 1, "QSUR") == 2
                assert {engines[1].output_info(*k) for k in ALL_SEVEN} == {2}
            for e in engines:
                e.download(PHASE_ALL)
                e.synchronize()
            torch.cuda.synchronize()
            sentinels_intact(declared, "group")
            got = {k: np.array(a, copy=True) for k, a in arrays.items()}
            for v, c in zip(("CCLM", "MOM5", "RCO"), cases):
                got.update({(v,) + k: np.array(c.lf.field[k], copy=True) for k in c.outputs
                            if id(c.lf.field[k]) not in declared})
            res.append(got)
        finally:
            for e in engines:
                e.close()
    same(res[0], res[1], "group of three")


# ---------------------------------------------------------------- 5: transports
KEPT = {(1, 1, "QSUR"): DEVICE, (1, 1, "HSEN"): DEVICE}


def kept_check(n, twin_values):
    def check(eng, case):
        for k in KEPT:
            assert eng.output_info(*k) == 1
            dev = read_device(eng, k, n)
            twin_values[k] = dev
    return check


def transport_pair(make, n, engine_kw=None, run=step_once, label=""):
    seen = {}
    (got, _, f), (twin, tcase, ft) = pair(make, KEPT, run=run, engine_kw=engine_kw, check=kept_check(n, seen), label=label)
    for k in KEPT:  # the device arrays hold what the twin downloaded
        assert bits_equal(seen[k], tcase.lf.field[k][:n]).all(), (label, k)
    return f, ft


def test_kept_outputs_of_caller_heap_arrays():
    """numpy arrays: the small grid's mapped staging arena, then (zero-copy off) mirrors behind
    the page-locked arena."""
    f, ft = transport_pair(lambda: build_case("MOM5", n=N, T=1, bias=True), N, label="heap, mapped arena")
    span = (8 * N + 255) // 256 * 256
    assert ft["staging"] - f["staging"] == 2 * span and ft["zero_copy"] - f["zero_copy"] == 2 * 8 * N
    # plain mirrors: one pool, the kept outputs behind the part the page-locked image covers
    f, ft = transport_pair(lambda: build_case("MOM5", n=N, T=1, bias=True), N,
                           engine_kw={"options": {"zero_copy": 0, "tiled_layout": 0}}, label="heap, plain mirrors")
    assert f["zero_copy"] == ft["zero_copy"] == 0 and f["staging"] > 0
    assert ft["staging"] - f["staging"] == 2 * span
    # tile-blocked mirrors: an image is whole tile rows of S slots (S = the larger of the read and
    # the written arrays' counts, here the read ones), so two written slots less leave it as it is
    f, ft = transport_pair(lambda: build_case("MOM5", n=N, T=1, bias=True), N,
                           engine_kw={"options": {"zero_copy": 0}}, label="heap, tiled mirrors")
    assert f["zero_copy"] == ft["zero_copy"] == 0 and 0 < f["staging"] == ft["staging"]


@pytest.mark.parametrize("options", [{}, {"zero_copy": 0}, {"zero_copy": 0, "lib_spans": 0}])
def test_kept_outputs_of_library_arrays(options):
    """fcx_host_malloc arrays in place (zero-copy auto), as spans, and as one copy per array.  The
    declared arrays are allocated last, each behind a spacer block, so that in the twin each is a
    download of its own."""
    with host_alloc.Arena() as arena:
        def make():
            case = build_case("MOM5", n=N, T=1, bias=True)
            held = {k: case.lf.field.pop(k) for k in list(case.lf.field) if k[2] in ("QSUR", "HSEN")}
            arena.adopt(case.lf)
            moved = {}
            for k, a in held.items():
                if id(a) not in moved:
                    arena.empty(64)  # spacer: not an array of the engine
                    moved[id(a)] = arena.empty(a.shape[0], a.dtype)
                    moved[id(a)][:] = a
                case.lf.field[k] = moved[id(a)]
            return case

        f, ft = transport_pair(make, N, engine_kw={"options": options}, label=f"library arrays {options}")
        assert f["staging"] == ft["staging"] == 0
        if not options:
            assert ft["zero_copy"] - f["zero_copy"] == 2 * 8 * N
        else:
            assert f["zero_copy"] == ft["zero_copy"] == 0
        if options == {"zero_copy": 0}:
            assert ft["spans"][1] - f["spans"][1] == 2 and f["spans"][0] == ft["spans"][0], (f, ft)


def test_kept_outputs_in_the_pipelined_step_and_the_async_step():
    n = 8 * 1024 + 515
    opts = {"pipeline_min_chunk": 1024, "pipeline_chunks": 8, "zero_copy": 0}
    transport_pair(lambda: build_case("MOM5", n=n, T=1, bias=True), n, engine_kw={"options": opts}, label="pipelined")

    def run_async(eng):
        eng.step_async(PHASE_ALL, T_STEP)
        eng.synchronize()

    transport_pair(lambda: build_case("CCLM", n=N, T=1, bias=True), N, run=run_async, label="step_async")


def test_unread_outputs_in_the_pipelined_step():
    """Chunk launches carry crossing records: the accumulated fluxes keep their arrays, QSUR is
    not stored in any chunk."""
    n = 8 * 1024 + 515
    opts = {"pipeline_min_chunk": 1024, "pipeline_chunks": 8, "zero_copy": 0}

    def check(eng, case):
        kinds = {k: eng.output_info(*k) for k in ALL_SEVEN}
        assert kinds.pop((1, 1, "QSUR")) == 2 and set(kinds.values()) == {1}, kinds

    pair(lambda: build_case("MOM5", n=n, T=1, bias=True), ALL_SEVEN, extra=lambda c: atmos_of(c, n, 1),
         engine_kw={"options": opts}, check=check, label="pipelined, unread")


# ---------------------------------------------------------------- 6: fp32
@pytest.mark.parametrize("variant", ["CCLM", "MOM5"])
def test_fp32_engine(variant):
    def check_q(eng, case):
        assert eng.output_info(1, 1, "QSUR") == 2
        stale(eng, (1, 1, "QSUR"))

    (_, _, f), (_, _, ft) = pair(lambda: as_dtype(build_case(variant, n=N32, T=1, bias=True), "float32"),
                                 {(1, 1, "QSUR"): UNREAD}, check=check_q, label=f"fp32 {variant} QSUR")
    assert ft["bytes"] - f["bytes"] == 4 * N32

    def check_all(eng, case):
        assert {eng.output_info(*k) for k in ALL_SEVEN} == {2}

    pair(lambda: as_dtype(build_case(variant, n=N32, T=1, bias=True), "float32"), ALL_SEVEN,
         extra=lambda c: atmos_of(c, N32, 1, dtype=np.float32), check=check_all, label=f"fp32 {variant} fused")


# ---------------------------------------------------------------- 7: the stale mix
def test_a_per_call_subroutine_refuses_a_stale_input_by_name():
    key = (1, 1, "QSUR")
    twin_case = build_case("CCLM", n=N, T=1, bias=True)
    twin = Engine(twin_case.lf, 1, twin_case.methods, corrections=twin_case.corrections)
    try:
        twin.step(PHASE_ALL, T_STEP)
        _lib.check(twin.lib.fcx_calc_spec_vapor_surface(twin.h, 1))
        _lib.check(twin.lib.fcx_calc_flux_mass_evap(twin.h, T_STEP))
        want = np.array(twin_case.lf.field[(1, 1, "MEVA")], copy=True)
    finally:
        twin.close()
    case = build_case("CCLM", n=N, T=1, bias=True)
    declared = fill_sentinels(case, {key: UNREAD})
    eng = Engine(case.lf, 1, case.methods, corrections=case.corrections, output_use={key: UNREAD})
    try:
        eng.step(PHASE_ALL, T_STEP)
        before = {k: np.array(case.lf.field[k], copy=True) for k in case.outputs if k != key}
        r = eng.lib.fcx_calc_flux_mass_evap(eng.h, T_STEP)
        msg = eng.lib.fcx_last_error().decode()
        assert r == E_STATE and "QSUR(1,t)" in msg and "stale" in msg, (r, msg)
        for k, a in before.items():  # nothing was launched or downloaded
            assert bits_equal(a, case.lf.field[k]).all(), k
        _lib.check(eng.lib.fcx_calc_spec_vapor_surface(eng.h, 1))  # a per-call plan always stores
        eng.device_ptr(*key)  # current again
        assert eng.output_info(*key) == 2  # still what the whole-phase plan does with it
        _lib.check(eng.lib.fcx_calc_flux_mass_evap(eng.h, T_STEP))
        assert bits_equal(case.lf.field[(1, 1, "MEVA")], want).all()
        sentinels_intact(declared, "stale mix")
    finally:
        eng.close()


def test_a_declaration_after_the_commit_is_a_state_error():
    case = build_case("CCLM", n=N, T=1, bias=True)
    eng = Engine(case.lf, 1, case.methods, corrections=case.corrections, output_use={(1, 1, "QSUR"): UNREAD})
    try:
        for use in (HOST, DEVICE, UNREAD):
            for key in ((1, 1, "QSUR"), (1, 1, "HSEN")):
                r = eng.lib.fcx_set_output_use(eng.h, key[0], key[1], IDX[key[2]], use)
                assert r == E_STATE and "committed" in eng.lib.fcx_last_error().decode(), (key, use, r)
        eng.step(PHASE_ALL, T_STEP)  # nothing changed: QSUR unread and not stored, HSEN downloaded
        assert eng.output_info(1, 1, "QSUR") == 2 and eng.output_info(1, 1, "HSEN") == 0
        assert np.all(np.isfinite(case.lf.field[(1, 1, "HSEN")]))
    finally:
        eng.close()


# ---------------------------------------------------------------- 8: early then normal phase
@pytest.mark.parametrize("variant,T", [("CCLM", 1), ("MOM5", 2)])
def test_early_then_normal_phase_with_stores_skipped(variant, T):
    """The coupling loop's two phases per time step on an engine without regriddings, where the
    stores really are left out: RBBR in the early phase, QSUR and MEVA in the normal one.  Every
    output still read equals the same loop's without declarations after each phase of each step."""
    use = {(s, 1, name): UNREAD for s in range(1, T + 1) for name in ("RBBR", "QSUR", "MEVA")}
    trace = []
    for declare in (True, False):
        case = build_case(variant, n=N, T=T, bias=True)
        declared = fill_sentinels(case, use) if declare else {}
        eng = Engine(case.lf, T, case.methods, corrections=case.corrections, averages=case.averages,
                     output_use=use if declare else None)
        seen = []
        try:
            for step in range(2):
                for phase in (PHASE_EARLY, PHASE_NORMAL):
                    case.lf.field[(1, 1, "TSUR")][:] += 0.125  # the host receives new inputs
                    eng.step(phase, T_STEP + 600 * step)
                    seen.append(snapshot(case, declared))
            sentinels_intact(declared, "two phases")
            if declare:
                for k in use:  # (T = 2: the register average consumes RBBR, and that family keeps the array)
                    kind = 1 if (T == 2 and k[2] == "RBBR") else 2
                    assert eng.output_info(*k) == kind, (k, eng.output_info(*k))
                    if kind == 2:
                        stale(eng, k)
        finally:
            eng.close()
        trace.append(seen)
    compared = 0
    for i, (got, twin) in enumerate(zip(*trace)):
        # (the first early phase: the normal phase's outputs are not computed yet, in either loop)
        got = {k: a for k, a in got.items() if np.all(np.isfinite(twin[k]))}
        if got:
            same(got, twin, f"{variant} T={T} phase run {i}")
        compared += len(got)
    assert compared >= 3 * len(trace[1][-1]) - 3 * len(use)


# ---------------------------------------------------------------- 8, 9: the set-ups through the driver
@pytest.mark.parametrize("zero_copy", [0, 2])
@pytest.mark.parametrize("which,mype,bias", [("MOM5_BALTIC", 0, True), ("CCLM_REGRID", 1, False)])
def test_set_up_with_selected_outputs_through_the_driver(which, mype, bias, zero_copy):
    """The early phase, then the normal phase, for every time step of the namelist: every put equals
    that of the same loop without the selection, and the arrays downloaded are fewer by exactly the
    unsent ones: with device mirrors and real device-to-host copies (zero-copy off), and with the
    arrays used in place through the mapped arena (auto at this size), where the bytes used in
    place shrink by the same arrays.  Both set-ups regrid, so every unread output is kept on the
    device (kind 1); a loop whose stores are really left out is
    test_early_then_normal_phase_with_stores_skipped."""
    grids = (301, 299, 311)
    runs = []
    for select in (True, False):
        s = setup_from_namelist(getattr(namelists, which), mype=mype, grid_size=grids)
        unsent = s.unsent_outputs()
        assert any(k[2] == "QSUR" for k in unsent)
        # every computed array starts as sentinels, in both loops: with mirrors (zero-copy off) only
        # a device-to-host copy writes a host array, so the arrays that changed are the downloads
        computed = {}
        for key in s.computed_slots():
            a = s.local_field.field[key]
            a.view(np.uint64)[:] = sentinel(a)
            computed[id(a)] = a
        declared = {id(s.local_field.field[k]): s.local_field.field[k] for k in unsent} if select else {}
        corr = (20000101, corrections(grids[0])) if bias else None
        eng = s.engine(corrections=corr, regrid=namelists.regrid_matrices(grids), select_outputs=select,
                       options={"zero_copy": zero_copy})
        try:
            coupler = SyntheticCoupler.for_setup(s)
            driver.run(s, eng, coupler)
            sentinels_intact(declared, which)
            if select:
                assert {eng.output_info(*k) for k in unsent} == {1}
            downloaded = sum(1 for a in computed.values() if not np.array_equal(a.view(np.uint64), sentinel(a)))
            runs.append((coupler.sent, eng.zero_copy_bytes(), downloaded,
                         len({id(s.local_field.field[k]) for k in unsent}),
                         sum(8 * s.local_field.field[k].shape[0] for k in {id(s.local_field.field[k]): k for k in unsent}.values())))
        finally:
            eng.close()
    (sent, in_place, d2h, n_unsent, unsent_bytes), (tsent, tin_place, td2h, _, _) = runs
    assert sent.keys() == tsent.keys() and sent
    for key in sent:
        assert np.all(np.isfinite(tsent[key])), key
        assert bits_equal(sent[key], tsent[key]).all(), key
    assert n_unsent >= 3 and td2h - d2h == n_unsent  # fewer downloaded arrays by exactly the unsent ones
    if zero_copy:
        assert unsent_bytes > 0 and tin_place - in_place == unsent_bytes
    else:
        assert in_place == tin_place == 0


