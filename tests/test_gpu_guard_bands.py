"""Guard-band gate: no write outside the outputs, no read outside the inputs, no input written.

Every array a case hands to the engine is carved out of ONE allocation with sentinel bands of
two layout tiles on each side (tests/guards.py), on device memory used in place, on the
caller's heap, and in library memory (spans and zero-copy).  Every case asserts
  (a) arena.check() == []: every band and every pure input bit-unchanged;
  (b) the outputs are the bits of the same case and options run from ordinary separate
      allocations (outputs pre-filled with NaN);
  (c) parity with the oracle (tests/parity.py; the fp32 engine against the fp64 oracle on the
      same fp32 inputs, its norm-wise gate), and accumulated / remapped values bit-identical
      to the sequential application on the engine's own fluxes.
Everything in (a) and (b) is bit-exact.  Shapes are the smallest that reach each edge: the
ragged tails of the 16-byte vector paths, one and several blocks, u/v grids shorter and longer
than the t grid, arrays longer than their grid (tail=37).

No deliberately overrunning kernel or library build is ever run on the GPU: that the harness
reports an overrun is shown on the CPU, by the planted faults of tests/test_guards.py.
"""
import dataclasses
import time

import numpy as np
import pytest

import oracle_lib
from guards import GuardedArena, distinct_arrays
from parity import FP32_NORM_GATE, assert_parity, error_report, write_report

pytestmark = pytest.mark.gpu

fcx = pytest.importorskip("fcx")
from fcx.basic import PHASE_ALL  # noqa: E402
from fcx.engine import Engine, run_group  # noqa: E402
from fcx.parallel import AtmosMap, local_atmos, synthetic_model_map  # noqa: E402
from fcx.synthetic import as_dtype, build_case, build_regrid_case  # noqa: E402

T_STEP = 3600 * 24 * 40
ATM_FIELDS = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))
RM_FIELDS = (("MEVA", 1), ("HSEN", 1), ("UMOM", 2), ("VMOM", 3))
STATS = {"cases": 0, "arrays": 0, "band_elements": 0, "violations": 0, "by_test": {}}
_REF, _PLAIN = {}, {}


@pytest.fixture(scope="module", autouse=True)
def summary():
    t0 = time.time()
    yield
    rec = {k: v for k, v in sorted(STATS.items()) if k != "_test"}
    write_report("guards_summary", {**rec, "module_wall_s": round(time.time() - t0, 2)})  # (beside the parity reports)


@pytest.fixture(autouse=True)
def _count(request):
    STATS["_test"] = request.node.originalname or request.node.name
    yield


def tally(arena, violations):
    STATS["cases"] += 1
    STATS["arrays"] += len(arena.regions)
    STATS["band_elements"] += arena.band_elements()
    STATS["violations"] += len(violations)
    STATS["by_test"][STATS["_test"]] = STATS["by_test"].get(STATS["_test"], 0) + 1


@dataclasses.dataclass
class Spec:
    """One case: how it is built and how the engine is driven."""
    name: str  # names the case (with dtype, options and mode) for the shared references
    build: object  # () -> fp64 host Case
    dtype: str = "float64"
    options: dict = dataclasses.field(default_factory=dict)
    mode: str = "step"  # step | step_async | per_call | run (run + run_atmos + synchronize)
    steps: int = 1
    amap: object = None  # AtmosMap: the atmosphere outputs hold exactly n_atmos elements
    shared: bool = False  # a boundary buffer of three slots, left = 0, right = 2
    mmap: object = None  # ModelMap of one remap
    atm_s: int = 1  # surface type of the accumulated / remapped fields (0: the averages)

    def case(self):
        c = self.build()
        return as_dtype(c, "float32") if self.dtype == "float32" else c

    def key(self, backend):
        return (self.name, self.dtype, backend, tuple(sorted(self.options.items())), self.mode, self.steps)


def plain(case, backend, lib_arena):
    """the case on ordinary separate allocations of the backend (aliases kept)"""
    if backend == "lib":
        lib_arena.adopt(case.lf)
    elif backend == "torch":
        import torch

        moved = {}
        for key, a, _ in distinct_arrays(case):
            moved[id(a)] = torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
        for key, a in list(case.lf.field.items()):
            case.lf.field[key] = moved[id(a)]
    return case


def drive(spec, case, eng):
    from test_gpu_zero_copy import _run_mode

    for k in range(spec.steps):
        t = T_STEP + 3600 * k
        if spec.mode == "run":
            eng.run(PHASE_ALL, t)
            eng.run_atmos(PHASE_ALL)
            eng.synchronize()
        else:
            _run_mode(case, eng, spec.mode, t)
    return t


def execute(spec, backend, arena_kw=None):
    """Run the spec on `backend`; arena_kw None: ordinary allocations.  Returns
    ({key: host array of the grid cells}, violations or None, last step time)."""
    from fcx import host_alloc

    case = spec.case()
    la = local_atmos(spec.amap, 0, 1) if spec.amap is not None else None
    if la is not None and spec.shared:
        la = dataclasses.replace(la, left=0, right=2, n_boundaries=3)
    extra = ([la.n_atmos] * len(ATM_FIELDS) if la is not None else []) + \
            ([spec.mmap.n_model] * len(RM_FIELDS) if spec.mmap is not None else []) + ([18] if spec.shared else [])
    lib_arena = host_alloc.Arena() if backend == "lib" and arena_kw is None else None
    arena = None
    if arena_kw is not None:
        arena = GuardedArena.for_case(case, backend, extra=extra, **arena_kw)
        new = lambda n, key: arena.empty(n, key, tail=0)  # noqa: E731
    else:
        plain(case, backend, lib_arena)

        def new(n, key):
            if backend == "torch":
                import torch

                return torch.full((n,), float("nan"), dtype=getattr(torch, spec.dtype), device="cuda:0")
            a = lib_arena.empty(n, spec.dtype) if backend == "lib" else np.empty(n, spec.dtype)
            a[:] = np.nan
            return a

    xo, atmos, remaps = {}, None, None
    if la is not None:
        for name, g in ATM_FIELDS:
            xo[("atm", name)] = new(la.n_atmos, ("atm", name))
        atmos = {"local": la, "fields": [(2, spec.atm_s, g, name, xo[("atm", name)]) for name, g in ATM_FIELDS]}
        if spec.shared:
            assert spec.dtype == "float64" and backend == "torch"
            buf = new(18, "shared")
            buf.fill_(0.0)
            if arena is not None:
                arena.protect("shared", 6, 12)
            xo["shared"] = buf
            atmos["shared"] = (buf, 6)
    if spec.mmap is not None:
        for name, g in RM_FIELDS:
            xo[("remap", name)] = new(spec.mmap.n_model, ("remap", name))
        remaps = [{"n_dst": spec.mmap.n_model, "src": spec.mmap.src, "dst": spec.mmap.dst, "w": spec.mmap.weight,
                   "fields": [(2, spec.atm_s, g, name, xo[("remap", name)]) for name, g in RM_FIELDS]}]
    if arena is not None:
        arena.snapshot()
    eng = Engine(case.lf, case.num_surface_types, case.methods, corrections=case.corrections,
                 averages=case.averages, regrid=case.regrid, atmos=atmos, remaps=remaps,
                 options=spec.options or None)
    try:
        t = drive(spec, case, eng)
    finally:
        eng.close()
    host = lambda a: a.detach().cpu().numpy() if backend == "torch" else np.array(a, copy=True)  # noqa: E731
    got = {k: host(case.lf.field[k])[:case.lf.grid_size[k[1] - 1]] for k in case.outputs}
    got.update({k: host(a) for k, a in xo.items()})
    violations = None
    if arena is not None:
        violations = arena.check()
        tally(arena, violations)
        arena.close()
    if lib_arena is not None:
        lib_arena.close()
    return got, violations, t


def reference(spec, t):
    """the oracle's outputs for the spec (fp32: on the fp32-rounded inputs widened exactly)"""
    k = (spec.name, spec.dtype, t)
    if k not in _REF:
        case = spec.build()
        if spec.dtype == "float32":
            case = as_dtype(as_dtype(case, "float32"), "float64")
        _REF[k] = oracle_lib.run_case(case, "c", current_step_time=t, regrid=bool(case.regrid))
    return _REF[k]


def oracle_gate(spec, flux, ref, t, label):
    """(c): fp64 -- assert_parity.  fp32 -- the suite's norm-wise gate on every field,
    max|x - ref| <= 1e-5 |ref|_inf against the fp64 oracle on the same fp32 inputs; a cell over
    it passes only inside the conditioning allowance of tests/test_gpu_fp32.py, 4 x the oracle's
    own movement under 16-ulp fp32 input perturbations.  (On the 1- and 3-cell grids used here
    the norm-wise error IS the element-wise relative error, which is ill-posed where HSEN's
    T_s - T_a EF or MEVA's q_s - q_a cancel, tests/parity.py; the allowance is that cell's
    conditioning, not a wider tolerance.)"""
    if spec.dtype == "float64":
        assert_parity(flux, ref, label=label)
        return
    over = {key: v[0] for key, v in error_report(flux, ref).items() if not v[0] <= FP32_NORM_GATE}
    if not over:
        return
    from test_gpu_fp32 import perturbation_movement

    k = (spec.name, "move", t)
    if k not in _REF:
        _REF[k] = perturbation_movement(as_dtype(as_dtype(spec.build(), "float32"), "float64"), t)
    bad = {}
    for key, norm in over.items():
        r = np.asarray(ref[key], dtype=np.float64)
        if not np.all(np.isfinite(flux[key]) == np.isfinite(r)):
            bad[key] = norm
            continue
        fin = np.isfinite(r)
        top = float(np.max(np.abs(r[fin]))) if fin.any() else 0.0
        allow = np.maximum(FP32_NORM_GATE * top, 4.0 * np.nan_to_num(_REF[k][key]))
        if np.any(np.abs(flux[key] - r)[fin] > allow[fin]):
            bad[key] = norm
    assert not bad, f"{label}: fp32 error over {FP32_NORM_GATE} norm-wise and over the cell's conditioning: {bad}"


def gate(spec, backend, label="", **arena_kw):
    """(a), (b) and (c) of the module docstring for one guarded run"""
    label = f"{spec.name} {spec.dtype} {backend} {spec.options} {spec.mode} {arena_kw} {label}"
    got, violations, t = execute(spec, backend, arena_kw)
    assert violations == [], label  # (a)
    k = spec.key(backend)
    if k not in _PLAIN:
        _PLAIN[k] = execute(spec, backend)[0]
    want = _PLAIN[k]
    assert got.keys() == want.keys()
    for key in got:  # (b)
        if key == "shared":  # (its middle slot: sentinels in the arena, checked by (a))
            assert np.array_equal(got[key][:6], want[key][:6]) and np.array_equal(got[key][12:], want[key][12:]), label
            continue
        assert np.array_equal(got[key], want[key], equal_nan=True), f"{label}: {key} differs from the plain run"
    ref = reference(spec, t)  # (c)
    flux = {key: np.asarray(got[key], dtype=np.float64) for key in ref}
    oracle_gate(spec, flux, ref, t, label)
    for (kind, name), a in ((key, a) for key, a in got.items() if isinstance(key[0], str) and key != "shared"):
        g = dict(ATM_FIELDS)[name]
        x = flux[(spec.atm_s, g, name)]
        if kind == "atm":
            seq = oracle_lib.atmos_accumulate(spec.amap.atmos_index, spec.amap.weight, x, spec.amap.n_atmos)
            inner = slice(1, -1) if spec.shared else slice(None)  # (the shared end cells wait for the finish)
            assert np.array_equal(a[inner], seq.astype(spec.dtype)[inner]), f"{label}: atmosphere {name}"
        else:
            seq = oracle_lib.remap_apply(spec.mmap.src, spec.mmap.dst, spec.mmap.weight, x, spec.mmap.n_model)
            assert np.array_equal(a, seq.astype(spec.dtype)), f"{label}: remap {name}"
    return got


def offsets(dtype):
    return (0, 8) if dtype == "float64" else (0, 4, 8, 12)


LAUNCH_OPTIONS = ({"cells_per_thread": 1}, {"specialize": 0}, {"nontemporal": 0}, {"max_blocks": 1})


# ------------------------------------------------------------------ device arrays in place
@pytest.mark.parametrize("variant", ["CCLM", "MOM5", "RCO"])
@pytest.mark.parametrize("dtype,n", [("float64", n) for n in (1, 2, 3, 127, 128, 129, 255, 257, 4097)] +
                         [("float32", n) for n in (1, 3, 5, 255, 257, 1023, 1025, 4099)])
def test_single_type_flux_kernels(variant, dtype, n):
    """T = 1, bias on: the specialised kernels' vector path and element-wise tail at every
    start offset; at the smallest and the largest odd size also one cell per thread, the
    generic kernel, plain loads and stores, and one block."""
    edge = n in ((3, 4097) if dtype == "float64" else (5, 4099))
    for options in ({},) + (LAUNCH_OPTIONS if edge else ()):
        spec = Spec(f"{variant}_n{n}", lambda: build_case(variant, n=n, T=1, bias=True), dtype, dict(options))
        for off in offsets(dtype):
            gate(spec, "torch", offset=off)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n", [1, 129, 777])
@pytest.mark.parametrize("variant,T", [("CCLM", 2), ("MOM5", 2), ("RCO", 2), ("CCLM", 3), ("RCO", 3), ("MOM5", 10)])
def test_multi_type_kernels(variant, T, n, dtype):
    """T = 2 (the register-average kernels), T = 3 with averages, T = 10"""
    spec = Spec(f"{variant}_T{T}_n{n}", lambda: build_case(variant, n=n, T=T, bias=True), dtype)
    for off in (0, 8):
        gate(spec, "torch", offset=off)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("variant", ["CCLM", "MOM5", "RCO"])
@pytest.mark.parametrize("grids", [(600, 550, 520), (513, 640, 700)])
def test_separate_grids_both_directions(grids, variant, dtype):
    """u/v grids shorter, then longer than the t grid: the band after the shorter arrays is
    the only witness of a pass bounded by the wrong grid"""
    nt, nu, nv = grids
    spec = Spec(f"{variant}_sep{grids}", lambda: build_case(variant, n=nt, T=2, bias=True, sep_grids=(nu, nv)), dtype)
    for off in (0, 8):
        gate(spec, "torch", offset=off)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("only", [(1, 1, "MEVA"), (1, 1, "HSEN"), (1, 2, "UMOM"), (0, 1, "PSUR"), (1, 1, "TSUR"),
                                  (0, 1, "VATM")])
def test_mixed_alignment(only, dtype):
    """exactly one output, then exactly one input, off the 16-byte boundary"""
    spec = Spec("CCLM_n4097", lambda: build_case("CCLM", n=4097, T=1, bias=True), dtype)
    for off in offsets(dtype)[1:]:
        gate(spec, "torch", offset=off, only=only)
    spec = Spec("MOM5_sep_mixed", lambda: build_case("MOM5", n=600, T=2, bias=True, sep_grids=(550, 520)), dtype)
    gate(spec, "torch", offset=offsets(dtype)[1], only=only)


def run_map(n, lengths):
    from test_gpu_multirank import random_run_map

    return random_run_map(n, lengths, seed=lengths[1] + 3)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("variant", ["CCLM", "MOM5", "RCO"])
@pytest.mark.parametrize("lengths", [(1, 5), (1, 10), (40, 64), (0, 5), (1, 400)])
@pytest.mark.parametrize("n", [1025, 4099])
def test_fused_accumulation(n, lengths, variant, dtype):
    """The fused accumulation of one engine into atmosphere outputs of exactly n_atmos
    elements from the arena: halo tiles, crossing records and their fix-up, the accumulation
    kernel for long segments, a grid cap; two steps, the second reuses the crossing records."""
    amap = run_map(n, lengths)
    for options in ({}, {"atmos_halo": 0}, {"max_blocks": 4}):
        spec = Spec(f"{variant}_n{n}_runs{lengths}", lambda: build_case(variant, n=n, T=1, bias=True), dtype,
                    dict(options), steps=2, amap=amap)
        gate(spec, "torch", offset=0)
    gate(spec, "torch", offset=8)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_fused_accumulation_one_atmosphere_cell(dtype):
    n = 1025
    w = np.random.default_rng(3).uniform(0.5, 1.5, n)
    amap = AtmosMap(np.zeros(n, np.int32), np.ascontiguousarray(w / w.sum()), 1)
    for options in ({}, {"atmos_halo": 0}):
        spec = Spec("CCLM_one_atmos_cell", lambda: build_case("CCLM", n=n, T=1, bias=True), dtype, dict(options),
                    steps=2, amap=amap)
        gate(spec, "torch", offset=0)


@pytest.mark.parametrize("lengths", [(1, 5), (1, 10)])
def test_fused_accumulation_shared_boundary_buffer(lengths):
    """a guarded boundary buffer of three slots, this engine's cells shared on the left (slot
    0) and on the right (slot 2): the middle slot stays bit-unchanged"""
    n = 1025
    spec = Spec(f"MOM5_shared_runs{lengths}", lambda: build_case("MOM5", n=n, T=1, bias=True), "float64", {},
                steps=2, amap=run_map(n, lengths), shared=True)
    got = gate(spec, "torch", offset=0)
    assert np.isfinite(got["shared"][:6]).all() and np.isfinite(got["shared"][12:]).all()


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_group_launch(dtype):
    """fcx_run_group over CCLM, MOM5 and RCO engines whose arrays are interleaved in one arena,
    the accumulation fused into the one launch"""
    import torch

    n, t = 1025, T_STEP
    amap = run_map(n, (1, 5))
    la = local_atmos(amap, 0, 1)
    variants = ("CCLM", "MOM5", "RCO")

    def run(guarded):
        cases = [build_case(v, n=n, T=1, bias=True) for v in variants]
        if dtype == "float32":
            cases = [as_dtype(c, "float32") for c in cases]
        arena = None
        if guarded:
            arena = GuardedArena.for_cases(cases, "torch", extra=[la.n_atmos] * len(ATM_FIELDS) * len(cases))
        else:
            for c in cases:
                plain(c, "torch", None)
        engines, outs = [], []
        stream = torch.cuda.current_stream().cuda_stream
        for i, c in enumerate(cases):
            if guarded:
                o = {name: arena.empty(la.n_atmos, (i, "atm", name), tail=0) for name, _ in ATM_FIELDS}
            else:
                o = {name: torch.full((la.n_atmos,), float("nan"), dtype=getattr(torch, dtype), device="cuda:0")
                     for name, _ in ATM_FIELDS}
            outs.append(o)
        if guarded:
            arena.snapshot()
        for c, o in zip(cases, outs):
            engines.append(Engine(c.lf, 1, c.methods, corrections=c.corrections, stream=stream,
                                  atmos={"local": la, "fields": [(2, 1, g, name, o[name]) for name, g in ATM_FIELDS]},
                                  options={"atmos_in_run": 0, "timing": 0, "host_staging": 0}))
        members = 0
        try:
            for k in range(2):
                run_group(engines, PHASE_ALL, t + 3600 * k)
                for e in engines:
                    e.run_atmos(PHASE_ALL)
            torch.cuda.synchronize()
            members = engines[0].last_group_size()
        finally:
            for e in engines:
                e.close()
        got = {}
        for i, (c, o) in enumerate(zip(cases, outs)):
            got.update({(i,) + k: c.lf.field[k].cpu().numpy() for k in c.outputs})
            got.update({(i, "atm", name): o[name].cpu().numpy() for name in o})
        violations = None
        if guarded:
            violations = arena.check()
            tally(arena, violations)
        return got, violations, members

    got, violations, members = run(True)
    assert violations == []
    assert members == 3
    want, _, _ = run(False)
    for key in want:
        assert np.array_equal(got[key], want[key], equal_nan=True), key
    for i, v in enumerate(variants):
        spec = Spec(f"{v}_n{n}", lambda: build_case(v, n=n, T=1, bias=True), dtype)
        ref = reference(spec, t + 3600)
        flux = {k: np.asarray(got[(i,) + k], dtype=np.float64) for k in ref}
        oracle_gate(spec, flux, ref, t + 3600, f"group {v} {dtype}")
        for name, g in ATM_FIELDS:
            seq = oracle_lib.atmos_accumulate(amap.atmos_index, amap.weight, flux[(1, g, name)], amap.n_atmos)
            assert np.array_equal(got[(i, "atm", name)], seq.astype(dtype)), (v, name)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_regridding(dtype):
    """all four regridding matrices, some destination rows without links"""
    probe = build_regrid_case(n=300, sep_grids=(310, 290))
    sizes = {0: 300, 1: 300, 2: 310, 3: 290}
    assert any((np.bincount(dst - 1, minlength=sizes[w]) == 0).any()
               for w, (src, dst, wt) in probe.regrid["matrices"].items())
    spec = Spec("regrid", lambda: build_regrid_case(n=300, sep_grids=(310, 290)), dtype)
    for off in (0, 8):
        gate(spec, "torch", offset=off)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n_dst", [1, 255, 1700])
@pytest.mark.parametrize("pack", [0, 1, 2])
def test_unfused_accumulation_and_remaps(pack, n_dst, dtype):
    """FCX_OPT_ATMOS_IN_RUN 0: the accumulation as its own kernel after the run; a remap that
    gathers from the arrays, from a packing pass, or from the flux launch's records.  With
    pack 0 also the generic flux kernel, which leaves the accumulation to atmos_kernel."""
    n = 4099
    mmap = synthetic_model_map(n, n_dst, links_per_cell=1 if n_dst == 1 else 2)
    for options in [{"atmos_in_run": 0, "remap_pack": pack}] + ([{"atmos_in_run": 0, "remap_pack": 0, "specialize": 0}]
                                                                if pack == 0 else []):
        spec = Spec(f"CCLM_n{n}_remap{n_dst}", lambda: build_case("CCLM", n=n, T=1, bias=True), dtype, options,
                    mode="run", amap=run_map(n, (1, 5)), mmap=mmap)
        gate(spec, "torch", offset=0)


# ------------------------------------------------------------------ host arrays
N_HOST = 4 * 1024 + 3
PIPE = {"pipeline_chunks": 4, "pipeline_min_chunk": 1024, "zero_copy": 0}
HEAP_MODES = {
    "default": ({}, "step"), "no_staging": ({"host_staging": 0}, "step"), "pipeline": (PIPE, "step"),
    "pipeline_no_staging": ({**PIPE, "host_staging": 0}, "step"), "deferred_scatter": ({"deferred_scatter": 1}, "step"),
    "pipeline_deferred_scatter": ({**PIPE, "deferred_scatter": 1}, "step"), "step_async": ({}, "step_async"),
    "pipeline_step_async": (PIPE, "step_async"), "per_call": ({}, "per_call")}


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("mode", list(HEAP_MODES))
def test_caller_heap_arrays(mode, dtype):
    """numpy arrays: the staging arena, direct copies, the chunk pipeline with a ragged last
    chunk, the deferred scatter, fcx_step_async + fcx_synchronize, the per-call sequence"""
    options, how = HEAP_MODES[mode]
    for variant, T in (("CCLM", 1), ("MOM5", 2)):
        spec = Spec(f"{variant}_T{T}_n{N_HOST}", lambda: build_case(variant, n=N_HOST, T=T, bias=True), dtype,
                    dict(options), mode=how, steps=2)
        for off in (0, 8):
            gate(spec, "numpy", offset=off)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("mode", ["default", "no_staging", "pipeline", "step_async"])
def test_caller_heap_atmosphere_and_remap_outputs(mode, dtype):
    """host atmosphere and remap outputs of exactly n_atmos / n_dst elements, guarded too"""
    options, how = HEAP_MODES[mode]
    spec = Spec(f"CCLM_n{N_HOST}_atm_remap", lambda: build_case("CCLM", n=N_HOST, T=1, bias=True), dtype,
                dict(options), mode=how, steps=2, amap=run_map(N_HOST, (1, 10)),
                mmap=synthetic_model_map(N_HOST, 255, links_per_cell=2))
    gate(spec, "numpy", offset=0)
    gate(spec, "numpy", offset=8)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("zero_copy", [1, 0])
@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("n", [1, 1001])
def test_library_memory(n, T, zero_copy, dtype):
    """fcx_host_malloc memory with bands on both sides of inputs as well as outputs: used in
    place (zero-copy) and through the span transport"""
    for mode in ("step", "step_async", "per_call"):
        spec = Spec(f"MOM5_T{T}_n{n}", lambda: build_case("MOM5", n=n, T=T, bias=True), dtype,
                    {"zero_copy": zero_copy}, mode=mode, steps=2)
        gate(spec, "lib", offset=0)
    gate(spec, "lib", offset=8)


# ------------------------------------------------------------------ arrays longer than their grid
TAIL_BACKENDS = {"device": ("torch", {}), "heap_staging": ("numpy", {}), "heap_direct": ("numpy", {"host_staging": 0}),
                 "heap_pipeline": ("numpy", PIPE), "spans": ("lib", {"zero_copy": 0}), "zero_copy": ("lib", {"zero_copy": 1})}


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("how", list(TAIL_BACKENDS))
def test_arrays_longer_than_their_grid(how, dtype):
    """fcx_bind_field takes ptr(1:n) with n >= grid_size: cells [grid_size, n) of inputs and
    outputs are never read or written (tail=37: the tail holds sentinels)"""
    backend, options = TAIL_BACKENDS[how]
    for name, build in (("MOM5_T1_n4099", lambda: build_case("MOM5", n=N_HOST, T=1, bias=True)),
                        ("CCLM_sep_T2", lambda: build_case("CCLM", n=600, T=2, bias=True, sep_grids=(550, 520)))):
        for mode in ("step", "step_async") if backend != "torch" else ("step",):
            spec = Spec(name, build, dtype, dict(options), mode=mode, steps=2)
            gate(spec, backend, offset=0, tail=37)
    gate(spec, backend, offset=8, tail=37)
