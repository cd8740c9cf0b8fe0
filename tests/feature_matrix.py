"""The opt-in engine features in combination: a seeded covering array of cases (pure Python), and
the one place that turns a case into engines (used by tests/test_feature_matrix.py on the host
and by tests/test_gpu_feature_matrix.py on the device, so both look at the same engines).

Every feature below promises (README, include/fcx.h) results that are bit for bit those of a plain
engine, and each has a test file of its own that switches on that feature alone.  Here they meet.

THE AXES (AXES below; a case is one level of each)
  prec       f64 | f64cr (FCX_OPT_CR_MATH) | f32 | f32wide (FCX_OPT_F32_MATH)
  types      T1 | T2 (water + ice with the type-0 averages: on merged grids the register-average
             kernels)
  variant    CCLM | MOM5 | RCO (a group case runs all three; the level names its first member)
  grids      shared (the u and v grids ARE the t grid) | sep (grids of their own, other sizes)
  consts     none | atm (two or three type-0 atmosphere inputs the variant reads, values of
             test_gpu_constant_fields.TYPICAL, UATM / VATM also 0.0) | ice (FICE of the last surface
             type: 1.0 at T = 2, the Baltic ice type; 1.0 or 0.0 at T = 1)
  outuse     none | qsur (QSUR(1,t) unread) | unread (T = 1: all seven exchange-grid outputs; T = 2:
             MEVA / HLAT / HSEN / RBBR of both types, of which the host reads the average) |
             device (the same slots kept on the device)
  received   none | unit (every atmosphere input that is no constant, through tests/received.py's
             `unit` map) | general (`general`: two weighted links per cell) | ocean (unit, plus
             TSUR / FICE of every type through a second map)
  consumers  none | accum (fused accumulation on random_run_map runs of 1-10 cells: segments cross
             the wave tiles, crossing records) | accum_halo (runs of 1-9: halo tiles, the launch
             in which an unread accumulated flux really loses its store) | accum_remap (accum + a
             two-link remap of two fields: packed records) | regrid (build_regrid_case)
  launch     run (fcx_step) | group (upload, fcx_run_group of the three variants, download)
  guard      off | on (FCX_OPT_CHECK_FINITE = 3: inputs and outputs)
  transport  default | pipeline (zero_copy 0, 4 chunks of >= 1024 cells) | libmem (fcx_host_malloc)

THE CASE LIST is a covering array: a seeded greedy construction (AETG-style) adds cases until
every pair of levels of two different axes is in some case, except the pairs of EXCLUSIONS.  The
committed seed is 0; FCX_MATRIX_SEED selects another for a longer search.  An excluded pair is one
the engine refuses; tests/test_feature_matrix.py holds every row to the engine's own message.

GRID SIZES.  fp64 4096 + 128 + 3, fp32 4096 + 256 + 5 (one layout tile, one more wave tile, an odd
tail); u / v grids of their own 4099 / 4225.  Every fourth case runs n = 129 or n = 300 (one tile,
partial vectors), with u / v grids of 131 / 127 and 310 / 290.

CORRECTLY ROUNDED CASES (f64cr).  Their TSUR / FICE / PSUR / PATM are rows of tests/golden/cr_math.npz
so that cr_expect.expected knows every site's value.  A row pairs TSUR with FICE and PSUR with
PATM, and the table has no two rows with the same TSUR, PSUR or PATM: those three are taken out of
the f64cr cases' constant set.  FICE = 0.0 (2,636 rows) and 1.0 (845 rows) stay: the cells' TSUR is
then drawn from those rows.  Received fields keep the pairing where the map is an injection of
weight 1.0 (`unit`: the model-grid sources are rows, TSUR and FICE, PSUR and PATM with the same
row per model cell); through the `general` map PSUR and PATM stay ordinary arrays (a weighted mix
of two rows is no row).
"""
import collections
import itertools
import os
import random

SEED = int(os.environ.get("FCX_MATRIX_SEED", "0"))

AXES = collections.OrderedDict([
    ("prec", ("f64", "f64cr", "f32", "f32wide")),
    ("types", ("T1", "T2")),
    ("variant", ("CCLM", "MOM5", "RCO")),
    ("grids", ("shared", "sep")),
    ("consts", ("none", "atm", "ice")),
    ("outuse", ("none", "qsur", "unread", "device")),
    ("received", ("none", "unit", "general", "ocean")),
    ("consumers", ("none", "accum", "accum_halo", "accum_remap", "regrid")),
    ("launch", ("run", "group")),
    ("guard", ("off", "on")),
    ("transport", ("default", "pipeline", "libmem")),
])

E_STATE = 2
# Pairs the engine does not support: (axis, level), (axis, level), why, and what Engine(...,
# commit=False).plan_check() (or the constructor) answers: the status and a piece of the message.
EXCLUSIONS = (
    {"pair": (("variant", "RCO"), ("outuse", "qsur")),
     "reason": "the RCO method set computes no QSUR (which_spec_vapor_surface_* 'none'): a declaration of an "
               "output no plan writes is the plan check's error (include/fcx.h, fcx_set_output_use)",
     "status": E_STATE, "text": "QSUR(1,t)"},
    {"pair": (("grids", "shared"), ("consumers", "regrid")),
     "reason": "a regridding reads one array and writes another; on u / v grids that ARE the t grid the destination "
               "slot is the source's own array (include/fcx.h, fcx_set_put_to)",
     "status": E_STATE, "text": "the destination is the source's own array"},
)

Case = collections.namedtuple("Case", ("index",) + tuple(AXES))


def all_pairs():
    """every pair of levels of two different axes, as ((axis, level), (axis, level)) in axis order"""
    out = []
    for (a, la), (b, lb) in itertools.combinations(AXES.items(), 2):
        out += [((a, x), (b, y)) for x in la for y in lb]
    return out


def excluded_pairs():
    return {tuple(sorted(row["pair"], key=lambda p: list(AXES).index(p[0]))) for row in EXCLUSIONS}


def pairs_of(levels):
    """the pairs one case covers; levels: {axis: level}"""
    items = [(a, levels[a]) for a in AXES]
    return set(itertools.combinations(items, 2))


def required_pairs():
    return set(all_pairs()) - excluded_pairs()


def build_cases(seed=SEED, candidates=30):
    """The greedy covering array: until no required pair is left, draw `candidates` cases -- each
    begins with a pair still uncovered and takes, axis by axis in a shuffled order, the level that
    covers the most uncovered pairs with the levels chosen so far (ties by the seeded generator) --
    and keep the one that covers the most."""
    rng = random.Random(20241021 + seed)
    excluded = excluded_pairs()
    left = required_pairs()
    axes = list(AXES)

    def allowed(levels, axis, level):
        for a, l in levels.items():
            p = tuple(sorted(((a, l), (axis, level)), key=lambda q: axes.index(q[0])))
            if p in excluded:
                return False
        return True

    def gain(levels, axis, level):
        g = 0
        for a, l in levels.items():
            p = tuple(sorted(((a, l), (axis, level)), key=lambda q: axes.index(q[0])))
            g += p in left
        return g

    cases = []
    while left:
        best, best_gain = None, -1
        for _ in range(candidates):
            (a, la), (b, lb) = rng.choice(sorted(left))
            levels = {a: la, b: lb}
            rest = [x for x in axes if x not in levels]
            rng.shuffle(rest)
            for axis in rest:
                options = [l for l in AXES[axis] if allowed(levels, axis, l)]
                top = max(gain(levels, axis, l) for l in options)
                levels[axis] = rng.choice([l for l in options if gain(levels, axis, l) == top])
            g = len(pairs_of(levels) & left)
            if g > best_gain:
                best, best_gain = levels, g
        cases.append(Case(len(cases), *(best[a] for a in AXES)))
        left -= pairs_of(best)
    for levels in WITNESSES:
        cases.append(Case(len(cases), *levels))
    return cases


# Cases the pairwise construction does not promise, appended to it (in AXES order).  One per
# precision in which an accumulated flux declared unread really loses its store -- one surface type,
# merged grids, halo tiles, whole-grid launches -- so that the accumulated value is the only witness
# of the dropped store's register path (the fp64 CCLM halo kernel keeps its accumulated fluxes: MOM5
# and RCO there); and the specialised CCLM kernel of fcx_kernels_cr.hip with wave-uniform constants.
WITNESSES = (
    ("f64", "T1", "MOM5", "shared", "atm", "unread", "unit", "accum_halo", "run", "on", "default"),
    ("f64cr", "T1", "RCO", "shared", "ice", "unread", "ocean", "accum_halo", "group", "off", "default"),
    ("f32", "T1", "CCLM", "shared", "atm", "unread", "general", "accum_halo", "run", "off", "libmem"),
    ("f32wide", "T1", "MOM5", "shared", "ice", "unread", "unit", "accum_halo", "run", "on", "default"),
    ("f64cr", "T1", "CCLM", "shared", "atm", "none", "none", "none", "run", "off", "default"),
)

CASES = build_cases()



def case_id(c):
    return "-".join([f"{c.index:02d}"] + [getattr(c, a) for a in AXES])


def describe(c):
    """the levels of a case for an assertion message"""
    return "case " + " ".join(f"{a}={getattr(c, a)}" for a in ("index",) + tuple(AXES))


def case_with(pair, index=0):
    """the plain case (first level of every axis) with the two levels of `pair` set"""
    levels = {a: AXES[a][0] for a in AXES}
    for a, l in pair:
        levels[a] = l
    return Case(index, *(levels[a] for a in AXES))


# ---------------------------------------------------------------------------------------------
# sizes
# ---------------------------------------------------------------------------------------------
N64, N32 = 4096 + 128 + 3, 4096 + 256 + 5
SEP = (4099, 4225)
SMALL = ((129, (131, 127)), (300, (310, 290)))


def sizes(c):
    """(n, (n_u, n_v) or None) of a case"""
    if c.index % 4 == 3:
        n, sep = SMALL[(c.index // 4) % 2]
    else:
        n, sep = (N32 if c.prec.startswith("f32") else N64), SEP
    return n, (sep if c.grids == "sep" else None)


def members(c):
    """the variants of the case's engines: one, or the three of a group (the case's first)"""
    if c.launch == "run":
        return (c.variant,)
    return (c.variant,) + tuple(v for v in AXES["variant"] if v != c.variant)


# ---------------------------------------------------------------------------------------------
# from a case to engines (needs numpy and the package; imported on first use)
# ---------------------------------------------------------------------------------------------
STEP_T = 3600 * 24 * 31          # February 1961 (the step time the perturbation allowance runs at)
STEP_GAP = 3600 * 24 * 45        # T_STEP of test_gpu_constant_fields.py: the second step is in March
STEPS = (STEP_T, STEP_T + STEP_GAP)
CR_LOOSE = ("TSUR", "PSUR", "PATM")  # no two fixture rows share a value: never constant at f64cr
FLUXES_T1 = (("QSUR", 1), ("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))
FLUXES_T2 = ("MEVA", "HLAT", "HSEN", "RBBR")
ATM_FIELDS = (("MEVA", 1), ("HLAT", 1), ("HSEN", 1), ("RBBR", 1), ("UMOM", 2), ("VMOM", 3))
REMAP_FIELDS = ("MEVA", "HSEN")
_FX = []


def fixture():
    import cr_expect

    if not _FX:
        root = os.path.dirname(os.path.abspath(__file__))
        _FX.append(cr_expect.Fixture(os.path.join(root, "golden", "cr_math.npz")))
    return _FX[0]


def is_cr(c):
    return c.prec == "f64cr"


def dtype_of(c):
    return "float32" if c.prec.startswith("f32") else "float64"


def engine_options(c):
    opts = {}
    if c.prec == "f64cr":
        opts["cr_math"] = 1
    if c.prec == "f32wide":
        opts["f32_math"] = 1
    return opts


def constants_of(c, variant):
    """{(surface type, name): value}, seeded by the case: the `atm` level draws among the
    atmosphere inputs the variant reads (f64cr: without PSUR and PATM)"""
    from test_gpu_constant_fields import ATMOS, READS, TYPICAL, ZERO

    rng = random.Random(1000 * c.index + sum(map(ord, variant)))
    T = 2 if c.types == "T2" else 1
    if c.consts == "atm":
        pool = [v for v in READS[variant] if v in ATMOS and not (is_cr(c) and v in CR_LOOSE)]
        names = rng.sample(pool, min(len(pool), rng.choice((2, 3))))
        return {(0, v): (0.0 if v in ZERO and rng.random() < 0.5 else TYPICAL[v]) for v in sorted(names)}
    if c.consts == "ice":
        return {(T, "FICE"): 1.0 if T == 2 else rng.choice((1.0, 0.0))}
    return {}


def output_use_of(c, variant, featured=True):
    """{(s, g, name): use} of the case's declared outputs (none for the twin)"""
    from fcx import _lib

    if not featured or c.outuse == "none":
        return {}
    if c.outuse == "qsur":
        return {} if variant == "RCO" and c.launch == "group" else {(1, 1, "QSUR"): _lib.FCX_OUT_UNREAD}
    use = _lib.FCX_OUT_UNREAD if c.outuse == "unread" else _lib.FCX_OUT_DEVICE
    if c.types == "T1":
        return {(1, g, name): use for name, g in FLUXES_T1 if not (variant == "RCO" and name == "QSUR")}
    return {(s, 1, name): use for s in (1, 2) for name in FLUXES_T2}


class Member:
    """One engine of a case, or its twin: the deterministic synthetic case with the constants
    filled in and the received fields expanded on the host (both engines' arrays start alike), and
    the keywords of fcx.engine.Engine.  arena: the fcx.host_alloc.Arena of a libmem case."""

    def __init__(self, c, variant, featured, arena=None):
        import numpy as np

        import received
        from fcx.basic import PHASE_EARLY, PHASE_NORMAL
        from fcx.parallel import local_atmos, synthetic_model_map
        from fcx.synthetic import as_dtype, build_case, build_regrid_case
        from test_gpu_constant_fields import declare
        from test_gpu_multirank import random_run_map

        self.c, self.variant, self.featured = c, variant, featured
        self.T = T = 2 if c.types == "T2" else 1
        n, sep = sizes(c)
        self.n = n
        seed = 20231015 + c.index
        if c.consumers == "regrid" and sep:
            case = build_regrid_case(variant, n=n, sep_grids=sep, T=T, bias=True, seed=seed)
        elif c.consumers == "regrid":  # (an excluded pair: the same put_to table on grids that are one grid)
            from fcx.synthetic import regrid_links

            case = build_case(variant, n=n, T=T, bias=True, seed=seed)
            case.regrid = {"matrices": {k: regrid_links(n, n, seed + 1 + k) for k in range(4)}}
            for s in range(1, T + 1):
                if variant != "RCO":
                    case.lf.put_to[(s, 1, "QSUR")] = 2 | 4
                case.lf.put_to[(s, 2, "UMOM")] = 1
                case.lf.put_to[(s, 3, "VMOM")] = 1
        else:
            case = build_case(variant, n=n, T=T, bias=True, sep_grids=sep, seed=seed)
        self.consts = constants_of(c, variant)
        if is_cr(c):
            self._fill_rows(case)
        if c.prec.startswith("f32"):
            case = as_dtype(case, "float32")
        self.case = case
        self.dtype = np.dtype(dtype_of(c))
        declare(case, self.consts)
        if featured and c.transport == "libmem" and arena is not None:
            arena.adopt(case.lf)
        self.arena = arena if (featured and c.transport == "libmem") else None
        # ---- received fields (declared in both; only the featured engine binds the maps)
        self.decl = None
        if c.received != "none":
            gs = case.lf.grid_size
            kind = "general" if c.received == "general" else "unit"
            atm = tuple(v for v in received.ATMOS if (0, v) not in self.consts
                        and not (is_cr(c) and kind == "general" and v in CR_LOOSE))
            atm_map = {g: received.links(kind, gs[g - 1], seed=1 + c.index) for g in (1, 2, 3)}
            oce = received.links("unit", gs[0], seed=7 + c.index) if c.received == "ocean" else None
            alloc = (lambda m, dt: self.arena.empty(m, dt)) if self.arena is not None else None
            self.decl = received.standard(case, atm_map, oce, atmos=atm, alloc=alloc)
            if self.consts:  # a constant and a received field are never one buffer
                for key in list(self.decl.fields):
                    if any(case.lf.field[key] is case.lf.field.get((s, g, v)) for (s, v) in self.consts for g in (1, 2, 3)):
                        del self.decl.fields[key], self.decl.sources[key]
            self.set_sources(0)
        # ---- keywords
        kw = {"corrections": case.corrections, "averages": case.averages, "regrid": case.regrid}
        opts = engine_options(c)
        self.outs = {}  # ("atm" | "remap", name) -> array
        self.amap = self.la = self.mmap = None
        s0 = 1 if T == 1 else 0
        self.s0 = s0
        if c.consumers in ("accum", "accum_halo", "accum_remap"):
            self.amap = random_run_map(n, (1, 9) if c.consumers == "accum_halo" else (1, 10), seed=4000 + c.index)
            self.la = local_atmos(self.amap, 0, 1)
            self.atm_fields = tuple((name, g) for name, g in ATM_FIELDS if g == 1 or sep is None)
            for name, _ in self.atm_fields:
                self.outs[("atm", name)] = np.full(max(self.la.n_atmos, 1), np.nan, dtype=self.dtype)
            kw["atmos"] = {"local": self.la, "fields": [((PHASE_EARLY if name == "RBBR" else PHASE_NORMAL), s0, g, name,
                                                         self.outs[("atm", name)]) for name, g in self.atm_fields]}
        if c.consumers == "accum_remap":
            self.mmap = synthetic_model_map(n, max(n // 8, 2), links_per_cell=2, seed=8000 + c.index)
            for name in REMAP_FIELDS:
                self.outs[("remap", name)] = np.full(self.mmap.n_model, np.nan, dtype=self.dtype)
            kw["remaps"] = [{"n_dst": self.mmap.n_model, "src": self.mmap.src, "dst": self.mmap.dst, "w": self.mmap.weight,
                             "fields": [(PHASE_NORMAL, s0, 1, name, self.outs[("remap", name)]) for name in REMAP_FIELDS]}]
        self.use = output_use_of(c, variant, featured)
        if featured:
            if c.guard == "on":
                opts["check_finite"] = 3
            if c.transport == "pipeline":
                opts.update(zero_copy=0, pipeline_chunks=4, pipeline_min_chunk=1024)
            kw["output_use"] = self.use or None
            kw["received"] = self.decl.engine_arg() if self.decl else None
        else:
            kw["use_constants"] = False
        kw["options"] = opts or None
        self.kw = kw

    # -- f64cr: the inputs are rows of the fixture
    def _rows(self, s, count, start=0):
        """row numbers for `count` cells of surface type s: the fixture's own order (cr_expect.
        Fixture.fill), restricted to the rows that hold the type's constant FICE, if it has one"""
        import numpy as np

        fx = fixture()
        value = self.consts.get((s, "FICE"))
        pool = np.arange(fx.n) if value is None else np.nonzero(fx["fice"] == value)[0]
        return pool[(start + 997 * (max(s, 1) - 1) + np.arange(count)) % pool.size]

    def _fill_rows(self, case):
        fx = fixture()
        fx.fill(case)
        done = set()
        for (s, g, name), a in case.lf.field.items():  # TSUR beside a constant FICE: rows that hold it
            if name == "TSUR" and s >= 1 and (s, "FICE") in self.consts and id(a) not in done:
                done.add(id(a))
                a[:] = fx["tsur"][self._rows(s, a.shape[0], 389 * (g - 1))]

    def set_sources(self, step):
        """the model-grid values of step `step` (new at every step) and, in the twin, their
        expansion into the exchange-grid arrays it computes on"""
        import received

        d, case = self.decl, self.case
        if d is None:
            return
        for key, (mkey, _) in d.fields.items():
            src = d.sources[key]
            src[:] = received.source_values(key[2], src.shape[0], src.dtype, step)
        if is_cr(self.c):
            fx = fixture()
            for (s, g, name), (mkey, _) in d.fields.items():
                m = d.sources[(s, g, name)].shape[0]
                if name in ("PSUR", "PATM") and mkey[0] == "atm":
                    d.sources[(s, g, name)][:] = fx[name.lower()][fx.rows(m, 53 * step + 389 * (g - 1))]
                elif name in ("TSUR", "FICE"):
                    d.sources[(s, g, name)][:] = fx[name.lower()][self._rows(s, m, 53 * step)]
        if not self.featured:  # (the featured engine's exchange-grid arrays are released: NaN from the commit on)
            d.fill_exchange(case)

    def engine(self, commit=True, stream=None):
        from fcx.engine import Engine

        kw = dict(self.kw)
        if stream is not None:
            kw["stream"] = stream
        return Engine(self.case.lf, self.case.num_surface_types, self.case.methods, commit=commit, **kw)


T_INPUTS = ("TSUR", "FICE", "PSUR", "PATM", "QATM", "TATM", "UATM", "VATM", "AMOI", "CMOI", "CHEA")
UV_INPUTS = {"CCLM": ("TSUR", "FICE", "PSUR", "UATM", "VATM", "AMOM"), "MOM5": ("TSUR", "FICE", "PSUR", "UATM", "VATM", "CMOM"),
             "RCO": ("UATM", "VATM")}


def launch_reads(c, variant, g):
    """the input names the variant's launches read on grid g: on the t grid what its methods read
    there (test_gpu_constant_fields.READS), on a u / v grid what QSUR and the momentum read (RCO:
    the wind alone; FICE only where QSUR is computed on that grid, which a regridding case does on
    the t grid alone); merged grids are one grid"""
    from test_gpu_constant_fields import READS

    t = tuple(v for v in READS[variant] if v in T_INPUTS)
    uv = tuple(v for v in UV_INPUTS[variant] if not (c.consumers == "regrid" and v == "FICE"))
    if c.grids == "shared":
        return tuple(dict.fromkeys(t + uv))
    return t if g == 1 else uv


def expected_constant_kind(c, variant, key):
    """fcx_constant_info of a declared constant after the run, from the documented rule
    (include/fcx.h, fcx_bind_constant; csrc/fcx_internal.h, uniform_family): 2, an engine-filled
    array, where a launch streams it: the fp32, MOM5, RCO and register-average kernels (at T = 2 the
    t grid's averages are formed in registers on merged grids and on grids of their own); 1, no
    array, in the fp64 generic (grids of their own) and CCLM launches of one surface type, and for
    a field no launch of the variant reads.  The case's constants are kernel inputs that are
    neither averaged, regridded, accumulated nor remapped."""
    s, g, name = key
    if name not in launch_reads(c, variant, g):
        return 1
    if c.prec.startswith("f32") or c.types == "T2":
        return 2
    if c.grids == "shared" and variant != "CCLM":
        return 2
    return 1


def expected_output_kind(c, variant, key, chunked):
    """fcx_output_info of a declared output after the run, from the documented rule (include/fcx.h,
    FCX_OUT_UNREAD; csrc/fcx_internal.h, skip_family).  1: kept in a device array; 2: the store was
    left out.  chunked: the engine's host arrays could be cut into pipeline chunks."""
    s, g, name = key
    if c.outuse == "device":
        return 1
    if c.consumers == "regrid":
        return 1  # any regridding of the engine keeps every buffer
    f32 = c.prec.startswith("f32")
    merged = c.grids == "shared"
    T1 = c.types == "T1"
    ravg = not T1  # (the t grid's averages are formed in registers on every grid layout)
    accum = c.consumers in ("accum", "accum_halo", "accum_remap")
    fused = accum and merged
    halo = fused and T1 and c.consumers == "accum_halo"
    lvariant = {"CCLM": 1, "MOM5": 2, "RCO": 3}[variant] if merged else 0

    def skip_family(halo_):
        if ravg:
            return False
        if not f32 and lvariant == 1 and T1 and halo_:
            return False
        if not f32 and lvariant == 0 and not T1 and not ravg and merged:
            return False
        return True

    want_ok = skip_family(halo) and (not (chunked or not halo) or skip_family(False))
    if T1 and accum and name != "QSUR" and (name, g) in ATM_FIELDS and (merged or g == 1):
        # an accumulated field: kept unless the launch's registers are its only reader (a fused
        # launch with halo tiles, whole grids only)
        if not fused or not halo or chunked:
            return 1
    if T1 and c.consumers == "accum_remap" and name in REMAP_FIELDS:
        return 1
    wbit = name in ("RBBR", "HLAT", "HSEN", "UMOM", "VMOM")
    consumed = (ravg and name in FLUXES_T2 + ("UMOM", "VMOM")) or (fused and T1 and (name, g) in ATM_FIELDS)
    if consumed and wbit and not want_ok:
        return 1
    return 2
