"""Shared by the receive-side tests (fcx_bind_received): the numpy restatement of the model grid
-> exchange grid map, the maps the tests use, and the pair of engines every test compares.

The expected value everywhere is a TWIN engine: the same case, with the exchange-grid arrays
bound as ordinary arrays that `expand` filled on the host.  `expand` is the map as fcx.h states
it, an explicit loop over the links in order from 0.0 (fp32: w * (double)x32 summed in double,
rounded to float once); tests/test_receive_abi.py checks it against hand-written values."""
import numpy as np

from fcx.basic import PHASE_EARLY, PHASE_NORMAL
from fcx.engine import Engine
from fcx.parallel import geometric_maps
from parity import bits_equal

ATMOS = ("PSUR", "PATM", "QATM", "TATM", "UATM", "VATM", "AMOI", "AMOM")
BOTTOM = ("TSUR", "FICE")
EARLY = ("TSUR",)  # read by the early phase (RBBR): received before it


def expand(src, dst, w, field, n_dst, dtype=np.float64):
    """out[d] = sum over the links k with dst[k] == d, in link order from 0.0, of
    w[k] * field[src[k]], in double; an exchange cell without a link gets 0.0; rounded to dtype
    once."""
    acc = np.zeros(n_dst, dtype=np.float64)
    # (np.add.at is the explicit loop acc[dst[k]] = acc[dst[k]] + w[k] * field[src[k]] for k = 0, 1, ...:
    # unbuffered, one link after the other, each product one IEEE double multiply)
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    np.add.at(acc, dst, np.asarray(w, dtype=np.float64) * np.asarray(field, dtype=np.float64)[src])
    return acc.astype(dtype)


def links(kind, n, seed=1):
    """(n_src, src, dst, w) onto an exchange grid of n cells.
    unit: runs of 4-9 exchange cells per model cell, weight 1.0 (the intersection-grid case);
    weighted: the same runs with weights that are not 1.0; empty: unit with every 7th exchange
    cell left without a link and one model cell unused; general: two links per exchange cell in
    a shuffled link order."""
    r = np.random.Generator(np.random.PCG64([seed, n, 31]))
    runs = r.integers(4, 10, n // 4 + 2)
    owner = np.repeat(np.arange(runs.size), runs)[:n].astype(np.int32)
    n_src = int(owner[-1]) + 2 if n else 1  # (the last model cell has no exchange cell)
    dst = np.arange(n, dtype=np.int32)
    if kind == "unit":
        return n_src, owner, dst, np.ones(n)
    if kind == "weighted":
        return n_src, owner, dst, r.uniform(0.9, 1.1, n)  # (near 1: the fields stay physical)
    if kind == "empty":
        keep = (dst % 7) != 3
        return n_src, owner[keep], dst[keep], np.ones(int(keep.sum()))
    if kind == "general":
        other = ((owner + r.integers(1, n_src, n)) % n_src).astype(np.int32)
        f = r.uniform(0.6, 0.9, n)
        s2 = np.stack([owner, other], 1).reshape(-1)
        d2 = np.stack([dst, dst], 1).reshape(-1)
        w2 = np.stack([f, 1.0 - f], 1).reshape(-1)
        p = r.permutation(s2.size)
        return n_src, np.ascontiguousarray(s2[p]), np.ascontiguousarray(d2[p]), np.ascontiguousarray(w2[p])
    raise ValueError(kind)


def transposed(index, n_model):
    """The receive map of an intersection grid: exchange cell x takes the value of the model
    cell it lies in (index[x]), weight 1.0 -- the transposed exchange -> model map."""
    index = np.ascontiguousarray(index, dtype=np.int32)
    return int(n_model), index, np.arange(index.size, dtype=np.int32), np.ones(index.size)


def geometric(side):
    """(n exchange cells, atmosphere receive map, ocean receive map) of geometric_maps(side)."""
    amap, omap = geometric_maps(side)
    n = int(amap.atmos_index.size)
    return n, transposed(amap.atmos_index, amap.n_atmos), transposed(omap.dst, omap.n_model)


def source_values(name, n_src, dtype, step=0):
    """Deterministic model-grid values of a field in its physical range (one -0.0 where the
    range allows a zero), different at every step."""
    lo, hi = {"PSUR": (98000.0, 103000.0), "PATM": (97000.0, 102000.0), "QATM": (0.002, 0.012),
              "TATM": (265.0, 295.0), "UATM": (-12.0, 12.0), "VATM": (-12.0, 12.0), "AMOI": (8e-4, 2e-3),
              "AMOM": (8e-4, 2e-3), "TSUR": (271.0, 300.0), "FICE": (0.0, 1.0), "FARE": (0.1, 0.9),
              "ALBE": (0.05, 0.8), "CMOI": (8e-4, 2e-3), "CHEA": (8e-4, 2e-3), "CMOM": (8e-4, 2e-3)}[name]
    r = np.random.Generator(np.random.PCG64([sum(map(ord, name)), n_src, step, 5]))
    a = r.uniform(lo, hi, n_src)
    if name in ("UATM", "VATM", "FICE") and n_src > 2:
        a[1] = -0.0
    return a.astype(dtype)


class Declared:
    """What one test declares as received: {(s, g, name): (map key, phase)} over maps
    {key: (grid, (n_src, src, dst, w))}; sources[(s, g, name)] are the model-grid arrays."""

    def __init__(self, case, maps, fields, step=0, alloc=None):
        self.maps, self.fields, self.sources = maps, fields, {}
        dtype = np.dtype(case.lf.dtype)
        for key, (mkey, _) in fields.items():
            n_src = maps[mkey][1][0]
            vals = source_values(key[2], n_src, dtype, step)
            a = alloc(n_src, dtype) if alloc else np.empty(n_src, dtype)
            a[:] = vals
            self.sources[key] = a

    def fill_exchange(self, case):
        """the twin's host-side expansion, into the case's own arrays (aliases follow)"""
        for key, (mkey, _) in self.fields.items():
            grid, (n_src, src, dst, w) = self.maps[mkey]
            a = case.lf.field[key]
            a[:] = expand(src, dst, w, np.asarray(self.sources[key]), a.shape[0], a.dtype)

    def engine_arg(self):
        out = []
        for mkey, (grid, (n_src, src, dst, w)) in self.maps.items():
            fl = [(ph, s, g, name, self.sources[(s, g, name)]) for (s, g, name), (mk, ph) in self.fields.items()
                  if mk == mkey]
            out.append({"grid": grid, "n_src": n_src, "src": src, "dst": dst, "w": w, "fields": fl})
        return out

    def poison(self, case):
        """NaN into the exchange-grid host arrays the declaration released (after commit)"""
        for key in self.fields:
            case.lf.field[key][:] = np.nan


def standard(case, atm_map, oce_map=None, atmos=ATMOS, bottom=BOTTOM, step=0, alloc=None):
    """The atmosphere inputs of type 0 through atm_map on every grid that has arrays of its own,
    TSUR / FICE of every surface type through oce_map; merged grids declare the t grid only."""
    lf = case.lf
    n = lf.grid_size
    maps, fields = {}, {}
    for g in (1, 2, 3):
        own = g == 1 or any(lf.field.get((0, g, v)) is not lf.field.get((0, 1, v)) for v in atmos)
        if not own:
            continue
        amap = atm_map if not isinstance(atm_map, dict) else atm_map[g]
        maps[("atm", g)] = (g, amap)
        for v in atmos:
            if (0, g, v) in lf.field:
                fields[(0, g, v)] = (("atm", g), PHASE_NORMAL)
        if oce_map is not None and g == 1:
            maps[("oce", g)] = (g, oce_map)
            for s in range(1, case.num_surface_types + 1):
                for v in bottom:
                    if (s, g, v) in lf.field:
                        fields[(s, g, v)] = (("oce", g), PHASE_EARLY if v in EARLY else PHASE_NORMAL)
    assert all(m[1][2].max(initial=-1) < n[m[0] - 1] for m in maps.values())
    return Declared(case, maps, fields, step, alloc)


def snapshot(case, extra=None):
    got = {k: np.array(case.lf.field[k], copy=True) for k in case.outputs}
    for k, a in (extra or {}).items():
        got[k] = np.array(a, copy=True)
    return got


def same(got, twin, label):
    assert got.keys() == twin.keys(), label
    for k in got:
        assert np.all(np.isfinite(got[k])), f"{label}: {k} not finite"
        bad = ~bits_equal(got[k], twin[k])
        assert not bad.any(), f"{label}: {k} differs from the twin in {int(bad.sum())} cells, first {int(np.argmax(bad))}"


def pair(make, declare, run, engine_kw=None, extra=None, check=None, label=""):
    """The engine with received fields and its twin over two builds of the same case.
    make() -> case; declare(case) -> Declared; run(eng, case, decl); extra(case) -> (engine
    keywords, {key: further output arrays}); check(eng, case, decl) on the receiving engine."""
    out = []
    for recv in (True, False):
        case = make()
        decl = declare(case)
        decl.fill_exchange(case)
        kw, arrays = extra(case) if extra else ({}, {})
        kw = dict(kw, **(engine_kw or {}))
        if recv:
            kw["received"] = decl.engine_arg()
        eng = Engine(case.lf, case.num_surface_types, case.methods, corrections=case.corrections,
                     averages=case.averages, regrid=case.regrid, **kw)
        try:
            if recv:
                decl.poison(case)
                for key in decl.fields:
                    assert eng.received_info(*key)[0] == 1, (label, key)
            run(eng, case, decl)
            if recv and check:
                check(eng, case, decl)
            out.append((snapshot(case, arrays), case, decl))
        finally:
            eng.close()
    same(out[0][0], out[1][0], label)
    return out[0], out[1]
