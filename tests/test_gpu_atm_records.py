"""FCX_OPT_ATM_RECORDS: the engine-owned atmosphere outputs kept on the device as one record
per atmosphere cell instead of one array per field.  The layout changes where the fused
kernels store and nothing of what they compute, and the downloads unpack the records first,
so every case builds the same engines twice -- atm_records 0 (the arrays, the yardstick) and
1 -- and requires every downloaded atmosphere output and every flux output to be the same
bytes.  Shapes are the smallest that reach each path: one wave tile plus a cell, three halo
tiles with a partial last one, maps that take the crossing records and the fix-up, maps with
empty atmosphere cells, several surface types, five fields, one atmosphere cell, shards."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from fcx.basic import PHASE_ALL, PHASE_NORMAL  # noqa: E402
from fcx.engine import Engine, run_group  # noqa: E402
from fcx.parallel import AtmosMap, local_atmos  # noqa: E402
from fcx.synthetic import build_case  # noqa: E402
from fcx.workload import ATM_FIELDS, VARIANTS, Workload  # noqa: E402

# mirrors of the host arrays on the device (no zero-copy at these sizes), direct downloads
BASE = {"zero_copy": 0, "host_staging": 0, "atmos_in_run": 0}


def run_map(n, lengths, seed):
    from test_gpu_multirank import random_run_map

    return random_run_map(n, lengths, seed)


class Rig:
    """One engine per variant over its own case, host arrays for every output."""

    def __init__(self, variants, n, amap, records, T=1, fields=ATM_FIELDS, options=None, seed=77):
        self.la = local_atmos(amap, 0, 1)
        self.cases, self.engines, self.outs = [], [], []
        opts = dict(BASE)
        opts.update(options or {})
        opts["atm_records"] = records
        s0 = 0 if T >= 2 else 1
        for v in variants:
            c = build_case(v, n=n, T=T, bias=True, seed=seed)
            o = {name: np.full(max(self.la.n_atmos, 1), np.nan) for name, _ in fields}
            atm = {"local": self.la, "fields": [(PHASE_NORMAL, s0, g, name, o[name]) for name, g in fields]}
            e = Engine(c.lf, c.num_surface_types, c.methods, corrections=c.corrections, averages=c.averages,
                       atmos=atm, options=opts)
            self.cases.append(c)
            self.engines.append(e)
            self.outs.append(o)

    def upload(self):
        for e in self.engines:
            e.upload(PHASE_ALL)

    def run(self, t, group=False):
        if group:
            run_group(self.engines, PHASE_ALL, t)
        else:
            for e in self.engines:
                e.run(PHASE_ALL, t)
        for e in self.engines:
            e.run_atmos(PHASE_ALL)

    def download(self):
        for e in self.engines:
            e.download(PHASE_ALL)
            e.synchronize()
        got = {}
        for i, (c, o) in enumerate(zip(self.cases, self.outs)):
            for k in c.outputs:
                got[(i,) + k] = np.array(c.lf.field[k], copy=True)
            for name, a in o.items():
                got[(i, "atm", name)] = a[: self.la.n_atmos].copy()
        return got

    def close(self):
        for e in self.engines:
            e.close()


def same_bytes(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    atm = [k for k in a if k[1] == "atm"]
    assert atm and all(np.isfinite(a[k]).all() for k in atm)  # every cell was written


def pair(variants, n, amap, group=False, expect=True, **kw):
    """the outputs with atm_records 0 and 1; expect: the records are in use with 1 (None: either)"""
    res = []
    for records in (0, 1):
        rig = Rig(variants, n, amap, records, **kw)
        try:
            on = [e.atm_records() for e in rig.engines]
            assert not any(on) if records == 0 else expect is None or all(x == expect for x in on)
            rig.upload()
            rig.run(3600, group)
            res.append(rig.download())
        finally:
            rig.close()
    same_bytes(*res)


@pytest.mark.parametrize("n", [129, 300])
@pytest.mark.parametrize("who", ["CCLM", "MOM5", "RCO", "group"])
def test_halo_tiles(n, who):
    """fp64, T = 1, random runs of 3..5 cells: the halo launch, whose waves store their runs of
    records densely.  129 cells: one wave tile plus a cell; 300: three halo tiles, the last one
    partial.  Each variant's own launch, and the three in one group launch."""
    amap = run_map(n, (3, 5), seed=3)
    if who == "group":
        pair(VARIANTS, n, amap, group=True)
    else:
        pair((who,), n, amap)


@pytest.mark.parametrize("group", [False, True])
def test_crossing_records_and_fixup(group):
    """Runs of 1..10 cells are too long for the halo: crossing records and the fix-up launch
    (of one engine, and the group's), which store single values into the records."""
    pair(VARIANTS if group else ("CCLM",), 300, run_map(300, (1, 10), seed=5), group=group)


def test_halo_tiles_off():
    pair(("MOM5",), 300, run_map(300, (3, 5), seed=3), options={"atmos_halo": 0})


@pytest.mark.parametrize("group", [False, True])
def test_empty_atmosphere_cells(group):
    """Runs of 0..5 cells: atmosphere cells without exchange cells are zeroed after the launch
    (atmos_zero_kernel), and a wave whose segments skip such a cell stores record by record."""
    amap = run_map(300, (0, 5), seed=41)
    assert np.setdiff1d(np.arange(amap.n_atmos), amap.atmos_index).size > 0
    pair(VARIANTS if group else ("RCO",), 300, amap, group=group)


def test_two_surface_types():
    """Water + ice: the type-0 averages held in registers are what is accumulated."""
    pair(("CCLM", "MOM5"), 300, run_map(300, (3, 5), seed=3), T=2)
    pair(("CCLM", "MOM5"), 300, run_map(300, (3, 5), seed=3), T=2, group=True)


def test_five_fields():
    """Five registered fields: records of five values (no dense store), or a clean fallback."""
    pair(("CCLM",), 300, run_map(300, (3, 5), seed=3), fields=ATM_FIELDS[:5], expect=None)


def test_one_field_keeps_the_arrays():
    pair(("CCLM",), 300, run_map(300, (3, 5), seed=3), fields=ATM_FIELDS[:1], expect=False)


@pytest.mark.parametrize("n", [5, 300])
def test_one_atmosphere_cell(n):
    """n_atmos = 1: a single segment (5 cells: the fused launch; 300: longer than half a wave
    tile, the separate accumulation kernel)."""
    w = np.random.default_rng(9).uniform(0.5, 1.5, n)
    amap = AtmosMap(np.zeros(n, dtype=np.int32), np.ascontiguousarray(w / w.sum()), 1)
    pair(("CCLM",), n, amap)


def test_long_segments_use_the_accumulation_kernel():
    pair(("CCLM",), 700, run_map(700, (130, 140), seed=7))


def test_three_shards_in_one_process():
    """A 600-cell grid as three shards: the shared boundary slots summed (the all-reduce) and
    written back into the records by atmos_finish."""
    import torch

    res = []
    for records in (0, 1):
        shards = [Workload(600, r, 3, variants=VARIANTS, atmos_map="random",
                           engine_options={"zero_copy": 0, "atm_records": records}) for r in range(3)]
        try:
            assert all(e.atm_records() == bool(records) for wl in shards for e in wl.engines)
            assert any(wl.la.left >= 0 or wl.la.right >= 0 for wl in shards)
            for wl in shards:
                wl.run_group(3600)
            total = sum(wl.shared for wl in shards)
            for wl in shards:
                wl.shared.copy_(total)
                wl.finish()
                wl.download()
            torch.cuda.synchronize()
            got = {}
            for r, wl in enumerate(shards):
                for i, (c, o) in enumerate(zip(wl.cases, wl.atm_outs)):
                    for k in c.outputs:
                        got[(r, i) + k] = np.array(c.lf.field[k], copy=True)
                    for name, _ in ATM_FIELDS:
                        got[(r, i, "atm", name)] = o[name][: wl.la.n_atmos].copy()
            res.append(got)
        finally:
            for wl in shards:
                wl.close()
    assert res[0].keys() == res[1].keys()
    for k in res[0]:
        assert res[0][k].tobytes() == res[1][k].tobytes(), k


@pytest.mark.parametrize("path", ["direct", "staging", "step"])
def test_download_paths(path):
    """The direct copies, the staging arena of caller heap arrays (host_staging 1), and the
    pipelined step (fcx_step over four chunks), each after the unpack launch."""
    n = 5000
    amap = run_map(n, (3, 5), seed=11)
    opts = {"direct": {}, "staging": {"host_staging": 1},
            "step": {"host_staging": 1, "pipeline_min_chunk": 1024, "pipeline_chunks": 4, "atmos_in_run": 1}}[path]
    res = []
    for records in (0, 1):
        rig = Rig(("CCLM",), n, amap, records, options=opts)
        try:
            assert rig.engines[0].atm_records() == bool(records)
            if path == "step":
                rig.engines[0].step(PHASE_ALL, 3600)
                rig.engines[0].synchronize()
                c, o = rig.cases[0], rig.outs[0]
                got = {(0,) + k: np.array(c.lf.field[k], copy=True) for k in c.outputs}
                got.update({(0, "atm", name): a[: rig.la.n_atmos].copy() for name, a in o.items()})
                res.append(got)
            else:
                rig.upload()
                rig.run(3600)
                res.append(rig.download())
        finally:
            rig.close()
    same_bytes(*res)


def test_run_download_run_download():
    """The arrays the downloads read are refreshed from the records before every download."""
    n = 300
    amap = run_map(n, (3, 5), seed=3)
    res = []
    for records in (0, 1):
        rig = Rig(("CCLM",), n, amap, records)
        try:
            rig.upload()
            rig.run(3600)
            first = rig.download()
            seen = set()
            for key, arr in rig.cases[0].lf.field.items():  # new air temperatures
                if key[2] == "TATM" and id(arr) not in seen:
                    seen.add(id(arr))
                    arr += 1.5
            rig.upload()
            rig.run(7200)
            second = rig.download()
            assert any(first[k].tobytes() != second[k].tobytes() for k in first if k[1] == "atm")
            res.append((first, second))
        finally:
            rig.close()
    same_bytes(res[0][0], res[1][0])
    same_bytes(res[0][1], res[1][1])


def test_auto_starts_at_two_pipeline_chunks():
    """atm_records 2 (auto, the default): off on a 32,768-cell grid, whose steps download every
    time and are dispatch-bound; on from 2 x PIPELINE_MIN_CHUNK exchange cells -- where the
    whole-grid launch is the halo launch that stores the records densely: not on a map whose
    runs of 4 cells never cross a wave tile, nor on one whose runs are too long for the halo."""
    for n, chunk, runs, want in ((32_768, None, (3, 5), False), (32_768, 16_384, (3, 5), True),
                                 (32_767, 16_384, (3, 5), False), (2 * 256 * 1024, None, (3, 5), True),
                                 (32_768, 16_384, (4, 4), False), (32_768, 16_384, (1, 10), False)):
        opts = {"zero_copy": 0, "host_staging": 0, "atm_records": 2}
        if chunk:
            opts["pipeline_min_chunk"] = chunk
        amap = run_map(n, runs, seed=1)
        c = build_case("CCLM", n=n, T=1, bias=False, seed=1)
        la = local_atmos(amap, 0, 1)
        o = {name: np.empty(la.n_atmos) for name, _ in ATM_FIELDS}
        atm = {"local": la, "fields": [(PHASE_NORMAL, 1, g, name, o[name]) for name, g in ATM_FIELDS]}
        e = Engine(c.lf, 1, c.methods, atmos=atm, options=opts)
        try:
            assert e.atm_records() == want, (n, chunk)
        finally:
            e.close()
