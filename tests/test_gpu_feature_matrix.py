"""The opt-in engine features in combination, on the GPU: one test per case of the covering array
of tests/feature_matrix.py (every pair of feature levels the engine supports is in some case).

Each case runs the FEATURED engine (constants as fcx_bind_constant, declared output uses, received
fields, the guard, the transport, correctly rounded or wide math, consumers, group launch) beside
its TWIN -- the same deterministic case in the same precision and math, every field an ordinary
array (constants filled in, received fields expanded on the host), default transport, guard off --
over two steps in different bias months, and holds the featured engine to:

 a. the twin, bit for bit (parity.bits_equal): every flux output the host still reads, every output
    kept on the device (read back), every atmosphere and remap output, every regridded field; an
    output whose store was dropped is refused by fcx_device_ptr (status 2);
 b. an oracle that shares no kernel with it, by precision:
      f64      parity.assert_tight against the C oracle;
      f64cr    cr_expect.expected fed the fixture's correctly rounded values, bit for bit (the gate
               of test_gpu_cr_math.hold), with assert_tight beside it;
      f32wide  np.float32 of an fp64 engine's outputs on the widened inputs, bit for bit (a type-0
               average that a plan forms from the stored floats: the construction sum);
      f32      the norm-wise fp32 gate with the conditioning allowance (test_gpu_random_configs);
    regridding cases: assert_tight has no gate for a regridded field, so f64 / f64cr take the
    gate of test_random_regridding (1e-10 mixed with the conditioning allowance, f64cr after its
    bit-exact primary gate), and f32wide the fp32 gate (test_gpu_f32_math.test_regridding_staged:
    a regridded value is read back as the stored float);
    atmosphere and remap outputs: oracle_lib.atmos_accumulate / remap_apply of the engine's own
    fluxes (of the twin's where the host cannot read them: (a) pins those that are readable),
    assert_array_equal;
 c. the queries: fcx_field_ranges / fcx_field_integrals (weighted) over every slot the case's
    launches read or write -- constants, received fields, device-kept outputs among them -- and
    fcx_atmos_ranges / fcx_atmos_integrals, equal to numpy's min / max and to fcx.engine.ExactSum
    of the twin's host arrays; a slot whose store was dropped is refused by name;
 d. the feature really ran: fcx_constant_info, fcx_output_info (expected from the documented
    rules, feature_matrix.expected_*), fcx_received_info, fcx_cr_math, fcx_f32_math,
    fcx_fused_accumulation, fcx_last_group_size, a clean fcx_check_result;
 e. arrays the engine gave up: declared output arrays keep their sentinel bits, constant and
    received exchange-grid host arrays are NaN from the commit on, every compared result is finite.
"""
import numpy as np
import pytest

import cr_expect
import feature_matrix as fm
import oracle_lib
from parity import FP32_NORM_GATE, assert_tight, bits_equal

pytestmark = pytest.mark.gpu

from fcx import _lib, host_alloc  # noqa: E402
from fcx.basic import PHASE_ALL  # noqa: E402
from fcx.engine import Engine, ExactSum, run_group  # noqa: E402
from fcx.synthetic import as_dtype  # noqa: E402
from test_gpu_constant_fields import poison  # noqa: E402
from test_gpu_output_use import fill_sentinels, read_device, sentinel  # noqa: E402

E_STATE = 2
UNREAD = _lib.FCX_OUT_UNREAD


def same(got, want, what, label):
    got, want = np.asarray(got), np.asarray(want)
    assert np.all(np.isfinite(got.astype(np.float64))), f"{label}: {what} not finite"
    bad = ~bits_equal(got, want)
    assert not bad.any(), f"{label}: {what} differs from the twin in {int(bad.sum())} cells, first {int(np.argmax(bad))}"


def run_step(c, engines, t):
    if c.launch == "run":
        engines[0].step(PHASE_ALL, t)
        return
    for e in engines:
        e.upload(PHASE_ALL)
    run_group(engines, PHASE_ALL, t)
    for e in engines:
        e.download(PHASE_ALL)
        e.synchronize()


def skipped_arrays(m, eng):
    """id -> key of the declared arrays whose store the last plan left out (fcx_output_info 2)"""
    return {id(m.case.lf.field[k]): k for k, u in m.use.items() if u == UNREAD and eng.output_info(*k) == 2}


def expected_group_size(c, eng):
    """fcx_run_group merges the members whose phase is one fused launch of the same shape
    (include/fcx.h): the accumulation rides in the launch (merged grids, no regridding) and the
    launch does not also write a remap's records (fcx_remap_info says 2 where it does)."""
    if c.launch != "group":
        return 0
    fused = c.consumers in ("accum", "accum_halo", "accum_remap") and c.grids == "shared"
    records = c.consumers == "accum_remap" and eng.remap_info(0)[1] == 2
    return 3 if fused and not records else 0


def query_slots(m):
    """the (s, g, name) slots the member's launches read or write, one per buffer: the inputs of
    feature_matrix.launch_reads, FARE of the averaged types, and every output"""
    lf, T = m.case.lf, m.T
    keys, seen = [], set()
    for g in (1, 2, 3):
        cand = [(s, g, v) for s in range(1, T + 1) for v in fm.launch_reads(m.c, m.variant, g)]
        if T == 2:
            cand += [(s, g, "FARE") for s in (1, 2) if g == 1]
        for k in cand + [k for k in m.case.outputs if k[1] == g]:
            if k in lf.field and id(lf.field[k]) not in seen:
                seen.add(id(lf.field[k]))
                keys.append(k)
    return keys


def clone(case):
    """the case with every array copied (aliases kept)"""
    import copy

    from fcx.local_field import LocalFields

    lf = case.lf
    new_lf = LocalFields(lf.grid_size, lf.device, lf.dtype)
    copies = {}
    for key, a in lf.field.items():
        if id(a) not in copies:
            copies[id(a)] = np.array(a, copy=True)
        new_lf.field[key] = copies[id(a)]
    new_lf.allocated, new_lf.put_to, new_lf.constant = set(lf.allocated), dict(lf.put_to), dict(lf.constant)
    new = copy.copy(case)
    new.lf = new_lf
    return new


def oracle_gates(c, tm, full, t, step, label):
    """(b) for the exchange-grid outputs: tm the twin member (its arrays hold the step's inputs and
    the twin's outputs), full = the featured engine's outputs, the twin's where it cannot be read"""
    from test_gpu_random_configs import conditioned_parity

    case = tm.case
    regrid = c.consumers == "regrid"

    def rebuilt():
        """a fresh copy of the step's inputs in double (aliases kept) for every perturbation trial"""
        def make():
            return as_dtype(case, "float64") if tm.dtype == np.float32 else clone(case)  # (widening copies)
        return make

    if c.prec in ("f64", "f64cr"):
        if c.prec == "f64cr":
            fx = fm.fixture()
            want = cr_expect.expected(case, t, fx.exp, fx.pow)
            assert want, label
            for k, v in want.items():
                ok = bits_equal(full[k], v)
                assert ok.all(), (f"{label}: {k} is not the correctly rounded value in {int((~ok).sum())} of {ok.size} "
                                  f"cells, first {np.nonzero(~ok)[0][:5].tolist()}")
        ref = oracle_lib.run_case(case, "c", current_step_time=t, regrid=regrid)
        if not regrid:
            assert_tight(case, full, ref, t, label, report=False)
        elif step == 0:  # (the allowance perturbs the step-0 inputs at STEP_T)
            conditioned_parity(rebuilt(), full, ref, label, regrid=True)
    elif c.prec == "f32wide" and not regrid:
        from test_gpu_f32_math import construction, same32, twin_of

        t64 = twin_of(case)
        e64 = Engine(t64.lf, t64.num_surface_types, t64.methods, corrections=t64.corrections, averages=t64.averages,
                     use_constants=False)
        try:
            e64.step(PHASE_ALL, t)
        finally:
            e64.close()
        for k in case.outputs:
            ok = same32(full[k], t64.lf.field[k])
            if k[0] == 0 and not ok.all():  # a plan that re-reads the stored fields: all cells alike
                ok = same32(full[k], construction(case, k))
            assert ok.all(), (f"{label}: {k} is not np.float32 of the fp64 engine's value in {int((~ok).sum())} of "
                              f"{ok.size} cells, first {np.nonzero(~ok)[0][:5].tolist()}")
    elif step == 0:  # f32, and f32wide with a regridding: the fp32 gate against the fp64 oracle
        ref = oracle_lib.run_case(as_dtype(case, "float64"), "c", current_step_time=t, regrid=regrid)
        got = {k: np.asarray(v, dtype=np.float64) for k, v in full.items()}
        conditioned_parity(rebuilt(), got, ref, label, tol=FP32_NORM_GATE, eps=2.0 ** -23, normwise=True, regrid=regrid)


def consumer_gates(m, full, label):
    """(b) for the atmosphere and remap outputs: the sequential sums of the engine's own values"""
    out = np.float32 if m.dtype == np.float32 else np.float64
    if m.amap is not None:
        for name, g in m.atm_fields:
            flux = np.asarray(full[(m.s0, g, name)], dtype=np.float64)
            want = oracle_lib.atmos_accumulate(m.amap.atmos_index, m.amap.weight, flux, m.amap.n_atmos)
            want = want[m.la.atmos_offset: m.la.atmos_offset + m.la.n_atmos].astype(out)
            np.testing.assert_array_equal(m.outs[("atm", name)][: m.la.n_atmos], want, err_msg=f"{label}: atmosphere {name}")
    if m.mmap is not None:
        for name in fm.REMAP_FIELDS:
            flux = np.asarray(full[(m.s0, 1, name)], dtype=np.float64)
            want = oracle_lib.remap_apply(m.mmap.src, m.mmap.dst, m.mmap.weight, flux, m.mmap.n_model).astype(out)
            np.testing.assert_array_equal(m.outs[("remap", name)], want, err_msg=f"{label}: remap {name}")


def queries(c, m, tm, eng, skipped, label):
    """(c): ranges and weighted integrals of every slot against the twin's host arrays"""
    lf, gs = tm.case.lf, tm.case.lf.grid_size
    rng = np.random.default_rng([c.index, 77])
    areas = {g: rng.uniform(0.5, 1.5, gs[g - 1]) for g in (1, 2, 3)}
    for g in (1, 2, 3):
        eng.set_areas(g, areas[g])
    slots = query_slots(m)
    live = [k for k in slots if id(m.case.lf.field[k]) not in skipped]
    for k in slots:
        if id(m.case.lf.field[k]) in skipped:  # refused by name, not answered
            for ask in (eng.field_ranges, eng.field_integrals):
                with pytest.raises(_lib.FcxError) as ex:
                    ask([k])
                assert ex.value.status == E_STATE and "whose store the last launch that computed it left out" in str(ex.value) \
                    and k[2] in str(ex.value), f"{label}: {k}: {ex.value}"
    ranges = eng.field_ranges(live)
    sums = eng.field_integrals(live, weighted=True)
    for k, r, s in zip(live, ranges, sums):
        a = np.asarray(lf.field[k])[: gs[k[1] - 1]]
        assert np.all(np.isfinite(a)), f"{label}: the twin's {k} is not finite"
        assert (r.min, r.max, r.n_nan, r.n_inf, r.first_bad) == (float(a.min()), float(a.max()), 0, 0, -1), \
            f"{label}: range of {k}: {r} against [{a.min()!r}, {a.max()!r}]"
        assert bytes(s) == bytes(ExactSum().add_terms(a, areas[k[1]])), f"{label}: integral of {k}: {s}"
    if m.amap is not None:
        na = m.la.n_atmos
        area = rng.uniform(0.5, 1.5, max(na, 1))
        eng.set_atmos_areas(area[:na] if na else area[:0])
        want = [tm.outs[("atm", name)][:na] for name, _ in m.atm_fields]
        ranges, sums = eng.atmos_ranges(PHASE_ALL), eng.atmos_integrals(PHASE_ALL, weighted=True)
        assert len(ranges) == len(sums) == len(want), label
        for (name, _), a, r, s in zip(m.atm_fields, want, ranges, sums):
            assert (r.min, r.max, r.n_nan, r.n_inf, r.first_bad) == (float(a.min()), float(a.max()), 0, 0, -1), \
                f"{label}: atmosphere range of {name}: {r}"
            assert bytes(s) == bytes(ExactSum().add_terms(a, area[:na])), f"{label}: atmosphere integral of {name}: {s}"


def feature_ran(c, m, eng, chunked, label):
    """(d): what the engine says it did, against the documented rules"""
    for key in eng.constants:
        want = fm.expected_constant_kind(c, m.variant, key)
        assert eng.constant_info(*key) == want, f"{label}: constant_info{key} = {eng.constant_info(*key)}, the rule says {want}"
    for key in m.use:
        want = fm.expected_output_kind(c, m.variant, key, chunked)
        assert eng.output_info(*key) == want, f"{label}: output_info{key} = {eng.output_info(*key)}, the rule says {want}"
    if m.decl is not None:
        for key in m.decl.fields:
            assert eng.received_info(*key)[0] == 1, f"{label}: received_info{key}"
    assert eng.cr_math() == (c.prec == "f64cr") and eng.f32_math() == (c.prec == "f32wide"), label
    if m.amap is not None:
        fused = c.grids == "shared"  # (the specialised and the register-average launches; grids of their own: atmos_kernel)
        assert eng.fused_accumulation(PHASE_ALL) == fused, f"{label}: fused_accumulation {not fused}"
    assert eng.last_group_size() == expected_group_size(c, eng), f"{label}: group of {eng.last_group_size()}"
    if c.guard == "on":
        assert eng.check_result() is None, f"{label}: {eng.check_result()}"


@pytest.mark.parametrize("c", fm.CASES, ids=fm.case_id)
def test_case(c):
    stream = None
    if c.launch == "group":
        torch = pytest.importorskip("torch")
        stream = torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream  # one stream: the members merge
    base = fm.describe(c)
    variants = fm.members(c)
    n, sep = fm.sizes(c)
    chunked = c.transport == "pipeline" and max((n,) + (sep or ())) >= 2 * 1024
    with host_alloc.Arena() as arena:
        twins = [fm.Member(c, v, False) for v in variants]
        feats = [fm.Member(c, v, True, arena) for v in variants]
        declared = [fill_sentinels(m.case, m.use) for m in feats]  # before the commit
        te, fe = [], []
        try:
            for m in twins:
                te.append(m.engine(stream=stream))
                assert not te[-1].constants
            for m in feats:
                fe.append(m.engine(stream=stream))
            for m, eng in zip(feats, fe):
                assert set(eng.constants) == {k for k in m.case.lf.constant}, (base, m.variant)
                assert bool(eng.constants) == bool(m.consts), (base, m.variant)
                poison(eng)
                if m.decl is not None:
                    m.decl.poison(m.case)
            for step, t in enumerate(fm.STEPS):
                for m in twins + feats:
                    m.set_sources(step)  # the host receives new model-grid values
                for m in feats:
                    if m.decl is not None:
                        m.decl.poison(m.case)
                run_step(c, te, t)
                run_step(c, fe, t)
                for m, tm, eng, decl_arrays in zip(feats, twins, fe, declared):
                    label = f"{base} member={m.variant} step={step}"
                    # (e) the arrays the engine gave up
                    for a in decl_arrays.values():
                        assert np.array_equal(a.view(sentinel(a).dtype), sentinel(a)), f"{label}: a declared host array was written"
                    for key in eng.constants:
                        assert np.all(np.isnan(m.case.lf.field[key])), f"{label}: the constant's host array {key} was written"
                    # (a) the twin, bit for bit
                    skipped = skipped_arrays(m, eng)
                    full = {k: np.array(tm.case.lf.field[k], copy=True) for k in tm.case.outputs}
                    compared = 0
                    for k in m.case.outputs:
                        a = m.case.lf.field[k]
                        if id(a) in skipped:
                            with pytest.raises(_lib.FcxError) as ex:
                                eng.device_ptr(*k)
                            assert ex.value.status == E_STATE and "stale" in str(ex.value), f"{label}: {k}: {ex.value}"
                            continue
                        if id(a) in decl_arrays:  # kept on the device
                            a = read_device(eng, k, m.case.lf.grid_size[k[1] - 1], m.dtype)
                        same(a, tm.case.lf.field[k], k, label)
                        full[k] = np.array(a, copy=True)
                        compared += 1
                    for k, a in m.outs.items():
                        same(a, tm.outs[k], k, label)
                        compared += 1
                    # (all seven outputs of a single type unread and no consumer: nothing reaches the host)
                    assert compared or len(skipped) == len({id(m.case.lf.field[k]) for k in m.case.outputs}), \
                        f"{label}: nothing left to compare"
                    # (b) oracles that do not share the kernel
                    oracle_gates(c, tm, full, t, step, label)
                    consumer_gates(m, full, label)
            for m, tm, eng in zip(feats, twins, fe):
                label = f"{base} member={m.variant}"
                feature_ran(c, m, eng, chunked, label)
                queries(c, m, tm, eng, skipped_arrays(m, eng), label)
                feature_ran(c, m, eng, chunked, label)  # (a query neither fills a uniform constant nor stores an output)
        finally:
            for e in te + fe:
                e.close()
