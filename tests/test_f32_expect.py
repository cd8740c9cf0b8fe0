"""tests/f32_expect.py, the float32 restatement of the plain fp32 engine, on the CPU.

1. The restatement pinned to csrc/fcx_physics.h: the header compiled at R = float by plain g++
   into tests/cpp/f32_physics_check.cpp (-ffp-contract=off, address and undefined-behaviour
   sanitizers, nothing preloaded) and run over a table of random cells and of the edges where a
   formula takes another branch; every formula bit for bit through uint32 views.  Both sides
   take the same site functions, this host's libm exp / log in double rounded to float once.
2. The proof that parity.assert_tight_f32 sees what FP32_NORM_GATE does not (the analogue of
   tests/test_ulp_gate.py): mutants of the restatement play the device.  Each one stays inside the
   norm-wise 1e-5 gate against the fp64 oracle and fails the tight gate.
"""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import f32_expect as fx
import oracle_lib
from parity import (BOUND, BUILT, EXACT, FP32_NORM_GATE, SEEDED, assert_tight_f32, bits_equal32, error_report,
                    gate_of)

pytest.importorskip("fcx")
from fcx.synthetic import as_dtype, build_case  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "f32_physics_check.cpp")
INC = os.path.join(ROOT, "components.flux_calculator_amd", "csrc")
STEP_T = 3600 * 24 * 31  # inside February 1961
F = np.float32

IN_COLS = ("fice", "ps", "pa", "ts", "ta", "qa", "qs", "u", "v", "a", "bias", "f1", "f2")
OUT_COLS = ("qsur", "vel", "meva_cclm", "meva_rco", "hsen_cclm", "hsen_rco", "mom_cclm_rate", "mom_rco_rate",
            "rbbr", "t_tilde", "rate_num", "ta_exner", "pow_exner", "mom_num", "mom_cclm_rate_num",
            "meva_cclm_num", "hsen_cclm_num", "site_exp", "umom_cclm", "vmom_rco", "hlat_water", "hlat_ice",
            "meva_bias", "average")


def libm_exp(x):
    """(float) ::exp((double) x), as the check program declares fcx::exp(float)"""
    x = np.asarray(x)
    assert x.dtype == np.float32
    return np.array([math.exp(float(v)) for v in x.ravel()], dtype=np.float64).astype(np.float32).reshape(x.shape)


def libm_log(x):
    x = np.asarray(x)
    assert x.dtype == np.float32
    return np.array([math.log(float(v)) for v in x.ravel()], dtype=np.float64).astype(np.float32).reshape(x.shape)


def rocm_include():
    for root in (os.environ.get("ROCM_PATH"), os.environ.get("HIP_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime.h")):
            return os.path.join(root, "include")
    return None


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """the header's host build at R = float"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    inc = rocm_include()
    if inc is None:
        pytest.skip("no HIP headers")
    d = tmp_path_factory.mktemp("f32_physics")
    exe = str(d / "f32_physics_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + inc, "-I" + INC, SRC,
                    "-o", exe], check=True)

    def run(table):
        a = np.ascontiguousarray(np.stack([table[c] for c in IN_COLS], axis=1), dtype=np.float32)
        a.tofile(str(d / "in.bin"))
        r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "F32_PHYSICS_CHECK_OK" in r.stdout, r.stdout + r.stderr
        o = np.fromfile(str(d / "out.bin"), dtype=np.float32).reshape(-1, len(OUT_COLS))
        return {c: np.ascontiguousarray(o[:, i]) for i, c in enumerate(OUT_COLS)}

    return run


def nxt(x, up):
    return np.nextafter(F(x), F(np.inf if up else -np.inf))


def make_table():
    """2,000 random cells of the synthetic distributions, then the edges (each on a random cell):
    vel just below / at / above u_min = 0.01 and vel == 0 (+0 and -0 winds); T_a == T_s and its
    two float32 neighbours; vel at 11 and its neighbours, and (6.6, 8.8); FICE 0 and 1; u == 0 or
    v == 0 with either sign; a bias that cancels MEVA (filled by the caller)."""
    r = np.random.default_rng(20231015)
    n = 2000
    t = {"fice": (r.random(n) < 0.3).astype(np.float64), "ps": r.uniform(95000.0, 105000.0, n)}
    t["pa"] = t["ps"] - r.uniform(50.0, 1500.0, n)
    t["ts"] = r.uniform(255.0, 303.0, n)
    t["ta"] = np.clip(t["ts"] + r.normal(0.0, 3.0, n), 240.0, 310.0)
    t["qa"] = r.uniform(5e-4, 2e-2, n)
    t["qs"] = r.uniform(1e-3, 2.5e-2, n)
    t["u"], t["v"] = r.normal(0.0, 7.0, n), r.normal(0.0, 7.0, n)
    t["a"] = r.uniform(5e-4, 3e-3, n)
    t["bias"] = r.normal(0.0, 1e-5, n)
    t["f1"] = r.uniform(0.0, 1.0, n)
    t = {k: v.astype(np.float32) for k, v in t.items()}
    t["f2"] = F(1) - t["f1"]
    edges = []

    def edge(row, **kw):
        e = {k: v[row] for k, v in t.items()}
        e.update({k: F(v) for k, v in kw.items()})
        edges.append(e)

    umin = F(0.01)
    for i, (u, v) in enumerate([(nxt(umin, False), 0.0), (umin, 0.0), (nxt(umin, True), 0.0), (0.0, umin),
                                (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (0.006, 0.008), (-0.006, 0.008)]):
        edge(i, u=u, v=v)
    for i in range(20, 30):
        ts = t["ts"][i]
        edge(i, ta=ts)
        edge(i, ta=nxt(ts, True))
        edge(i, ta=nxt(ts, False))
    for i, (u, v) in enumerate([(11.0, 0.0), (-11.0, 0.0), (0.0, 11.0), (nxt(11.0, False), 0.0),
                                (nxt(11.0, True), 0.0), (6.6, 8.8), (-6.6, 8.8), (8.8, 6.6), (0.0, nxt(11.0, False))]):
        edge(40 + i, u=u, v=v)
    for i in range(50, 60):
        edge(i, fice=0.0)
        edge(i, fice=1.0, ts=min(float(t["ts"][i]), 273.15))
    for i in range(60, 64):
        edge(i, u=0.0)
        edge(i, u=-0.0)
        edge(i, v=0.0)
        edge(i, v=-0.0)
    n_cancel = 16
    for i in range(70, 70 + n_cancel):
        edge(i)  # bias = -MEVA, below
    out = {k: np.concatenate([t[k], np.array([e[k] for e in edges], dtype=np.float32)]) for k in t}
    return out, n_cancel


def mirror(t):
    """every column of the check program from f32_expect, with libm's sites"""
    e, lg = libm_exp, libm_log
    vel = fx.wind(t["u"], t["v"])
    o = {"qsur": fx.qsur_cclm(t["fice"], t["ps"], t["ts"], e), "vel": vel,
         "meva_cclm": fx.meva_cclm(t["a"], t["ps"], t["qa"], t["qs"], t["ta"], vel),
         "meva_rco": fx.meva_rco(t["qa"], t["ts"], vel, e),
         "hsen_cclm": fx.hsen_cclm(t["a"], t["pa"], t["ps"], t["qa"], t["ta"], t["ts"], vel, e, lg),
         "hsen_rco": fx.hsen_rco(t["ta"], t["ts"], vel),
         "mom_cclm_rate": fx.mom_cclm_rate(t["a"], t["ps"], t["qs"], t["ts"], vel),
         "mom_rco_rate": fx.mom_rco_rate(vel), "rbbr": fx.rbbr_stbo(t["ts"]),
         "t_tilde": fx.t_tilde(t["ts"], t["qs"]), "rate_num": fx.rate_num(t["a"], vel, t["ps"]),
         "ta_exner": fx.ta_exner(t["ta"], t["ps"], t["pa"], e, lg),
         "pow_exner": fx.pow_exner(t["ps"] / t["pa"], fx.K.exner_y, e, lg),
         "mom_num": fx.mom_num(t["a"], vel, t["ps"]), "site_exp": e(t["qs"])}
    o["mom_cclm_rate_num"] = o["mom_num"] / (fx.K.rd * o["t_tilde"])
    o["meva_cclm_num"] = fx.meva_cclm_num(o["rate_num"], t["qa"], t["qs"], t["ta"])
    o["hsen_cclm_num"] = fx.hsen_cclm_num(o["rate_num"], t["qa"], t["ts"], o["ta_exner"])
    ph = fx.Physics(e, lg)
    o["umom_cclm"] = ph.momentum(o["mom_cclm_rate"], t["u"])
    o["vmom_rco"] = ph.momentum(o["mom_rco_rate"], t["v"])
    o["hlat_water"] = ph.latent(o["meva_rco"], True)
    o["hlat_ice"] = ph.latent(o["meva_rco"], False)
    o["meva_bias"] = o["meva_cclm"] + t["bias"]
    o["average"] = ph.average([o["meva_cclm"], o["meva_rco"]], [t["f1"], t["f2"]])
    for k, v in o.items():
        assert v.dtype == np.float32, k
    return o


def test_restatement_is_the_header_bit_for_bit(checker):
    t, n_cancel = make_table()
    t["bias"][-n_cancel:] = -mirror(t)["meva_cclm"][-n_cancel:]  # a bias that cancels MEVA
    want = checker(t)
    mine = mirror(t)
    assert set(mine) == set(OUT_COLS)
    for c in OUT_COLS:
        ok = bits_equal32(mine[c], want[c])
        i = np.nonzero(~ok)[0]
        assert ok.all(), (f"{c}: {i.size} of {ok.size} rows differ, first {i[:5].tolist()}: mirror "
                          f"{mine[c][i[:3]].tolist()} header {want[c][i[:3]].tolist()}")
    # the edges are what they claim to be
    assert (want["meva_bias"][-n_cancel:] == 0.0).all()
    vel = want["vel"]
    assert (vel == F(11.0)).sum() >= 3 and (vel == nxt(11.0, False)).sum() >= 1 and (vel == nxt(11.0, True)).sum() >= 1
    assert (vel == F(0.01)).sum() >= 2 and (vel == 0.0).sum() >= 4 and ((vel > 0) & (vel < F(0.01))).sum() >= 1
    assert (t["ta"] == t["ts"]).sum() >= 10
    neg0 = (want["umom_cclm"] == 0.0) & np.signbit(want["umom_cclm"])
    pos0 = (want["umom_cclm"] == 0.0) & ~np.signbit(want["umom_cclm"])
    assert neg0.any() and pos0.any()  # -(rate * +0) = -0, -(rate * -0) = +0


def test_constants_are_the_double_folded_once():
    """R(kRd / kRv) and its kin differ from the float32-folded values (else the 'folded in
    float32' mutant below would prove nothing)."""
    k = fx.K
    assert k.rd_rv.dtype == np.float32 and k.exner_y.dtype == np.float32
    assert k.rv_rd_m1 != F(fx.D_RV) / F(fx.D_RD) - F(1) or k.one_m_rd_rv != F(1) - F(fx.D_RD) / F(fx.D_RV) \
        or k.rd_rv != F(fx.D_RD) / F(fx.D_RV) or k.exner_y != F(fx.D_RD) / F(fx.D_CP)


def test_a_python_float_operand_is_refused():
    with pytest.raises(AssertionError, match="not float32"):
        fx.wind(np.ones(3), np.ones(3, np.float32))


# ---- whole cases ----------------------------------------------------------------------------
def case32(variant, n=300, T=1, **kw):
    return as_dtype(build_case(variant, n=n, T=T, bias=kw.pop("bias", True), **kw), "float32")


def oracle64(c32):
    return oracle_lib.run_case(as_dtype(c32, "float64"), "c", current_step_time=STEP_T)


needs_oracle = pytest.mark.skipif(oracle_lib.load("c") is None, reason="libfco.so is not built")


def norm_gate(got, ref, label):
    rep = error_report({k: np.asarray(v, dtype=np.float64) for k, v in got.items()}, ref)
    bad = {k: v[0] for k, v in rep.items() if not v[0] <= FP32_NORM_GATE}
    assert not bad, f"{label}: over the norm-wise gate: {bad}"


def tight(c32, got, label="cpu"):
    return assert_tight_f32(c32, got, STEP_T, label, report=False)


@needs_oracle
@pytest.mark.parametrize("variant", ["CCLM", "MOM5", "RCO"])
@pytest.mark.parametrize("shape", [dict(T=1), dict(T=3), dict(T=2, sep_grids=(310, 290), rsdr=True)],
                         ids=["T1", "T3", "T2_sep_rsdr"])
def test_restatement_passes_both_gates(variant, shape):
    """expected() on whole cases: inside the norm-wise gate of the fp64 oracle, and bit-identical
    to itself through assert_tight_f32 in every gate (every output classified and covered)."""
    c32 = case32(variant, **shape)
    got = fx.expected(c32, STEP_T)
    assert set(got) == set(c32.outputs)
    norm_gate(got, oracle64(c32), variant)
    rep = tight(c32, got)
    assert set(rep) == {"%d:%d:%s" % k for k in c32.outputs}
    assert all(v["bit_identical_share"] == 1.0 and v["worst_ratio"] == 0.0 and not v["failed_cells"]
               for v in rep.values())


@needs_oracle
@pytest.mark.parametrize("per_type", [
    {2: dict(which_flux_mass_evap="copy", which_flux_heat_latent="water")},
    {2: dict(which_flux_mass_evap="zero", which_flux_heat_sensible="zero",
             which_flux_momentum="zero", which_flux_radiation_blackbody="zero")},
    {3: dict(which_flux_mass_evap="copy", which_flux_heat_latent="copy",
             which_flux_heat_sensible="copy", which_flux_momentum="copy",
             which_flux_radiation_blackbody="copy", which_spec_vapor_surface_t="copy",
             which_spec_vapor_surface_u="copy", which_spec_vapor_surface_v="copy")},
    {1: dict(which_flux_mass_evap="RCO"), 2: dict(which_flux_heat_sensible="RCO")},
], ids=["meva_copy", "zero", "all_copy", "mixed_rco"])
def test_method_edges(per_type):
    """'zero', 'copy' (the bias added once more per alias) and mixed methods, T = 3."""
    c32 = case32("CCLM", n=1025, T=3, per_type=per_type)
    got = fx.expected(c32, STEP_T)
    norm_gate(got, oracle64(c32), "edges")
    tight(c32, got)


def moved32(a, ulps):
    return (np.ascontiguousarray(a).view(np.int32) + np.asarray(ulps, dtype=np.int32)).view(np.float32)


@pytest.mark.parametrize("variant", ["CCLM", "MOM5"])
def test_legitimate_device_passes(variant):
    """A device whose expf is an ulp off: QSUR moved +-1 ulp at random, everything downstream
    consistent with it (the seeded restatement).  Passes; MEVA is then not the unseeded bits."""
    c32 = case32(variant, n=1025, T=2)
    plain = fx.expected(c32, STEP_T)
    r = np.random.default_rng(3)
    q = {k: moved32(v, r.choice([-1, 1], v.shape)) for k, v in plain.items() if k[2] == "QSUR"}
    got = fx.expected(c32, STEP_T, qsur=q)
    rep = tight(c32, got)
    assert 0.0 < rep["1:1:QSUR"]["worst_ratio"] <= 1.0
    assert not bits_equal32(got[(1, 1, "MEVA")], plain[(1, 1, "MEVA")]).all()


def test_seed_must_be_float32():
    c32 = case32("CCLM", n=5)
    with pytest.raises(AssertionError, match="float32"):
        fx.expected(c32, STEP_T, qsur={(1, 1, "QSUR"): np.zeros(5)})


# ---- mutants: inside the norm-wise gate, outside the tight one --------------------------------
def fused(a, b, c):
    """a * b + c with one rounding: the product of two floats is exact in double; the double sum
    rounded to float (the issue's recipe for a contracted FMA)"""
    return (a.astype(np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


class FusedAverage(fx.Physics):
    def average(self, xs, fares):
        acc = np.zeros(xs[0].shape, np.float32)
        for x, fa in zip(xs, fares):
            acc = fused(x, fa, acc)
        return acc


class ReverseAverage(fx.Physics):
    def average(self, xs, fares):
        return fx.Physics.average(self, xs[::-1], fares[::-1])


def consts(**kw):
    k = fx.Consts()
    for name, v in kw.items():
        assert getattr(k, name).dtype == np.float32 and np.asarray(v).dtype == np.float32
        setattr(k, name, v)
    return k


def wrong_rd():
    rd = 287.0501
    return consts(rd=F(rd), rd_rv=F(rd / fx.D_RV), one_m_rd_rv=F(1.0 - rd / fx.D_RV),
                  rv_rd_m1=F(fx.D_RV / rd - 1.0), exner_y=F(rd / fx.D_CP))


def float_folded():
    rd, rv, cp = F(fx.D_RD), F(fx.D_RV), F(fx.D_CP)
    return consts(rd_rv=rd / rv, one_m_rd_rv=F(1) - rd / rv, rv_rd_m1=rv / rd - F(1), exner_y=rd / cp)


def patch_fused_rate(mp):
    """the a*b+c of the exchange rate: 1 + c q in t_tilde, 0.49e-3 + 0.065e-3 vel in mom_rco_rate"""
    mp.setattr(fx, "t_tilde", lambda ts, q, k=fx.K: ts * fused(q, k.rv_rd_m1, k.one))

    def mom_rco_rate(vel):
        c_aw = np.where(vel < F(11.0), F(1.2E-03), fused(vel, F(0.065E-03), F(0.49E-03)))
        return F(1.225) * c_aw * vel

    mp.setattr(fx, "mom_rco_rate", mom_rco_rate)


def patch_no_umin(mp):
    mp.setattr(fx, "rate_num", lambda a, vel, ps, k=fx.K: a * vel * ps)


def patch_vel_11(mp):
    def mom_rco_rate(vel):
        c_aw = np.where(vel <= F(11.0), F(1.2E-03), F(0.49E-03) + F(0.065E-03) * vel)
        return F(1.225) * c_aw * vel

    mp.setattr(fx, "mom_rco_rate", mom_rco_rate)


def calm_cells_near_umin(case):
    """The calm cells of fcx/synthetic.py draw |u|, |v| < 0.007: there max(vel, u_min) is up to
    twice vel, and against winds of 25 m/s the norm-wise gate does see 'vel for max(vel, u_min)'
    (1.1e-4 of max |MEVA| at n = 300).  It is blind from u_min - vel < 1e-5 * 25 m/s on: the
    calm cells are put at vel = 0.0099."""
    u, v = case.lf.field[(0, 1, "UATM")], case.lf.field[(0, 1, "VATM")]
    calm = np.sqrt(u * u + v * v) < 0.01
    assert calm.sum() >= 3
    u[calm], v[calm] = np.where(u[calm] < 0, -0.0099, 0.0099), 0.0


def one_storm_cell(case):
    """The wrong branch at vel == 11 moves UMOM or VMOM of that cell by 0.4 %: at least 5.2e-4
    N/m2, and 4.7e-4 of max |UMOM| with the synthetic winds (max 25 m/s, |UMOM| 1.6) -- the
    norm-wise gate sees that.  It stops seeing it when ONE cell of the field is large: a cell with
    (85, 85) m/s has |UMOM| 125, and the same error is 4e-6 of it.  (That a single large cell
    hides every other cell's error is what is wrong with a norm-wise gate.)"""
    u, v = case.lf.field[(0, 1, "UATM")], case.lf.field[(0, 1, "VATM")]
    at11 = np.sqrt(u * u + v * v).astype(np.float32) == F(11.0)
    assert at11.any()
    j = int(np.nonzero(~at11)[0][0])
    u[j], v[j] = 85.0, 85.0


MUTANTS = {
    # name: (variant, n, T, change of the case or None, patch(monkeypatch) or None, Physics factory, the
    # gate that must name it or None for any)
    # (1 + c q fused differs from the two roundings in 0.6 % of the cells: 4,097 cells, not 300)
    "fma_in_rate_cclm": ("CCLM", 4097, 1, None, patch_fused_rate, fx.Physics, SEEDED),
    "fma_in_rate_rco": ("RCO", 300, 1, None, patch_fused_rate, fx.Physics, EXACT),
    "fma_in_averages": ("MOM5", 300, 3, None, None, FusedAverage, BUILT),
    "krd_287.0501": ("CCLM", 300, 1, None, None, lambda: fx.Physics(k=wrong_rd()), SEEDED),
    "constants_folded_in_float32": ("MOM5", 300, 1, None, None, lambda: fx.Physics(k=float_folded()), None),
    "vel_for_max_vel_umin": ("CCLM", 300, 1, calm_cells_near_umin, patch_no_umin, fx.Physics, SEEDED),
    "vel_lt_11_inverted_at_11": ("RCO", 300, 1, one_storm_cell, patch_vel_11, fx.Physics, EXACT),
    "averages_in_reverse_order": ("MOM5", 300, 3, None, None, ReverseAverage, BUILT),
}


@needs_oracle
@pytest.mark.parametrize("name", sorted(MUTANTS))
def test_mutant_passes_the_norm_gate_and_fails_the_tight_one(name, monkeypatch):
    variant, n, T, change, patch, physics, gate = MUTANTS[name]
    case = build_case(variant, n=n, T=T, bias=True)
    if change:
        change(case)
    c32 = as_dtype(case, "float32")
    true = fx.expected(c32, STEP_T)
    with monkeypatch.context() as mp:
        if patch:
            patch(mp)
        got = fx.expected(c32, STEP_T, physics=physics())
    moved = {k: int((~bits_equal32(got[k], true[k])).sum()) for k in got}
    assert any(moved.values()), f"{name}: the mutant moves no cell of this case"
    norm_gate(got, oracle64(c32), name)
    with pytest.raises(AssertionError, match=r"\[%s\]" % (gate or ".*")):
        tight(c32, got)


def test_hsen_rco_le_for_lt_changes_no_bit():
    """'<=' for '<' in hsen_rco picks the other c_aw exactly where T_a == T_s, and there the
    formula's last factor T_s - T_a is +0: rho_a c_pa c_aw vel * (+0) is +0 for either (finite,
    positive) c_aw.  The two are the same function on finite inputs, so no gate on the output can
    tell them apart and none is claimed to; the cells are in the case (fcx/synthetic.py, 0.5 %)."""
    c32 = case32("RCO", n=1000, T=1)
    ta, ts = c32.lf.field[(1, 1, "TATM")], c32.lf.field[(1, 1, "TSUR")]
    eq = ta == ts
    assert eq.sum() >= 3
    vel = fx.wind(c32.lf.field[(1, 1, "UATM")], c32.lf.field[(1, 1, "VATM")])
    c_aw = np.where(ta <= ts, F(1.13E-03), F(0.66E-03))
    mutant = F(1.225) * F(1.008E+03) * c_aw * vel * (ts - ta)
    assert bits_equal32(mutant, fx.hsen_rco(ta, ts, vel)).all()
    assert (mutant[eq] == 0.0).all() and not np.signbit(mutant[eq]).any()


def test_refusals_are_gate_of_s():
    """The fp32 gate refuses what gate_of refuses (an RCO MEVA with the bias added twice), nothing
    else: the restatement itself computes that case."""
    c32 = case32("RCO", n=300, T=2, per_type={2: dict(which_flux_mass_evap="copy")})
    got = fx.expected(c32, STEP_T)
    with pytest.raises(AssertionError, match="more than once"):
        gate_of(c32, (1, 1, "MEVA"))
    with pytest.raises(AssertionError, match="more than once"):
        tight(c32, got)
    assert BOUND == gate_of(case32("RCO", n=300, T=1), (1, 1, "MEVA"))
