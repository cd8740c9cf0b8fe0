"""The tight fp64 gates of tests/parity.py (assert_tight) tested on the CPU: stand-in "device"
outputs made from the C oracle.  A stand-in that differs from the oracle only the way a
legitimate device may (last-ulp exp/log) passes; every subtly wrong one fails assert_tight
while the 1e-10 gate (assert_parity) on the same data stays green -- that contrast is why the
tight gates exist.  Needs only libfco.so."""
import copy

import numpy as np
import pytest

import oracle_lib
from parity import (BOUND, BUILT, EXACT, SEEDED, _bound_cap, assert_parity, assert_tight, bits_equal, gate_of,
                    seeded_case)

pytest.importorskip("fcx")
from fcx.synthetic import build_case  # noqa: E402

if oracle_lib.load("c") is None:
    pytest.skip("libfco.so is not built", allow_module_level=True)

STEP_T = 3600 * 24 * 31
N = 4097
LV, LS = 2.501e6, 2.835e6


def oracle(case):
    return oracle_lib.run_case(case, "c", current_step_time=STEP_T)


def tight(case, got, ref, label="cpu"):
    return assert_tight(case, got, ref, STEP_T, label, report=False)


def moved(a, ulps):
    """a moved by `ulps` units in the last place (away from zero for ulps > 0)"""
    return (np.ascontiguousarray(a).view(np.int64) + np.asarray(ulps, dtype=np.int64)).view(np.float64)


def rebuild(case, got):
    """HLAT = MEVA * L and the type-0 averages again from the stand-in's own per-type values,
    the way a device forms them from its registers."""
    key_of = {id(case.lf.field[k]): k for k in got}
    value = lambda k: got[key_of[id(case.lf.field[k])]] if id(case.lf.field[k]) in key_of else case.lf.field[k]  # noqa: E731
    for s, g, name in got:
        if s >= 1 and name == "HLAT":
            m = case.methods["which_flux_heat_latent"][s - 1]
            if m in ("water", "ice"):
                got[(s, g, name)] = value((s, 1, "MEVA")) * (LV if m == "water" else LS)
    for s, g, name in got:
        if s == 0:
            acc = np.zeros_like(got[(s, g, name)])
            for i in range(1, case.num_surface_types + 1):
                acc = acc + value((i, g, name)) * case.lf.field[(i, g, "FARE")]
            got[(s, g, name)] = acc
    return got


def legitimate_device(case, ref, seed=3, qsur_ulps=1):
    """QSUR = the oracle's moved +-qsur_ulps at random; everything downstream = the oracle re-run
    seeded with that QSUR; HSEN (CCLM/MOM5) and RCO MEVA moved within half their cap."""
    rng = np.random.default_rng(seed)
    got = {k: np.array(v, copy=True) for k, v in ref.items()}
    q = {k: moved(v, qsur_ulps * rng.choice([-1, 1], v.shape)) for k, v in ref.items() if k[2] == "QSUR"}
    if q:
        got.update(oracle(seeded_case(case, q)))
    for k, v in ref.items():
        if k[0] >= 1 and k[2] != "QSUR" and gate_of(case, k) == BOUND:
            got[k] = v + rng.uniform(-0.5, 0.5, v.shape) * _bound_cap(case, k, v)
    return rebuild(case, got)


def wrong_inputs(case, name, factor, stypes=None):
    """The oracle's outputs for the case with one input array scaled: a kernel whose constant
    or operand is wrong by that factor."""
    bad = copy.deepcopy(case)  # (one deepcopy: aliases stay aliases)
    seen = set()
    for (s, g, n), a in bad.lf.field.items():
        if n == name and id(a) not in seen and (stypes is None or s in stypes):
            seen.add(id(a))
            a *= factor
    assert seen
    return oracle(bad)


def fails_tight_only(case, got, ref, gate):
    """assert_tight raises, naming `gate`; the 1e-10 gate does not see it"""
    with pytest.raises(AssertionError, match=r"\[%s\]" % gate):
        tight(case, got, ref)
    assert_parity(got, ref, label="1e-10 gate")


def test_bits_equal_signed_zero_and_nan_payload():
    a = np.array([0.0, -0.0, np.nan, 1.0, np.nan])
    b = np.array([-0.0, -0.0, np.nan, 1.0, 2.0])
    b[2:3].view(np.int64)[0] |= 0x5555  # another NaN payload
    assert bits_equal(a, b).tolist() == [False, True, True, True, False]


@pytest.mark.parametrize("variant", ["CCLM", "MOM5", "RCO"])
@pytest.mark.parametrize("T", [1, 3])
def test_legitimate_device_passes(variant, T):
    case = build_case(variant, n=N, T=T, bias=True)
    ref = oracle(case)
    got = legitimate_device(case, ref)
    rep = tight(case, got, ref)
    assert set(rep) == {"%d:%d:%s" % k for k in case.outputs}
    bounded = [v for v in rep.values() if v["gate"] == BOUND]
    assert bounded and all(0.0 < v["worst_ratio"] <= 1.0 for v in bounded)
    assert all(not v["failed_cells"] for v in rep.values())
    if variant != "RCO":  # the moved QSUR reached MEVA: the plain oracle is not what it is held to
        assert not bits_equal(got[(1, 1, "MEVA")], ref[(1, 1, "MEVA")]).all()


@pytest.mark.parametrize("variant", ["CCLM", "MOM5", "RCO"])
def test_oracle_against_itself_is_all_bit_identical(variant):
    case = build_case(variant, n=300, T=2, bias=True, sep_grids=(310, 290), rsdr=True)
    ref = oracle(case)
    rep = tight(case, ref, ref)
    assert all(v["bit_identical_share"] == 1.0 and v["worst_ratio"] == 0.0 for v in rep.values())


@pytest.mark.parametrize("per_type", [
    {2: dict(which_flux_mass_evap="copy", which_flux_heat_latent="water")},
    {2: dict(which_flux_mass_evap="zero", which_flux_heat_sensible="zero",
             which_flux_momentum="zero", which_flux_radiation_blackbody="zero")},
    {3: dict(which_flux_mass_evap="copy", which_flux_heat_latent="copy",
             which_flux_heat_sensible="copy", which_flux_momentum="copy",
             which_flux_radiation_blackbody="copy", which_spec_vapor_surface_t="copy",
             which_spec_vapor_surface_u="copy", which_spec_vapor_surface_v="copy")},
    {1: dict(which_flux_mass_evap="RCO"), 2: dict(which_flux_heat_sensible="RCO")},
])
def test_method_edges_classify_and_pass(per_type):
    """zero / copy (the bias added once more per alias: reproduced by the seeded run) / mixed
    methods: every output lands in a gate, and a legitimate device passes."""
    case = build_case("CCLM", n=1025, T=3, bias=True, per_type=per_type)
    ref = oracle(case)
    assert {gate_of(case, k) for k in case.outputs} <= {EXACT, SEEDED, BOUND, BUILT}
    tight(case, legitimate_device(case, ref), ref)


def test_copy_of_bounded_rco_meva_is_refused():
    """RCO MEVA with the bias added twice (a 'copy' alias) has no derived bound: no gate is
    weakened for it, the case is refused."""
    case = build_case("RCO", n=300, T=2, bias=True, per_type={2: dict(which_flux_mass_evap="copy")})
    with pytest.raises(AssertionError, match="more than once"):
        gate_of(case, (1, 1, "MEVA"))
    gate_of(build_case("RCO", n=300, T=2, bias=False, per_type={2: dict(which_flux_mass_evap="copy")}), (1, 1, "MEVA"))


@pytest.mark.parametrize("factor", [1.0 + 1e-12, 1.0 + 1e-13])
def test_wrong_heat_coefficient_fails(factor):
    """CHEA off in its 12th / 13th digit (MOM5 HSEN): far inside 1e-10, over the HSEN bound."""
    case = build_case("MOM5", n=N, T=1, bias=True)
    ref = oracle(case)
    fails_tight_only(case, wrong_inputs(case, "CHEA", factor), ref, BOUND)


def test_wrong_moisture_coefficient_fails():
    """AMOI off in its 12th digit (CCLM MEVA): QSUR is untouched, so the seeded run is the plain
    oracle and MEVA is not its bits.  (Bias off: MEVA is then off by 1e-12 of itself in every
    cell; with it one cell where flux and bias cancel would cross 1e-10 as well.)"""
    case = build_case("CCLM", n=N, T=1, bias=False)
    ref = oracle(case)
    fails_tight_only(case, wrong_inputs(case, "AMOI", 1.0 + 1e-12), ref, SEEDED)


def test_surface_temperature_off_by_four_ulps_fails():
    """TSUR * (1 + 4 eps): sigma T^4 is no longer the oracle's bits.  (1025 cells: on a larger grid
    some cell has |T_s - T_a EF| < 3e-3 K, where 4 eps of T_s alone are 1e-10 of HSEN.)"""
    case = build_case("CCLM", n=1025, T=1, bias=True)
    ref = oracle(case)
    got = wrong_inputs(case, "TSUR", 1.0 + 4 * 2.0 ** -52)
    with pytest.raises(AssertionError, match=r"RBBR'\) \[%s\]" % EXACT):
        tight(case, got, ref)
    assert_parity(got, ref, label="1e-10 gate")


def test_average_in_reverse_type_order_fails():
    """One cell of a type-0 average summed in reverse type order (T = 3)."""
    case = build_case("MOM5", n=N, T=3, bias=True)
    ref = oracle(case)
    for key in ((0, 1, "RBBR"), (0, 1, "HSEN")):
        got = {k: np.array(v, copy=True) for k, v in ref.items()}
        rev = np.zeros(N)
        for s in (3, 2, 1):
            rev = rev + ref[(s, 1, key[2])] * case.lf.field[(s, 1, "FARE")]
        j = int(np.nonzero(~bits_equal(rev, ref[key]))[0][0])
        got[key][j] = rev[j]
        fails_tight_only(case, got, ref, BUILT)


def test_one_meva_cell_one_ulp_off_fails():
    case = build_case("CCLM", n=N, T=1, bias=True)
    ref = oracle(case)
    got = {k: np.array(v, copy=True) for k, v in ref.items()}
    got[(1, 1, "MEVA")][1234:1235] = moved(ref[(1, 1, "MEVA")][1234:1235], 1)
    rebuild(case, got)  # (HLAT follows the moved MEVA: only the seeded gate can see it)
    with pytest.raises(AssertionError, match=r"MEVA'\) \[%s\].*: 1 of %d cells" % (SEEDED, N)):
        tight(case, got, ref)
    assert_parity(got, ref, label="1e-10 gate")


def test_qsur_64_ulps_off_fails():
    """A coarse exp: QSUR 64 ulps off, everything downstream consistent with it."""
    case = build_case("CCLM", n=N, T=1, bias=True)
    ref = oracle(case)
    got = legitimate_device(case, ref, qsur_ulps=64)
    with pytest.raises(AssertionError, match=r"QSUR'\) \[%s\]" % BOUND):
        tight(case, got, ref)
    assert_parity(got, ref, label="1e-10 gate")


def test_latent_heat_of_ice_on_water_fails():
    """HLAT formed with kLs where the method says water.  (13 % off: the 1e-10 gate sees this one
    too; it is here for the MEVA_dev * L identity, which must name the right L per type.)"""
    case = build_case("RCO", n=N, T=1, bias=True)
    ref = oracle(case)
    got = {k: np.array(v, copy=True) for k, v in ref.items()}
    got[(1, 1, "HLAT")] = got[(1, 1, "MEVA")] * LS
    with pytest.raises(AssertionError, match=r"HLAT'\) \[%s\]" % BUILT):
        tight(case, got, ref)


def test_positive_zero_for_negative_zero_fails():
    """UMOM = -(fa * u) is -0.0 where u = +0.0; a kernel that writes +0.0 there is equal under
    ==, and under the 1e-10 gate, but not the reference's bits."""
    case = build_case("RCO", n=300, T=1, bias=True)
    case.lf.field[(0, 1, "UATM")][7] = 0.0
    ref = oracle(case)
    assert np.signbit(ref[(1, 2, "UMOM")][7]) and ref[(1, 2, "UMOM")][7] == 0.0
    got = {k: np.array(v, copy=True) for k, v in ref.items()}
    got[(1, 2, "UMOM")][7] = 0.0
    fails_tight_only(case, got, ref, EXACT)
