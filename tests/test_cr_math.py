"""csrc/fcx_crmath.h on the CPU: the header compiled by plain g++ into tests/cpp/cr_math_check.cpp
(-ffp-contract=off, address and undefined-behaviour sanitizers) and run over every case of
tests/golden/cr_math.npz.  Inside its domains the header uses IEEE operations only, so what
this program returns is what the gfx950 build returns (tests/test_gpu_cr_math.py holds the
device to the same file).  The fixture was written by tests/tools/make_cr_fixture.py with
mpmath at 300 bits; nothing here needs mpmath.

The header has ONE phase, the accurate one (its comment says why), so there is no fast phase's
rounding test to hold; the accurate phase is called directly beside the public functions."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import cr_expect
import oracle_lib
from parity import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "cr_math_check.cpp")
INC = os.path.join(ROOT, "components.flux_calculator_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cr_math.npz")

SITE_BIT = {"qsur": 1, "rco": 2, "exner": 4}  # the fixture's kind: the cell is a hard case of the site


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """the header's host build; the tests that use it need g++, the others do not"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("cr_math")
    exe = str(d / "cr_math_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + INC, SRC, "-o", exe], check=True)

    def run(mode, args):
        a = np.ascontiguousarray(args, dtype=np.float64)
        a.tofile(str(d / "in.bin"))
        r = subprocess.run([exe, mode, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0 and "CR_MATH_CHECK_OK" in r.stdout, r.stdout + r.stderr
        o = np.fromfile(str(d / "out.bin"), dtype=np.float64).reshape(-1, 4)
        return {"value": o[:, 0], "accurate": o[:, 1], "in_domain": o[:, 2] == 1.0, "default": o[:, 3]}

    return run


@pytest.fixture(scope="module")
def fx():
    return cr_expect.Fixture(GOLDEN)


def test_fixture_shape(fx):
    """The file as tests/tools/make_cr_fixture.py writes it: under 300 KB; a thousand hard cases
    for each temperature site and two thousand for the Exner power (every hard temperature cell
    is a hard Exner cell too), the nearest of which no evaluation with an error above 2^-76 rounds
    without more precision; ordinary draws for every site; arguments that are the formulas' own.
    Keeping the k nearest of N uniform draws leaves distances up to about k / 2N ulp: 5e-5 for
    1,000 of 10^7, 1e-4 for 2,000."""
    assert os.path.getsize(GOLDEN) <= 300 * 1000
    kind = fx["kind"]
    for site, bit in SITE_BIT.items():
        hard = (kind & bit) != 0
        d = fx[site + "_dist"]
        assert hard.sum() >= (2000 if site == "exner" else 1000)
        assert np.isnan(d[~hard]).all()
        assert d[hard].max() < 2e-4 and d[hard].min() < 2.0 ** -22  # ulps from a rounding midpoint
        assert (~hard).sum() >= 1680
    assert (kind == 0).sum() >= 1680
    assert bits_equal(fx["qsur_arg"], cr_expect.qsur_arg(fx["fice"], fx["tsur"])).all()
    assert bits_equal(fx["rco_arg"], cr_expect.rco_arg(fx["tsur"])).all()
    assert bits_equal(fx["exner_x"], fx["psur"] / fx["patm"]).all()


@pytest.mark.parametrize("site", ["qsur", "rco"])
def test_cr_exp_every_case(checker, fx, site):
    """cr_exp and the accurate phase called directly equal the 300-bit rounding in every case,
    the hard ones (from 5e-8 ulp of a midpoint on) included; none is set aside."""
    o = checker("exp", fx[site + "_arg"])
    assert o["in_domain"].all()
    assert bits_equal(o["value"], fx[site + "_res"]).all()
    assert bits_equal(o["accurate"], fx[site + "_res"]).all()


def test_cr_pow_every_case(checker, fx):
    x = fx["exner_x"]
    o = checker("pow", np.stack([x, np.full_like(x, fx.y)], axis=1).ravel())
    assert o["in_domain"].all()
    assert bits_equal(o["value"], fx["exner_res"]).all()
    assert bits_equal(o["accurate"], fx["exner_res"]).all()


def test_whole_domain_of_the_power(checker):
    """x over [0.5, 2] with its ends, the neighbours of 1 and the reduction's branch points:
    against Python's exact rational arithmetic where the power is exact (y = 1: x**1 = x;
    y = 0.5 on squares), so the test needs no wider reference."""
    r = np.random.Generator(np.random.PCG64(7))
    x = np.concatenate([[0.5, 2.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), math.sqrt(2.0), math.sqrt(0.5),
                         np.nextafter(math.sqrt(2.0), 2.0), np.nextafter(math.sqrt(0.5), 0.0)],
                        r.uniform(0.5, 2.0, 500)])
    o = checker("pow", np.stack([x, np.ones_like(x)], axis=1).ravel())
    assert o["in_domain"].all() and bits_equal(o["value"], x).all()
    q = np.floor(r.uniform(0.7072, 1.4142, 500) * 2.0 ** 26) / 2.0 ** 26  # 27-bit roots: exact squares
    o = checker("pow", np.stack([q * q, np.full_like(q, 0.5)], axis=1).ravel())
    assert o["in_domain"].all() and bits_equal(o["value"], q).all()


def test_fallback_outside_the_domain(checker):
    """NaN, +-Inf, 0, a negative base, an overflowing and an underflowing argument, and arguments
    below 2^-30 take the default build's function: exactly exp(x) / exp(y * log(x))."""
    inf, nan = float("inf"), float("nan")
    xs = np.array([nan, inf, -inf, 0.0, -0.0, 710.0, 1000.0, -746.0, -1000.0, 690.5, 1e-10, -1e-10, 2.0 ** -31, 5e-324])
    o = checker("exp", xs)
    assert not o["in_domain"].any()
    assert bits_equal(o["value"], o["default"]).all()
    assert o["value"][1] == inf and o["value"][2] == 0.0 and o["value"][3] == 1.0 and o["value"][5] == inf
    y = cr_expect.EXNER_Y
    pairs = np.array([[nan, y], [inf, y], [0.0, y], [-1.0, y], [-0.0, y], [1.0, y], [2.5, y], [0.49, y], [1e300, y],
                      [5e-324, y], [1.01, nan], [1.01, 0.0], [1.01, 2.0], [1.01, -y], [1.01, inf]])
    o = checker("pow", pairs.ravel())
    assert not o["in_domain"].any()
    assert bits_equal(o["value"], o["default"]).all()
    assert np.isnan(o["value"][3]) and o["value"][2] == 0.0 and o["value"][1] == inf and o["value"][5] == 1.0
    # the domain's own ends are inside
    assert checker("exp", np.array([2.0 ** -30, -2.0 ** -30, 690.0, -690.0]))["in_domain"].all()
    assert checker("pow", np.array([0.5, 0.0625, 2.0, 1.0]))["in_domain"].all()


def test_libm_share_on_the_ordinary_draws(fx):
    """What bounds the GPU test's share of cells that differ from the live oracle: this host's
    libm against the correct rounding, per site on the cells that are ordinary draws for that
    site (its hard cases are chosen within 1e-4 ulp of a midpoint, where a libm good to an ulp
    misrounds almost every other one; over all rows no correctly rounding engine could meet a 0.5 %
    cap).  At most 0.5 %."""
    for site in ("qsur", "rco"):
        ordinary = (fx["kind"] & SITE_BIT[site]) == 0
        differs = ~bits_equal(cr_expect.libm_exp(fx[site + "_arg"]), fx[site + "_res"])
        assert differs[ordinary].mean() <= 0.005
    ordinary = (fx["kind"] & SITE_BIT["exner"]) == 0
    differs = ~bits_equal(cr_expect.libm_pow(fx["exner_x"], fx.y), fx["exner_res"])
    assert differs[ordinary].mean() <= 0.005


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("variant", ["CCLM", "MOM5", "RCO"])
def test_cr_expect_is_the_oracle_with_libm(variant, T):
    """cr_expect pinned: with libm's own math.exp and math.pow it equals the C oracle on a
    build_case of 4,097 cells, bit for bit in every cell, for each variant (T = 2: an ice type
    with HLAT 'ice' and per-type bottom fields)."""
    from fcx.synthetic import build_case

    t = 3600 * 24 * 31
    case = build_case(variant, n=4097, T=T, bias=True)
    ref = oracle_lib.run_case(case, "c", current_step_time=t)
    exp = cr_expect.expected(case, t, cr_expect.libm_exp, cr_expect.libm_pow)
    want = {"CCLM": {"QSUR", "HSEN"}, "MOM5": {"QSUR", "HSEN"}, "RCO": {"MEVA", "HLAT"}}[variant]
    assert {k[2] for k in exp} == want
    assert len(exp) >= T * len(want)
    for k, v in exp.items():
        assert bits_equal(v, ref[k]).all(), k


def test_fixture_fills_a_case(fx):
    """Fixture.fill puts table rows into a case so that every site argument is in the table: the
    look-up functions then cover the whole case (a KeyError otherwise)."""
    from fcx.synthetic import build_case

    for variant, T, sep in (("CCLM", 1, None), ("RCO", 3, None), ("MOM5", 2, (310, 290))):
        case = fx.fill(build_case(variant, n=300, T=T, bias=True, sep_grids=sep))
        exp = cr_expect.expected(case, 0, fx.exp, fx.pow)
        assert exp and all(np.isfinite(v).all() for v in exp.values())
