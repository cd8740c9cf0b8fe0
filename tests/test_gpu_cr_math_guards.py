"""Guard bands around every array of an fp64 engine with FCX_OPT_CR_MATH on (tests/guards.py, the
gate of tests/test_gpu_guard_bands.py): no byte outside an output is written, nothing outside an
input reaches a result, no input is written.  The correctly rounded kernels load and store
exactly as the fp64 kernels do (two cells per lane, 128-cell wave tiles), at fewer waves per
SIMD; one T = 1 fused case (halo tiles, crossing records, a ragged last lane and one cell past a
tile) and one T = 2 case."""
import pytest

from test_gpu_guard_bands import Spec, _count, gate, offsets, run_map  # noqa: F401  (_count: autouse)

pytestmark = pytest.mark.gpu

from fcx.synthetic import build_case  # noqa: E402

CR = {"cr_math": 1}


@pytest.mark.parametrize("lengths", [(1, 5), (1, 10)])
def test_fused_cclm_t1(lengths):
    n = 1025
    amap = run_map(n, lengths)
    for options in ({}, {"atmos_halo": 0}):
        spec = Spec(f"crmath_CCLM_n{n}_runs{lengths}", lambda: build_case("CCLM", n=n, T=1, bias=True), "float64",
                    {**options, **CR}, steps=2, amap=amap)
        gate(spec, "torch", offset=0)
    gate(spec, "torch", offset=8)
    gate(spec, "torch", offset=0, tail=37)


@pytest.mark.parametrize("variant", ["MOM5", "RCO"])
def test_t2(variant):
    spec = Spec(f"crmath_{variant}_T2_n777", lambda: build_case(variant, n=777, T=2, bias=True), "float64", dict(CR))
    for off in offsets("float64"):
        gate(spec, "torch", offset=off)
    gate(spec, "torch", offset=0, tail=37)
