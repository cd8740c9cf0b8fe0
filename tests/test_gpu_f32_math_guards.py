"""Guard bands around every array of an fp32 engine with FCX_OPT_F32_MATH on (tests/guards.py,
the gate of tests/test_gpu_guard_bands.py): no byte outside an output is written, nothing outside
an input reaches a result, no input is written, and the cells of an array past its grid size
stay untouched.  The wide kernels load and store the float arrays of the fp32 engine (the fused
ones two cells per lane in 128-cell wave tiles, the others four), so the sizes are that module's:
1025 and 4099 cells for the T = 1 fused launch (a ragged last lane, several wave tiles and one
cell past a tile), 1, 129 and 777 for the multi-type kernel."""
import pytest

from test_gpu_guard_bands import Spec, _count, gate, offsets, run_map  # noqa: F401  (_count: autouse)

pytestmark = pytest.mark.gpu

from fcx.synthetic import build_case  # noqa: E402

WIDE = {"f32_math": 1}


@pytest.mark.parametrize("lengths", [(1, 5), (1, 10), (0, 5)])
@pytest.mark.parametrize("n", [1025, 4099])
def test_fused_cclm_t1(n, lengths):
    """halo tiles, crossing records and their fix-up, a grid cap; two steps"""
    amap = run_map(n, lengths)
    for options in ({}, {"atmos_halo": 0}, {"max_blocks": 4}):
        spec = Spec(f"f32math_CCLM_n{n}_runs{lengths}", lambda: build_case("CCLM", n=n, T=1, bias=True), "float32",
                    {**options, **WIDE}, steps=2, amap=amap)
        gate(spec, "torch", offset=0)
    gate(spec, "torch", offset=8)
    gate(spec, "torch", offset=0, tail=37)


@pytest.mark.parametrize("n", [1, 129, 777])
def test_mom5_t2(n):
    """T = 2: the multi-type wide kernel at every start offset, and arrays longer than their grid"""
    spec = Spec(f"f32math_MOM5_T2_n{n}", lambda: build_case("MOM5", n=n, T=2, bias=True), "float32", dict(WIDE))
    for off in offsets("float32"):
        gate(spec, "torch", offset=off)
    gate(spec, "torch", offset=0, tail=37)
