"""Field ranges inside the guard-band arena (tests/guards.py): the fields are carved out of one
device allocation between sentinel bands of NaN, each bound a few cells longer than its grid with
sentinels in the tail.  The ranges are those of the same data without bands -- nothing outside a
field's grid cells reaches a result, a sentinel NaN would show in n_nan -- and every band and
every field is byte-identical afterwards: nothing is written but the engine's own scratch.
Array starts at every 16-B offset, so both the 16-B loads and the value-by-value path run."""
import numpy as np
import pytest

from guards import GuardedArena
from ranges import assert_range, expect

pytestmark = pytest.mark.gpu

from fcx.engine import Engine  # noqa: E402
from fcx.synthetic import as_dtype, build_case  # noqa: E402


@pytest.mark.parametrize("dtype, offset", [("float64", 0), ("float64", 8), ("float32", 0), ("float32", 4),
                                           ("float32", 12)])
@pytest.mark.parametrize("n", [130, 4097])
def test_ranges_read_only_the_grid_cells_and_write_nothing(n, dtype, offset):
    case = build_case("CCLM", n=n, T=1)
    if dtype == "float32":
        case = as_dtype(case, "float32")
    arena = GuardedArena.for_case(case, "torch", offset=offset, tail=3)
    rng = np.random.default_rng([n, offset])
    try:
        for r in arena.regions:  # outputs too: every array holds numbers, some a NaN or an Inf
            x = rng.uniform(-9.0, 9.0, r.n).astype(dtype)
            if rng.integers(0, 2):
                x[rng.integers(0, r.n)] = rng.choice([np.nan, np.inf, -np.inf])
            x[r.n - 1] = 11.0  # the last grid cell counts
            arena._store(r, x)
            r.output = False  # nothing may be written
        eng = Engine(case.lf, 1, case.methods)
        try:
            arena.snapshot()
            slots = list(case.lf.field)
            got = eng.field_ranges(slots)
            for k, g in zip(slots, got):
                cells = case.lf.grid_size[k[1] - 1]
                assert_range(g, expect(arena.host(case.lf.field[k], cells)), (n, dtype, offset, k))
                assert g.max >= 11.0
            assert arena.check() == []
        finally:
            eng.close()
    finally:
        arena.close()
