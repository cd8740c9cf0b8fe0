"""The guard-band harness (tests/guards.py) on the CPU: it reports planted faults by array,
side and offset, and the reference alone leaves every band and every pure input untouched.

The GPU gate (tests/test_gpu_guard_bands.py) only ever runs the product kernels; that the
harness CAN fail is shown here, with faults planted through numpy in both dtypes and at every
start-offset mode.  The in-place oracle runs prove that what the GPU tests assert is what the
reference itself does: no band read into a result, no band written, no input written -- and
that the synthetic cases hold no input the reference writes (the outputs of a case come from
its method tables, fcx.synthetic.build_case, never from the engine's own classification).
"""
import numpy as np
import pytest

import oracle_lib
from guards import BAND, GuardedArena, sentinels

fcx = pytest.importorskip("fcx")
from fcx.synthetic import as_dtype, build_case, build_regrid_case  # noqa: E402

NT, NU, NV = 41, 33, 27  # odd lengths, n_u < n_t
OUT_KEY, IN_KEY, U_KEY = (1, 1, "MEVA"), (0, 1, "PSUR"), (1, 2, "UMOM")


def offset_modes(dtype):
    """(offset, only): the same start offset modulo 16 B for every array, then exactly one
    array (an output, an input) misaligned with everything else aligned"""
    step = np.dtype(dtype).itemsize
    modes = [(off, None) for off in range(0, 16, step)]
    modes += [(off, key) for off in range(step, 16, step) for key in (OUT_KEY, IN_KEY)]
    return modes


MODES = [(d, off, only) for d in ("float64", "float32") for off, only in offset_modes(d)]


def guarded(dtype, offset, only, tail=0, extra=()):
    case = build_case("CCLM", n=NT, T=1, bias=False, sep_grids=(NU, NV))
    if dtype == "float32":
        case = as_dtype(case, "float32")
    arena = GuardedArena.for_case(case, "numpy", extra=extra, offset=offset, only=only, tail=tail).snapshot()
    return case, arena


@pytest.mark.parametrize("dtype,offset,only", MODES)
def test_layout(dtype, offset, only):
    """starts at the asked offset, bands of at least two layout tiles, sentinels everywhere
    else, aliases kept, values moved"""
    twin = build_case("CCLM", n=NT, T=1, bias=False, sep_grids=(NU, NV))
    case, arena = guarded(dtype, offset, only)
    assert arena.check() == []
    regs = sorted(arena.regions, key=lambda r: r.start)
    assert regs[0].start >= BAND and arena.capacity - (regs[-1].start + regs[-1].length) >= BAND
    for a, b in zip(regs, regs[1:]):
        assert b.start - (a.start + a.length) >= BAND
    for r in regs:
        want = offset if only is None or only == r.key else 0
        assert (arena.base + r.start * arena.es) % 16 == want, r.key
        assert case.lf.field[r.key].ctypes.data == arena.base + r.start * arena.es
    for key, a in twin.lf.field.items():
        assert case.lf.field[key].shape == a.shape
        np.testing.assert_array_equal(case.lf.field[key], a.astype(dtype), err_msg=str(key))
        for other, b in twin.lf.field.items():
            assert (a is b) == (case.lf.field[key] is case.lf.field[other]), (key, other)
    inside = np.zeros(arena.capacity, dtype=bool)
    for r in regs:
        inside[r.start:r.start + r.n] = True
    bits = arena.bits()
    assert np.array_equal(bits[~inside], sentinels(dtype, 0, arena.capacity)[~inside])
    assert np.isnan(arena.buf[~inside]).all()
    assert arena.band_elements() == int((~inside).sum())


@pytest.mark.parametrize("dtype,offset,only", MODES)
def test_planted_faults_are_named(dtype, offset, only):
    for key in (OUT_KEY, IN_KEY):
        # one element before the array
        case, arena = guarded(dtype, offset, only)
        r = arena.region(key)
        arena.buf[r.start - 1] = 1.0
        assert arena.check() == [(key, "before", -1, 1)]
        # one element after it
        case, arena = guarded(dtype, offset, only)
        r = arena.region(key)
        arena.buf[r.start + r.n] = 1.0
        assert arena.check() == [(key, "after", 0, 1)]
    # a 2-cell "vector" stored at the last cell of an odd-length array
    case, arena = guarded(dtype, offset, only)
    r = arena.region(OUT_KEY)
    assert r.n % 2 == 1
    arena.buf[r.start + r.n - 1:r.start + r.n + 1] = (2.0, 3.0)
    assert arena.check() == [(OUT_KEY, "after", 0, 1)]
    # the u pass bounded by the t grid: n_t elements into the n_u-long array
    case, arena = guarded(dtype, offset, only)
    r = arena.region(U_KEY)
    assert r.n == NU
    arena.buf[r.start:r.start + NT] = np.arange(NT)
    assert arena.check() == [(U_KEY, "after", 0, NT - NU)]
    # an input written
    case, arena = guarded(dtype, offset, only)
    case.lf.field[IN_KEY][3] += 1.0
    assert arena.check() == [(IN_KEY, "input changed", 3, 1)]
    # an output written: not a violation
    case, arena = guarded(dtype, offset, only)
    case.lf.field[OUT_KEY][:] = 5.0
    assert arena.check() == []


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_shifted_band_copy_and_tail_are_seen(dtype):
    """a band copied back one element off (a transfer from a shifted position) is not its own
    pattern; with tail=k the cells past the grid are band inside the bound array"""
    case, arena = guarded(dtype, 0, None)
    r = arena.region(OUT_KEY)
    end = r.start + r.n
    arena.buf[end:end + 16] = np.array(arena.buf[end + 1:end + 17], copy=True)
    assert arena.check() == [(OUT_KEY, "after", 0, 16)]
    case, arena = guarded(dtype, 0, None, tail=37)
    for key in (OUT_KEY, IN_KEY):
        r = arena.region(key)
        assert case.lf.field[key].shape[0] == r.n + 37 == r.length
        assert np.isnan(case.lf.field[key][r.n:]).all()
    assert arena.check() == []
    case.lf.field[OUT_KEY][NT + 36] = 0.0
    case.lf.field[IN_KEY][NT] = 0.0
    assert sorted(arena.check()) == sorted([(OUT_KEY, "after", 36, 1), (IN_KEY, "after", 0, 1)])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_protected_cells_inside_an_array(dtype):
    case, arena = guarded(dtype, 0, None, extra=(18,))
    buf = arena.empty(18, "shared")
    buf[:] = 0.0
    arena.protect("shared", 6, 12)
    assert arena.check() == []
    buf[:6] = 1.0
    buf[12:] = 2.0
    assert arena.check() == []
    buf[7] = 0.0
    assert arena.check() == [("shared", "inside", 7, 1)]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_dead_lane_stand_in_poisons_the_sum(dtype):
    """a lane past the end that read the array instead of 1 and reached a sum"""
    case, arena = guarded(dtype, 0, None)
    r = arena.region(IN_KEY)
    x = arena.buf[r.start:r.start + r.n]
    assert np.isfinite(x.sum())
    assert not np.isfinite(x.sum() + arena.buf[r.start + r.n])
    assert not np.isfinite(arena.buf[r.start - 1:r.start + r.n].sum())


def oracle_cases():
    for v in ("CCLM", "MOM5", "RCO"):
        for T in (1, 3):
            yield f"{v}_T{T}", lambda v=v, T=T: build_case(v, n=1025, T=T, bias=True)
        yield f"{v}_sep", lambda v=v: build_case(v, n=600, T=2, bias=True, sep_grids=(550, 520))
        yield f"{v}_sep_rsdr", lambda v=v: build_case(v, n=513, T=2, bias=False, sep_grids=(640, 700), rsdr=True)
    yield "regrid", lambda: build_regrid_case()


ORACLE = dict(oracle_cases())


@pytest.mark.parametrize("tail", [0, 37])
@pytest.mark.parametrize("offset", [0, 8])
@pytest.mark.parametrize("name", list(ORACLE))
def test_oracle_in_place_is_clean(name, offset, tail):
    """The reference arithmetic in place on the guarded arrays (OracleState copy=False): bands
    and pure inputs bit-unchanged, outputs the bits of the run on ordinary arrays."""
    t = 3600 * 24 * 40
    twin = ORACLE[name]()
    ref = oracle_lib.run_case(twin, "c", current_step_time=t, regrid=bool(twin.regrid))
    case = ORACLE[name]()
    arena = GuardedArena.for_case(case, "numpy", offset=offset, tail=tail).snapshot()
    inputs = [r for r in arena.regions if not r.output]
    assert inputs and len(inputs) < len(arena.regions)
    o = oracle_lib.OracleState(case, t, copy=False)
    oracle_lib.run_state(o, "c", (1, 2), regrid=bool(case.regrid))
    assert arena.check() == []
    got = arena.outputs(case)
    for k, r in ref.items():
        assert np.array_equal(got[k], r, equal_nan=True), k
        assert np.isfinite(got[k]).all(), k
