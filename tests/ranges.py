"""The numpy restatement of fcx_field_range, shared by the range and guard tests.

min / max: np.fmin.reduce / np.fmax.reduce over the first n cells (NaN when every cell is NaN or
n = 0); the counts by np.isnan / np.isinf; first_bad = the first cell that is not finite, -1 when
there is none.  min / max are compared with ==, so either zero passes; the counts and the index
are compared exactly.
"""
import numpy as np

from fcx.engine import FieldRange


def expect(x, n=None):
    """FieldRange of the first n cells of x (all of it when n is None), by numpy."""
    x = np.asarray(x)
    x = x if n is None else x[:n]
    if x.size:
        mn, mx = float(np.fmin.reduce(x)), float(np.fmax.reduce(x))
    else:
        mn = mx = float("nan")
    bad = np.flatnonzero(~np.isfinite(x))
    return FieldRange(mn, mx, int(np.isnan(x).sum()), int(np.isinf(x).sum()), int(bad[0]) if bad.size else -1)


def same_value(a, b):
    return (a == b) or (np.isnan(a) and np.isnan(b))


def assert_range(got, want, label=""):
    """got (the engine's FieldRange) against want (expect(...))."""
    assert same_value(got.min, want.min), (label, "min", got, want)
    assert same_value(got.max, want.max), (label, "max", got, want)
    assert (got.n_nan, got.n_inf, got.first_bad) == (want.n_nan, want.n_inf, want.first_bad), (label, got, want)
