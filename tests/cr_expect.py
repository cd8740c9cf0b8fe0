"""numpy restatement of the three transcendental sites of the fp64 engine (csrc/fcx_physics.h)
and of the formulas downstream of them, with the site's function as a parameter.

Every operation is one IEEE double operation in the reference's order (numpy float64 arrays,
no fused multiply-add), so given the same exp / pow the result is the oracle's, bit for bit
(tests/test_cr_math.py pins that with libm's own math.exp and math.pow).  Given the correctly
rounded values of tests/golden/cr_math.npz it is what an engine with FCX_OPT_CR_MATH must
return, in every cell.

exp_fn(arg) and pow_fn(x, y) take float64 arrays (y a float) and return float64 arrays.

  expected(case, t, exp_fn, pow_fn) -> {(s, g, name): array} for the case's
      QSUR            method CCLM (every grid)
      MEVA, HLAT      MEVA method RCO (+ the month's bias), HLAT 'water' / 'ice' over it
      HSEN            methods CCLM and MOM5
  of every surface type s >= 1 (the type-0 averages are pinned by construction from these,
  parity.assert_tight).  Cases with 'copy' aliases are not handled.
"""
import math

import numpy as np

K_CP, K_LV, K_LS, K_RD, K_RV, K_UMIN = 1005.0, 2.501e6, 2.835e6, 287.05, 461.51, 0.01
EXNER_Y = K_RD / K_CP
_QSUR_TABLE = {1: "which_spec_vapor_surface_t", 2: "which_spec_vapor_surface_u", 3: "which_spec_vapor_surface_v"}


def libm_exp(a):
    return np.array([math.exp(x) for x in np.asarray(a, dtype=np.float64)], dtype=np.float64)


def libm_pow(x, y):
    return np.array([math.pow(v, y) for v in np.asarray(x, dtype=np.float64)], dtype=np.float64)


def qsur_arg(fice, ts):
    aw, ai, t1, t2w, t2i = 17.2693882, 21.8745584, 273.16, 35.86, 7.66
    alpha = aw + (ai - aw) * fice
    t2 = t2w + (t2i - t2w) * fice
    return alpha * (ts - t1) / (ts - t2)


def qsur_cclm(fice, ps, ts, exp_fn):
    e = 610.78 * exp_fn(qsur_arg(fice, ts))
    return (K_RD / K_RV) * e / (ps - (1.0 - K_RD / K_RV) * e)


def rco_arg(ts):
    return 17.269 * (ts - 273.15) / (ts - 35.86)


def meva_rco(qa, ts, u, v, exp_fn):
    e_w = 6.1078E+02 * exp_fn(rco_arg(ts))
    q_w = 0.62197 * e_w / 1.013E+05
    vel = np.sqrt(u * u + v * v)
    return 1.225 * 1.15E-03 * vel * (q_w - qa)


def hsen_cclm(a, pa, ps, qs, ta, ts, u, v, pow_fn):
    tt = ts * (1.0 + (K_RV / K_RD - 1.0) * qs)
    vel = np.sqrt(u * u + v * v)
    fa = a * np.maximum(vel, K_UMIN) * ps / (K_RD * tt)
    ef = pow_fn(ps / pa, EXNER_Y)
    return fa * K_CP * (ts - ta * ef)


def _host(a):
    return np.asarray(a if isinstance(a, np.ndarray) else a.detach().cpu().numpy(), dtype=np.float64)


def expected(case, t, exp_fn, pow_fn):
    import oracle_lib

    lf, out = case.lf, {}
    f = lambda s, g, name: _host(lf.field[(s, g, name)])  # noqa: E731
    for tab in case.methods.values():
        assert "copy" not in [m.rstrip() for m in tab], "cr_expect: cases with 'copy' aliases are not handled"
    bias = None
    if case.corrections is not None:
        init_date, corr = case.corrections
        bias = np.ascontiguousarray(np.asarray(corr, dtype=np.float64)[:, oracle_lib.current_month(init_date, t) - 1])
    for s in range(1, case.num_surface_types + 1):
        for g, table in _QSUR_TABLE.items():
            if case.methods[table][s - 1].rstrip() == "CCLM" and (s, g, "QSUR") in case.outputs:
                out[(s, g, "QSUR")] = qsur_cclm(f(s, g, "FICE"), f(s, g, "PSUR"), f(s, g, "TSUR"), exp_fn)
        if case.methods["which_flux_mass_evap"][s - 1].rstrip() == "RCO":
            me = meva_rco(f(s, 1, "QATM"), f(s, 1, "TSUR"), f(s, 1, "UATM"), f(s, 1, "VATM"), exp_fn)
            if bias is not None:
                me = me + bias
            out[(s, 1, "MEVA")] = me
            hl = case.methods["which_flux_heat_latent"][s - 1].rstrip()
            if hl in ("water", "ice"):
                out[(s, 1, "HLAT")] = me * (K_LV if hl == "water" else K_LS)
        m = case.methods["which_flux_heat_sensible"][s - 1].rstrip()
        if m in ("CCLM", "MOM5"):
            a = f(s, 1, "AMOI" if m == "CCLM" else "CHEA")
            out[(s, 1, "HSEN")] = hsen_cclm(a, f(s, 1, "PATM"), f(s, 1, "PSUR"), f(s, 1, "QATM"), f(s, 1, "TATM"),
                                            f(s, 1, "TSUR"), f(s, 1, "UATM"), f(s, 1, "VATM"), pow_fn)
    return out


class Fixture:
    """tests/golden/cr_math.npz: the cell table, and the sites' functions as look-ups in it."""

    def __init__(self, path):
        z = np.load(path)
        self.z = {k: z[k] for k in z.files}
        self.n = int(self.z["tsur"].shape[0])
        self.y = float(self.z["exner_y"])
        assert self.y == EXNER_Y
        bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.int64)  # noqa: E731
        self._exp = {}
        for arg, res in (("qsur_arg", "qsur_res"), ("rco_arg", "rco_res")):
            for a, r in zip(bits(self.z[arg]).tolist(), self.z[res].tolist()):
                assert self._exp.setdefault(a, r) == r
        self._pow = {}
        for a, r in zip(bits(self.z["exner_x"]).tolist(), self.z["exner_res"].tolist()):
            assert self._pow.setdefault(a, r) == r

    def __getitem__(self, k):
        return self.z[k]

    def exp(self, arg):
        """The correctly rounded exp of arguments of the table (KeyError for any other)."""
        a = np.ascontiguousarray(arg, dtype=np.float64)
        return np.array([self._exp[b] for b in a.view(np.int64).tolist()], dtype=np.float64).reshape(a.shape)

    def pow(self, x, y):
        assert y == self.y
        a = np.ascontiguousarray(x, dtype=np.float64)
        return np.array([self._pow[b] for b in a.view(np.int64).tolist()], dtype=np.float64).reshape(a.shape)

    def rows(self, n, start=0):
        """n row numbers of the table from row `start` on, wrapping around."""
        return (start + np.arange(n)) % self.n

    def fill(self, case):
        """Write the table's inputs into every TSUR / FICE / PSUR / PATM array of the case (in
        place, aliases kept): cell j of surface type s on grid g takes row (j + 997 (s - 1) +
        389 (g - 1)) mod n; the atmosphere fields (type 0, shared by the types) take the row of
        type 1.  PSUR and PATM stay paired, and TSUR and FICE, so every site argument of the
        case is an argument of the table."""
        done = set()
        for (s, g, name), a in case.lf.field.items():
            if name not in ("TSUR", "FICE", "PSUR", "PATM") or id(a) in done:
                continue
            done.add(id(a))
            st = 1 if name in ("PSUR", "PATM") else max(s, 1)
            r = self.rows(a.shape[0], 997 * (st - 1) + 389 * (g - 1))
            a[:] = self.z[name.lower()][r]
        return case
