"""numpy float32 restatement of the plain fp32 engine (FCX_PRECISION_F32 without
FCX_OPT_F32_MATH): every formula of csrc/fcx_physics.h at R = float and the loop glue of
process<> / uv_grid<> / momentum<> in csrc/fcx_kernels.hip, the counterpart of tests/cr_expect.py.

At R = float every operation of fcx_physics.h except the three transcendental sites (the exp of
qsur_cclm, the exp of meva_rco, pow_exner = exp(y * log x)) is one IEEE single operation in a
fixed order: the build has -ffp-contract=off, float division and sqrtf are correctly rounded on
gfx950 and denormals are kept.  numpy float32 arrays do the same operations, so given the sites'
functions the result is the device's, bit for bit.  tests/test_f32_expect.py pins this module
to the header's own host build (tests/cpp/f32_physics_check.cpp) through uint32 views.

Constants are formed as the header forms them: a decimal literal R(17.2693882) is the double
rounded once, np.float32(17.2693882); R(kRd / kRv), R(1.0 - kRd / kRv), R(kRv / kRd - 1.0) and
R(kRd / kCp) are folded in double and rounded once; the float literals of qsur_cclm / meva_rco /
hsen_rco / mom_rco_rate are combined in float32 (ai - aw, rho_a * c_aw, ...).

  expected(case32, t, exp_fn=cr_exp, log_fn=cr_log, qsur=None) -> {(s, g, name): float32 array}
      for every output of the fp32 case (fcx.synthetic.as_dtype(case, "float32")).
      exp_fn / log_fn: the sites' functions on float32 arrays; the default is the correctly
      rounded one, np.float32(np.exp(np.float64(x))).
      qsur = {(s, g, "QSUR"): array}: the seeded run of parity.seeded_case -- every QSUR method
      counts as 'none' and the given (device) arrays stand in the case's QSUR slots.

The glue follows the reference's flux-major order (oracle/fco.c), which the type-major kernel
reproduces: 'copy' is the aliased type-1 array, the month's bias slice (float32, as the engine
uploads it) is added once per type whose MEVA method is not 'none' (so parity._bias_additions
times per array), HLAT = MEVA * float32(L), UMOM / VMOM = -(rate * u), RSDR = RSDD_0, the type-0
averages acc = float32(0); acc = acc + x_s * FARE_s in type order.  The module refuses nothing
itself; parity.assert_tight_f32 refuses what parity.gate_of refuses.
"""
import numpy as np

F = np.float32
_QSUR_TABLE = {1: "which_spec_vapor_surface_t", 2: "which_spec_vapor_surface_u", 3: "which_spec_vapor_surface_v"}

# flux_constants.F90:13-32 as doubles (fcx_physics.h kCp ... kUmin)
D_CP, D_LV, D_LS, D_RD, D_RV, D_SIGMA, D_UMIN = 1005.0, 2.501e6, 2.835e6, 287.05, 461.51, 5.67e-8, 0.01


class Consts:
    """Every constant of the header at R = float.  A mutant of tests/test_f32_expect.py replaces
    members of a copy."""

    def __init__(self):
        self.cp, self.lv, self.ls, self.rd = F(D_CP), F(D_LV), F(D_LS), F(D_RD)
        self.sigma, self.umin = F(D_SIGMA), F(D_UMIN)
        self.rd_rv = F(D_RD / D_RV)  # folded in double, rounded once
        self.one_m_rd_rv = F(1.0 - D_RD / D_RV)
        self.rv_rd_m1 = F(D_RV / D_RD - 1.0)
        self.exner_y = F(D_RD / D_CP)
        self.one = F(1)


K = Consts()


def _f32(*arrays):
    for a in arrays:
        assert isinstance(a, (np.ndarray, np.float32)) and a.dtype == np.float32, f"not float32: {getattr(a, 'dtype', type(a))}"
    return arrays[0] if len(arrays) == 1 else arrays


def cr_exp(x):
    """the correctly rounded single exp: the double exp (error 2^-53 relative) rounded to float;
    a double rounding can differ from the correct rounding only within 2^-29 ulp of a float
    midpoint"""
    return _f32(np.exp(np.asarray(_f32(x), dtype=np.float64)).astype(np.float32))


def cr_log(x):
    return _f32(np.log(np.asarray(_f32(x), dtype=np.float64)).astype(np.float32))


# ---- fcx_physics.h, formula by formula -----------------------------------------------------
def qsur_arg(fice, ts):
    aw, ai, t1, t2w, t2i = F(17.2693882), F(21.8745584), F(273.16), F(35.86), F(7.66)
    alpha = aw + (ai - aw) * fice
    t2 = t2w + (t2i - t2w) * fice
    return _f32(alpha * (ts - t1) / (ts - t2))


def qsur_cclm(fice, ps, ts, exp_fn=cr_exp, k=K):
    e = F(610.78) * exp_fn(qsur_arg(fice, ts))
    return _f32(k.rd_rv * e / (ps - k.one_m_rd_rv * e))


def t_tilde(ts, q, k=K):
    return _f32(ts * (k.one + k.rv_rd_m1 * q))


def wind(u, v):
    return _f32(np.sqrt(u * u + v * v))


def rate_num(a, vel, ps, k=K):
    return _f32(a * np.fmax(vel, k.umin) * ps)


def meva_cclm_num(num, qa, qs, ts, k=K):
    fa = num / (k.rd * t_tilde(ts, qs, k))
    return _f32(fa * (qs - qa))


def meva_cclm(a, ps, qa, qs, ts, vel, k=K):
    return meva_cclm_num(rate_num(a, vel, ps, k), qa, qs, ts, k)


def rco_arg(ts):
    return _f32(F(17.269) * (ts - F(273.15)) / (ts - F(35.86)))


def meva_rco(qa, ts, vel, exp_fn=cr_exp):
    rho_a, c_aw, eps, p_0, r = F(1.225), F(1.15E-03), F(0.62197), F(1.013E+05), F(6.1078E+02)
    e_w = r * exp_fn(rco_arg(ts))
    q_w = eps * e_w / p_0
    return _f32(rho_a * c_aw * vel * (q_w - qa))


def pow_exner(x, y, exp_fn=cr_exp, log_fn=cr_log):
    return _f32(exp_fn(_f32(y * log_fn(x))))


def ta_exner(ta, ps, pa, exp_fn=cr_exp, log_fn=cr_log, k=K):
    return _f32(ta * pow_exner(ps / pa, k.exner_y, exp_fn, log_fn))


def hsen_cclm_num(num, qs, ts, taef, k=K):
    fa = num / (k.rd * t_tilde(ts, qs, k))
    return _f32(fa * k.cp * (ts - taef))


def hsen_cclm(a, pa, ps, qs, ta, ts, vel, exp_fn=cr_exp, log_fn=cr_log, k=K):
    return hsen_cclm_num(rate_num(a, vel, ps, k), qs, ts, ta_exner(ta, ps, pa, exp_fn, log_fn, k), k)


def hsen_rco(ta, ts, vel):
    rho_a, c_pa = F(1.225), F(1.008E+03)
    c_aw = np.where(ta < ts, F(1.13E-03), F(0.66E-03))
    return _f32(rho_a * c_pa * c_aw * vel * (ts - ta))


def mom_num(a, vel, ps):
    return _f32(a * vel * ps)


def mom_cclm_rate(a, ps, qs, ts, vel, k=K):
    return _f32(mom_num(a, vel, ps) / (k.rd * t_tilde(ts, qs, k)))


def mom_rco_rate(vel):
    rho_a = F(1.225)
    c_aw = np.where(vel < F(11.0), F(1.2E-03), F(0.49E-03) + F(0.065E-03) * vel)
    return _f32(rho_a * c_aw * vel)


def rbbr_stbo(ts, k=K):
    return _f32(k.sigma * (ts * ts * ts * ts))


class Physics:
    """The formulas as one replaceable set (what expected() calls): the mutants of
    tests/test_f32_expect.py subclass it."""

    def __init__(self, exp_fn=cr_exp, log_fn=cr_log, k=K):
        self.exp_fn, self.log_fn, self.k = exp_fn, log_fn, k

    def qsur_cclm(self, fice, ps, ts):
        return qsur_cclm(fice, ps, ts, self.exp_fn, self.k)

    def wind(self, u, v):
        return wind(u, v)

    def meva_cclm(self, a, ps, qa, qs, ts, vel):
        return meva_cclm(a, ps, qa, qs, ts, vel, self.k)

    def meva_rco(self, qa, ts, vel):
        return meva_rco(qa, ts, vel, self.exp_fn)

    def hsen_cclm(self, a, pa, ps, qs, ta, ts, vel):
        return hsen_cclm(a, pa, ps, qs, ta, ts, vel, self.exp_fn, self.log_fn, self.k)

    def hsen_rco(self, ta, ts, vel):
        return hsen_rco(ta, ts, vel)

    def mom_cclm_rate(self, a, ps, qs, ts, vel):
        return mom_cclm_rate(a, ps, qs, ts, vel, self.k)

    def mom_rco_rate(self, vel):
        return mom_rco_rate(vel)

    def rbbr_stbo(self, ts):
        return rbbr_stbo(ts, self.k)

    def latent(self, me, water):
        return _f32(me * (self.k.lv if water else self.k.ls))

    def momentum(self, rate, w):
        return _f32(-(rate * w))

    def average(self, xs, fares):
        """acc = 0; acc = acc + x_s * FARE_s in type order (calc:376-383)"""
        acc = np.zeros(xs[0].shape, np.float32)
        for x, fa in zip(xs, fares):
            acc = acc + x * fa
        return _f32(acc)


def _host(a):
    return a if isinstance(a, np.ndarray) else a.detach().cpu().numpy()


def month_bias(case, t):
    """the month's slice of the bias corrections as the fp32 engine uploads it: double -> float"""
    if case.corrections is None:
        return None
    import oracle_lib

    init_date, corr = case.corrections
    corr = np.asarray(corr, dtype=np.float64)
    return np.ascontiguousarray(corr[:, oracle_lib.current_month(init_date, t) - 1]).astype(np.float32)


def expected(case, t, exp_fn=cr_exp, log_fn=cr_log, qsur=None, physics=None):
    """One coupling step of the fp32 case in float32 (module docstring)."""
    ph = physics or Physics(exp_fn, log_fn)
    T = case.num_surface_types
    # a private float32 copy of every array, aliases kept
    copies, A = {}, {}
    for key, a in case.lf.field.items():
        if id(a) not in copies:
            h = _host(a)
            assert h.dtype == np.float32, f"{key}: f32_expect takes an fp32 case, got {h.dtype}"
            copies[id(a)] = np.array(h, dtype=np.float32, copy=True)
        A[key] = copies[id(a)]
    method = {tab: [m.rstrip() for m in v] for tab, v in case.methods.items()}
    if qsur is not None:  # the seeded run: the device's own QSUR, no QSUR method
        for key, q in qsur.items():
            q = np.asarray(_host(q))
            assert q.dtype == np.float32, f"{key}: the seed is not float32"
            A[key][...] = q
        for tab in _QSUR_TABLE.values():
            method[tab] = ["none"] * len(method[tab])
    f = lambda s, g, name: A[(s, g, name)]  # noqa: E731

    def put(s, g, name, val):
        out = A[(s, g, name)]
        assert val.dtype == np.float32 and val.shape == out.shape, (s, g, name, val.dtype, val.shape)
        out[...] = val

    def average(g, name):
        if (0, g, name) in case.lf.allocated:
            put(0, g, name, ph.average([f(i, g, name) for i in range(1, T + 1)],
                                       [f(i, g, "FARE") for i in range(1, T + 1)]))

    vel_of = {}

    def vel(s, g):
        key = (id(A[(s, g, "UATM")]), id(A[(s, g, "VATM")]))
        if key not in vel_of:
            vel_of[key] = ph.wind(f(s, g, "UATM"), f(s, g, "VATM"))
        return vel_of[key]

    early = [(g, n) for p, g, n in case.averages if p == 1]
    normal = [(g, n) for p, g, n in case.averages if p != 1]
    # ---- calc_flux_radiation_blackbody, the early averages
    for s in range(1, T + 1):
        m = method["which_flux_radiation_blackbody"][s - 1]
        if m == "zero":
            put(s, 1, "RBBR", np.zeros_like(f(s, 1, "RBBR")))
        elif m == "StBo":
            put(s, 1, "RBBR", ph.rbbr_stbo(f(s, 1, "TSUR")))
    for g, n in early:
        average(g, n)
    # ---- calc_spec_vapor_surface on the t, u and v grids
    done = set()
    for g, tab in _QSUR_TABLE.items():
        for s in range(1, T + 1):
            if method[tab][s - 1] == "CCLM" and (s, g, "QSUR") in A and (id(A[(s, g, "QSUR")]), s) not in done:
                done.add((id(A[(s, g, "QSUR")]), s))  # (merged grids: the u / v slots are the t array)
                put(s, g, "QSUR", ph.qsur_cclm(f(s, g, "FICE"), f(s, g, "PSUR"), f(s, g, "TSUR")))
    # ---- calc_flux_mass_evap; P2: TATM in the T_s slot of the CCLM / MOM5 formula
    bias = month_bias(case, t)
    for s in range(1, T + 1):
        m = method["which_flux_mass_evap"][s - 1]
        if m == "none":
            continue
        if m == "zero":
            put(s, 1, "MEVA", np.zeros_like(f(s, 1, "MEVA")))
        elif m in ("CCLM", "MOM5"):
            a = f(s, 1, "AMOI" if m == "CCLM" else "CMOI")
            put(s, 1, "MEVA", ph.meva_cclm(a, f(s, 1, "PSUR"), f(s, 1, "QATM"), f(s, 1, "QSUR"), f(s, 1, "TATM"),
                                           vel(s, 1)))
        elif m == "RCO":
            put(s, 1, "MEVA", ph.meva_rco(f(s, 1, "QATM"), f(s, 1, "TSUR"), vel(s, 1)))
        if bias is not None:  # every method but 'none', 'copy' (the aliased array) included
            put(s, 1, "MEVA", _f32(f(s, 1, "MEVA") + bias))
    # ---- calc_flux_heat_latent
    for s in range(1, T + 1):
        m = method["which_flux_heat_latent"][s - 1]
        if m == "zero":
            put(s, 1, "HLAT", np.zeros_like(f(s, 1, "HLAT")))
        elif m in ("water", "ice"):
            put(s, 1, "HLAT", ph.latent(f(s, 1, "MEVA"), m == "water"))
    # ---- calc_flux_heat_sensible; P3: QATM in the q_s slot
    for s in range(1, T + 1):
        m = method["which_flux_heat_sensible"][s - 1]
        if m == "zero":
            put(s, 1, "HSEN", np.zeros_like(f(s, 1, "HSEN")))
        elif m in ("CCLM", "MOM5"):
            a = f(s, 1, "AMOI" if m == "CCLM" else "CHEA")
            put(s, 1, "HSEN", ph.hsen_cclm(a, f(s, 1, "PATM"), f(s, 1, "PSUR"), f(s, 1, "QATM"), f(s, 1, "TATM"),
                                           f(s, 1, "TSUR"), vel(s, 1)))
        elif m == "RCO":
            put(s, 1, "HSEN", ph.hsen_rco(f(s, 1, "TATM"), f(s, 1, "TSUR"), vel(s, 1)))
    # ---- calc_flux_momentum_east (u grid), _north (v grid)
    for g, name, w in ((2, "UMOM", "UATM"), (3, "VMOM", "VATM")):
        for s in range(1, T + 1):
            m = method["which_flux_momentum"][s - 1]
            if m == "zero":
                put(s, g, name, np.zeros_like(f(s, g, name)))
            elif m in ("CCLM", "MOM5"):
                a = f(s, g, "AMOM" if m == "CCLM" else "CMOM")
                rate = ph.mom_cclm_rate(a, f(s, g, "PSUR"), f(s, g, "QSUR"), f(s, g, "TSUR"), vel(s, g))
                put(s, g, name, ph.momentum(rate, f(s, g, w)))
            elif m == "RCO":
                put(s, g, name, ph.momentum(ph.mom_rco_rate(vel(s, g)), f(s, g, w)))
    # ---- distribute_shortwave_radiation_flux: RSDR_s = RSDD_0
    if (0, 1, "RSDD") in A:
        for s in range(1, T + 1):
            if (s, 1, "RSDR") in A:
                put(s, 1, "RSDR", f(0, 1, "RSDD"))
    for g, n in normal:
        average(g, n)
    out = {k: A[k].copy() for k in case.outputs}
    for k, v in out.items():
        assert v.dtype == np.float32, k
    return out
