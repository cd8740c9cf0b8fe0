"""Parity metric of SURVEY.md 8d (fp64): per field
    max_j |x - x_ref| / max(|x_ref[j]|, 1e-6 * ||x_ref||_inf)  <=  1e-10
(mixed abs/rel, normalised per field: pure elementwise relative error is ill-posed where
q_s - q_a or T_s - T_a*EF cancel).  Integer/index results are compared bit-exactly.
Beside it, assert_tight (below) holds every fp64 output cell to a bit-exact, a seeded bit-exact
or a derived few-eps gate.
"""
import numpy as np

FP64_TOL = 1e-10
# fp32 variant ("fp32: report only").  Its error is reported against
# the fp64 oracle on the same (float32-rounded) inputs; the gate below is a sanity bound on
# the norm-wise error max|x - ref| / ||ref||_inf, not a parity claim.
FP32_NORM_GATE = 1e-5


def mixed_error(x, ref):
    x = np.asarray(x, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if x.shape != ref.shape:
        raise AssertionError(f"shape {x.shape} != {ref.shape}")
    if ref.size == 0:
        return 0.0
    if not np.all(np.isfinite(x) == np.isfinite(ref)):
        return np.inf
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    scale = np.maximum(np.abs(ref[fin]), 1e-6 * np.max(np.abs(ref[fin])))
    scale = np.where(scale == 0.0, 1.0, scale)
    return float(np.max(np.abs(x[fin] - ref[fin]) / scale))


def assert_parity(got: dict, ref: dict, tol=FP64_TOL, label=""):
    worst = {}
    for key, r in ref.items():
        e = mixed_error(got[key], r)
        worst[key] = e
    bad = {k: v for k, v in worst.items() if not v <= tol}
    assert not bad, f"{label}: fields over tolerance {tol}: {bad}; " + "; ".join(
        _where(got[k], ref[k], tol, k) for k in bad)
    return worst


def _where(x, ref, tol, key):
    """the failing cells of one field (count, first indices and values) for the message"""
    x = np.asarray(x, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    top = np.max(np.abs(ref[fin])) if fin.any() else 1.0
    scale = np.maximum(np.abs(ref), 1e-6 * top)
    with np.errstate(invalid="ignore"):
        off = ~(np.abs(x - ref) <= tol * np.where(scale == 0.0, 1.0, scale)) & ~(np.isnan(x) & np.isnan(ref))
    idx = np.nonzero(off)[0]
    return (f"{key}: {idx.size} of {x.size} cells, first {idx[:8].tolist()}, "
            f"got {x[idx[:4]].tolist()} want {ref[idx[:4]].tolist()}")


def norm_error(x, ref):
    """max_j |x - x_ref| / ||x_ref||_inf (norm-wise; the fp32 report)."""
    x = np.asarray(x, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    if not np.all(np.isfinite(x) == np.isfinite(ref)):
        return np.inf
    fin = np.isfinite(ref)
    top = np.max(np.abs(ref[fin])) if fin.any() else 0.0
    return float(np.max(np.abs(x[fin] - ref[fin])) / (top if top > 0 else 1.0))


def cell_report(got: dict, ref: dict):
    """Per field, over every cell: the mixed error (the gate), the plain elementwise max
    relative error, the counts of cells above 1e-10 by either measure, the bit-identical
    cells.  {"s:g:NAME": {...}}"""
    rep = {}
    for key, r in ref.items():
        g = np.asarray(got[key], dtype=np.float64)
        r = np.asarray(r, dtype=np.float64)
        fin = np.isfinite(r)
        top = float(np.max(np.abs(r[fin]))) if fin.any() else 0.0
        d = np.abs(g - r)
        nz = np.abs(r) > 0
        rel = np.zeros_like(r)
        np.divide(d, np.abs(r), out=rel, where=nz)
        rel[~nz & (d > 0)] = np.inf
        scale = np.maximum(np.abs(r), 1e-6 * top)
        mixed = np.divide(d, scale, out=np.zeros_like(r), where=scale > 0)
        rep["%d:%d:%s" % key] = {
            "cells": int(r.size), "mixed": mixed_error(g, r), "max_rel": float(rel.max(initial=0.0)),
            "cells_rel_gt_1e-10": int((rel > FP64_TOL).sum()),
            "cells_mixed_gt_1e-10": int((mixed > FP64_TOL).sum()),
            "bit_identical_cells": int((g == r).sum())}
    return rep


def write_report(name, rep):
    """gpurun_out/<name>.json (copied into profiles/ by the round's evidence scripts)."""
    import json
    import os

    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "parity")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, name + ".json"), "w") as f:
        json.dump(rep, f, indent=1)


def error_report(got: dict, ref: dict):
    """{field: (norm-wise error, mixed error, elementwise max relative error)}"""
    out = {}
    for key, r in ref.items():
        g = np.asarray(got[key], dtype=np.float64)
        r = np.asarray(r, dtype=np.float64)
        nz = np.abs(r) > 0
        rel = float(np.max(np.abs(g[nz] - r[nz]) / np.abs(r[nz]))) if nz.any() else 0.0
        out[key] = (norm_error(g, r), mixed_error(g, r), rel)
    return out


def sample_case(case, idx):
    """The case restricted to the cells idx (aliasing kept, the bias corrections sliced): for
    re-running the oracle on a few cells of a large grid.  u/v grids = t grid only."""
    from fcx.synthetic import build_case

    idx = np.asarray(idx)
    small = build_case(case.name.split("_")[0], n=idx.size, T=case.num_surface_types)
    remap = {}
    for key, a in case.lf.field.items():
        if id(a) not in remap:
            remap[id(a)] = np.ascontiguousarray(np.asarray(a)[idx])
        small.lf.field[key] = remap[id(a)]
    small.methods = {k: list(v) for k, v in case.methods.items()}
    if case.corrections is not None:
        init_date, corr = case.corrections
        corr = np.asarray(corr)
        small.corrections = (init_date, np.ascontiguousarray(corr[idx] if corr.shape[0] != 12 else corr[:, idx]))
    else:
        small.corrections = None
    return small


def conditioned_full(case, got, ref, t, label, tol=FP64_TOL, ulps=16, trials=8):
    """The SURVEY 8d gate over every cell, with the allowance of
    tests/test_gpu_random_configs.py::conditioned_parity for ill-conditioned cells: a cell
    over the gate (where HSEN = F c_p (T_s - T_a EF) or MEVA = F (q_s - q_a) cancel, one ulp of
    the device's pow / exp against the host libm's moves it by more than 1e-10 of its value)
    passes if the GPU is within twice the oracle's own movement when the cell's inputs are
    perturbed by `ulps` ulps (eight seeded perturbations, random signs per cell); any other
    error fails.  Returns {field: {"cells_over_gate", "max_err_over_movement"}}."""
    import oracle_lib

    bad = {}
    for key, r in ref.items():
        g = np.asarray(got[key], dtype=np.float64)
        r = np.asarray(r, dtype=np.float64)
        if not np.all(np.isfinite(g) == np.isfinite(r)):
            raise AssertionError(f"{label}: {key} finite/non-finite cells differ")
        fin = np.isfinite(r)
        top = float(np.max(np.abs(r[fin]))) if fin.any() else 0.0
        scale = np.maximum(np.abs(r), 1e-6 * top)
        with np.errstate(invalid="ignore", divide="ignore"):
            off = fin & (np.abs(g - r) > tol * np.where(scale == 0.0, 1.0, scale))
        if off.any():
            bad[key] = np.nonzero(off)[0]
    out = {"%d:%d:%s" % k: {"cells_over_gate": int(v.size)} for k, v in bad.items()}
    if not bad:
        return out
    idx = np.unique(np.concatenate(list(bad.values())))
    if idx.size > 10_000:
        raise AssertionError(f"{label}: {idx.size} cells over the gate")
    small = sample_case(case, idx)
    base = oracle_lib.run_case(small, "c", current_step_time=t)
    move = {k: np.zeros(idx.size) for k in bad}
    eps = float(np.finfo(np.float64).eps)
    for trial in range(trials):
        c = sample_case(case, idx)
        outs = {id(c.lf.field[k]) for k in c.outputs}
        rng = np.random.default_rng([trial, 99])
        seen = set()
        for a in c.lf.field.values():
            if id(a) in outs or id(a) in seen or not isinstance(a, np.ndarray) or a.dtype != np.float64:
                continue
            seen.add(id(a))
            a *= 1.0 + ulps * eps * rng.choice([-1.0, 1.0], a.shape)
        rp = oracle_lib.run_case(c, "c", current_step_time=t)
        for k in bad:
            move[k] = np.fmax(move[k], np.abs(np.asarray(rp[k]) - np.asarray(base[k])))
    pos = {int(j): i for i, j in enumerate(idx)}
    problems = []
    for k, cells in bad.items():
        sel = np.array([pos[int(j)] for j in cells])
        assert np.array_equal(np.asarray(base[k])[sel], np.asarray(ref[k])[cells]), (label, k, "oracle on the sample")
        err = np.abs(np.asarray(got[k])[cells] - np.asarray(ref[k])[cells])
        allow = 2.0 * move[k][sel]
        ratio = float(np.max(err / np.where(allow > 0, allow, np.inf))) if cells.size else 0.0
        out["%d:%d:%s" % k]["max_err_over_movement"] = ratio
        out["%d:%d:%s" % k]["cells"] = [int(x) for x in cells[:16]]
        if np.any(err > allow):
            problems.append(f"{k}: {int(np.sum(err > allow))} of {cells.size} cells over the gate are not explained "
                            f"by input rounding (first {cells[err > allow][:4].tolist()})")
    if problems:
        raise AssertionError(f"{label}: " + "; ".join(problems))
    return out


# --------------------------------------------------------------------------------------
# Tight fp64 gates: bit-exact, seeded-exact and derived-bound (beside the 1e-10 gate above)
# --------------------------------------------------------------------------------------
EPS = 2.0 ** -52
EXACT, SEEDED, BOUND, BUILT = "exact", "seeded-exact", "derived-bound", "construction"
QSUR_CAP = 8.0  # |d| <= 8 eps |ref|
HSEN_CAP = (4.0, 4.0)  # |d| <= 4 eps |F c_p T_a EF| + 4 eps |ref|
MEVA_RCO_CAP = (6.0, 4.0)  # |d| <= 6 eps |rho_a c_aw vel q_w| + 4 eps |ref|

_FLUX_TABLE = {"MEVA": "which_flux_mass_evap", "HLAT": "which_flux_heat_latent",
               "HSEN": "which_flux_heat_sensible", "UMOM": "which_flux_momentum",
               "VMOM": "which_flux_momentum", "RBBR": "which_flux_radiation_blackbody"}
_QSUR_TABLE = {1: "which_spec_vapor_surface_t", 2: "which_spec_vapor_surface_u",
               3: "which_spec_vapor_surface_v"}
# flux_constants.F90:13-32 and the RCO formulas' own constants (scale terms of the bounds only)
_CP, _LV, _LS, _RD, _RV, _UMIN = 1005.0, 2.501e6, 2.835e6, 287.05, 461.51, 0.01


def bits_equal(a, b):
    """Per cell: equal bit patterns through an int64 view (-0.0 != +0.0); NaN matches NaN
    whatever the payload, and never a number."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        raise AssertionError(f"shape {a.shape} != {b.shape}")
    na, nb = np.isnan(a), np.isnan(b)
    return (na & nb) | (~na & ~nb & (a.view(np.int64) == b.view(np.int64)))


def _method(case, s, g, name):
    """The method that computes (s, g, name); a 'copy' alias takes the method of the aliased
    type-1 field (prepare:36-38)."""
    table = _QSUR_TABLE[g] if name == "QSUR" else _FLUX_TABLE[name]
    m = case.methods[table][s - 1].rstrip()
    if m == "copy":
        m = case.methods[table][0].rstrip()
        if m == "copy":
            raise AssertionError(f"({s},{g},{name}): 'copy' of a 'copy'")
    return m


def _bias_additions(case, s):
    """How often calc:112-116 adds the bias to the MEVA array of type s: once per surface type
    whose MEVA slot is that array and whose method is not 'none'."""
    if case.corrections is None:
        return 0
    a = case.lf.field[(s, 1, "MEVA")]
    return sum(1 for i in range(1, case.num_surface_types + 1)
               if case.lf.field.get((i, 1, "MEVA")) is a
               and case.methods["which_flux_mass_evap"][i - 1].rstrip() != "none")


def gate_of(case, key):
    """The gate that holds the output field key = (s, g, name), from the case's method tables.
    Raises for a field that none of the gates covers."""
    s, g, name = key
    T = case.num_surface_types
    if s == 0:  # a type-0 average: as exact as the weakest of the per-type fields it sums
        if name == "TSUR":
            return EXACT
        parts = {gate_of(case, (i, g, name)) for i in range(1, T + 1)}
        if parts <= {EXACT}:
            return EXACT
        return SEEDED if parts <= {EXACT, SEEDED} else BUILT
    if name == "RSDR":
        return EXACT
    if name not in _FLUX_TABLE and name != "QSUR":
        raise AssertionError(f"{key}: no gate for this field")
    m = _method(case, s, g, name)
    if m == "zero":
        return EXACT
    if name == "RBBR" and m == "StBo":
        return EXACT
    if name == "QSUR" and m == "CCLM":
        return BOUND
    if name == "MEVA" and m in ("CCLM", "MOM5"):
        return SEEDED
    if name == "MEVA" and m == "RCO":
        if _bias_additions(case, s) > 1:
            raise AssertionError(f"{key}: RCO MEVA with the bias added more than once (a 'copy' alias) "
                                 "has no derived bound")
        return BOUND
    if name == "HLAT" and m in ("water", "ice"):
        return {EXACT: EXACT, SEEDED: SEEDED, BOUND: BUILT}[gate_of(case, (s, 1, "MEVA"))]
    if name == "HSEN" and m in ("CCLM", "MOM5"):
        return BOUND
    if name in ("HSEN", "UMOM", "VMOM") and m == "RCO":
        return EXACT
    if name in ("UMOM", "VMOM") and m in ("CCLM", "MOM5"):
        return SEEDED
    raise AssertionError(f"{key}: method {m!r} is in none of the gates")


def seeded_case(case, got):
    """The case with every which_spec_vapor_surface_{t,u,v} method 'none' and the QSUR arrays
    replaced by the device's own QSUR outputs (aliases kept: with shared grids the u and v
    slots are the t array, with separate grids each grid is seeded from its own array)."""
    import copy

    from fcx.local_field import LocalFields

    seeds = {id(case.lf.field[k]): np.array(got[k], dtype=np.float64, copy=True)
             for k in got if k[2] == "QSUR"}
    lf = LocalFields(case.lf.grid_size)
    lf.field = {k: (seeds.get(id(a), a) if k[2] == "QSUR" else a) for k, a in case.lf.field.items()}
    lf.allocated = set(case.lf.allocated)
    lf.put_to = dict(case.lf.put_to)
    new = copy.copy(case)
    new.lf = lf
    new.methods = {k: (["none"] * len(v) if k.startswith("which_spec_vapor_surface") else list(v))
                   for k, v in case.methods.items()}
    return new


def _host(a):
    return a if isinstance(a, np.ndarray) else a.detach().cpu().numpy()


def _bound_cap(case, key, ref, eps=EPS):
    """The per-cell cap of a derived-bound field, its scale term in numpy (float64) from the
    inputs; eps = the arithmetic's epsilon (2**-52, or 2**-23 for assert_tight_f32)."""
    s, g, name = key
    f = lambda v: np.asarray(_host(case.lf.field[(s, g, v)]), dtype=np.float64)  # noqa: E731
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    if name == "QSUR":
        return QSUR_CAP * eps * ref
    vel = np.sqrt(f("UATM") * f("UATM") + f("VATM") * f("VATM"))
    if name == "HSEN":
        a = f("AMOI" if _method(case, s, g, name) == "CCLM" else "CHEA")
        ps, ts = f("PSUR"), f("TSUR")
        rate = a * np.maximum(vel, _UMIN) * ps / (_RD * ts * (1.0 + (_RV / _RD - 1.0) * f("QATM")))
        ef = (ps / f("PATM")) ** (_RD / _CP)
        return HSEN_CAP[0] * eps * np.abs(rate * _CP * f("TATM") * ef) + HSEN_CAP[1] * eps * ref
    if name == "MEVA":
        ts = f("TSUR")
        q_w = 0.62197 * (6.1078E+02 * np.exp(17.269 * (ts - 273.15) / (ts - 35.86))) / 1.013E+05
        return MEVA_RCO_CAP[0] * eps * np.abs(1.225 * 1.15E-03 * vel * q_w) + MEVA_RCO_CAP[1] * eps * ref
    raise AssertionError(f"{key}: no derived bound")


def assert_tight(case, got, ref, t, label, report=True):
    """Every cell of every output of a fp64 case in one of three gates, each far inside the
    1e-10 gate, none using the perturbation allowance.  got = the device's outputs, ref = the
    plain oracle's (oracle_lib.run_case(case, "c", current_step_time=t)); case = the host case
    (for device-resident runs its host twin).  eps = 2**-52; "bit-identical" = equal int64
    views (-0.0 != +0.0), NaN cells equal NaN cells.

    The device and the oracle run the same IEEE operations in the same order except at three
    sites of fcx_physics.h: the exp of qsur_cclm, the exp of meva_rco and pow_exner =
    exp(y log x) against the oracle's pow.  Fields (by the case's method tables; a 'copy' alias
    is the aliased type-1 array and takes its class):

    exact         bit-identical to ref.  RBBR, RSDR, the TSUR average, HSEN/UMOM/VMOM of the RCO
                  method, every 'zero' method, the averages of these.
    seeded-exact  bit-identical to a second oracle run on seeded_case(): QSUR methods 'none',
                  QSUR = the device's own output.  MEVA/UMOM/VMOM of CCLM and MOM5, HLAT over
                  such a MEVA, their averages.  The bias (added once per aliased 'copy') is
                  reproduced by that run.
                  By construction, from the device's own values, for EVERY such field whatever
                  its class: HLAT == MEVA_dev * L (kLv 'water', kLs 'ice'), and every type-0
                  average == acc = 0; for s in type order: acc = acc + x_s * FARE_s in float64.
                  This is the only per-cell gate of HLAT over an RCO MEVA and of the averages
                  that sum a bounded field ("construction" in the report); it pins them exactly
                  given their bounded inputs.
    derived-bound per cell against ref, scale terms in numpy from the inputs:
                  QSUR (CCLM)       |d| <= 8 eps |ref|
                  HSEN (CCLM, MOM5) |d| <= 4 eps |F c_p T_a EF| + 4 eps |ref|
                  MEVA (RCO)        |d| <= 6 eps |rho_a c_aw vel q_w| + 4 eps |ref|

    Derivation of the caps.  ROCm documents 1 ulp for fp64 exp and log, glibc's exp and pow are
    within 1 ulp, and one ulp of x is at most eps |x|; so two results of exp on the same
    argument differ by at most 2 eps relative.  A rounded operation on both sides (each result
    within eps/2) adds at most eps to a relative difference; constants and inputs are the same
    bits on both sides.
      QSUR: e = p0 * exp(.) 3 eps; c e 4 eps; ps - c' e: c' e (4 eps) is at most 0.02 of the
        result (e < 5 kPa, ps > 90 kPa), 0.1 eps, plus its rounding 1.1 eps; the quotient
        4 + 1.1 + 1 = 6.1 eps.  Cap 8.
      HSEN: y log x with x = ps/pa in (1, 1.02): the 1.5-ulp error of the argument is below
        1e-2 eps absolute, so exp(y log x) is within 1.01 ulp of x**y and the oracle's pow
        within 1; EF lies in [1, 2), where an ulp is eps: 2.0 eps.  T_a EF 3.0 eps.  The
        difference T_s - T_a EF moves by 3.0 eps |T_a EF| and is rounded (eps of itself); the
        product with F c_p (same bits) adds eps: |d| <= 3.0 eps |F c_p T_a EF| + 2 eps |ref|
        (3.0 + 3 if F c_p is allowed a rounding of its own).  Caps 4 + 4.  F = a max(vel, u_min) p_s / (R_d T_s (1 + (R_v/R_d - 1) q_a)): the
        reference passes q_a for the surface humidity here (flux_calculator_calculate P3).
      MEVA (RCO): e_w = r exp(.) 3 eps; q_w = eps_c e_w / p_0 two operations, 5 eps;
        q_w - q_a moves by 5 eps |q_w| and is rounded; the product with rho_a c_aw vel and at
        most ONE bias addition round again: |d| <= 5 eps |K q_w| + 3 eps |ref| with K = rho_a
        c_aw vel.  Caps 6 + 4.  (The two roundings before the bias are relative to the value
        before it; they stay inside the caps while 2 |bias| <= |K q_w| + |ref|.  With the bias
        added twice, a 'copy' alias, there is no such bound: gate_of() refuses that case.)
    The caps are not fitted to any device output and are not to be raised for one.

    Returns {"s:g:NAME": {"gate", "cells", "bit_identical_share", "worst_ratio", "failed_cells"}}
    (bit_identical_share: against the seeded run for a seeded-exact field, else against ref;
    worst_ratio: |d| / cap of a bounded field; failed_cells: {gate: cells}, empty when green),
    writes it with write_report as ulp_gate_<label>.json (also when it fails), and raises an
    AssertionError that lists every failing field with its gate and cell count."""
    import oracle_lib

    assert set(got) == set(ref), f"{label}: outputs {sorted(set(got) ^ set(ref))} on one side only"
    gates = {k: gate_of(case, k) for k in ref}  # raises for an unclassified field
    assert set(gates) == set(case.outputs), f"{label}: fields of the case in no gate"
    dev = {id(case.lf.field[k]): np.asarray(got[k], dtype=np.float64) for k in got}
    value = lambda k: dev.get(id(case.lf.field[k]), _host(case.lf.field[k]))  # noqa: E731
    seeded = None
    if SEEDED in gates.values():
        seeded = oracle_lib.run_case(seeded_case(case, got), "c", current_step_time=t)
    out, problems = {}, []

    def fail(rec, key, gate, ok, what):
        idx = np.nonzero(~ok)[0]
        rec["failed_cells"][gate] = rec["failed_cells"].get(gate, 0) + int(idx.size)
        g = np.asarray(got[key])
        problems.append(f"{key} [{gate}] {what}: {idx.size} of {ok.size} cells, first {idx[:6].tolist()}, "
                        f"got {g[idx[:3]].tolist()}")

    for key, gate in gates.items():
        s, g, name = key
        x, r = np.asarray(got[key], dtype=np.float64), np.asarray(ref[key], dtype=np.float64)
        same = bits_equal(x, r)
        rec = {"gate": gate, "cells": int(x.size), "bit_identical_share": float(same.mean()) if x.size else 1.0,
               "worst_ratio": 0.0, "failed_cells": {}}
        covered = np.zeros(x.shape, dtype=bool)
        if gate == EXACT:
            covered[:] = True
            if not same.all():
                fail(rec, key, gate, same, "differs from the oracle")
        elif gate == SEEDED:
            covered[:] = True
            ok = bits_equal(x, seeded[key])
            rec["bit_identical_share"] = float(ok.mean()) if x.size else 1.0
            if not ok.all():
                fail(rec, key, gate, ok, "differs from the oracle seeded with the device's QSUR")
        elif gate == BOUND:
            covered[:] = True
            cap = _bound_cap(case, key, r)
            d = np.abs(x - r)
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(d == 0.0, 0.0, d / cap)
            ratio = np.where(np.isnan(x) & np.isnan(r), 0.0, ratio)
            ratio = np.where(np.isnan(ratio), np.inf, ratio)  # NaN on one side only
            ok = ratio <= 1.0
            rec["worst_ratio"] = float(ratio.max(initial=0.0))
            if not ok.all():
                fail(rec, key, gate, ok, f"over its cap (worst ratio {rec['worst_ratio']:.3g})")
        # by construction, from the device's own values
        if s >= 1 and name == "HLAT" and _method(case, s, g, name) in ("water", "ice"):
            covered[:] = True
            L = _LV if _method(case, s, g, name) == "water" else _LS
            ok = bits_equal(x, value((s, 1, "MEVA")) * L)
            if not ok.all():
                fail(rec, key, BUILT, ok, f"is not MEVA_dev * {L}")
        if s == 0:
            covered[:] = True
            acc = np.zeros(x.shape)
            for i in range(1, case.num_surface_types + 1):
                acc = acc + value((i, g, name)) * _host(case.lf.field[(i, g, "FARE")])
            ok = bits_equal(x, acc)
            if not ok.all():
                fail(rec, key, BUILT, ok, "is not the in-order sum of x_s * FARE_s of the device's x_s")
        assert covered.all(), f"{label}: {key} has cells in no gate"
        out["%d:%d:%s" % key] = rec
    if report:
        write_report("ulp_gate_" + "".join(c if c.isalnum() or c in "-_." else "_" for c in label), out)
    if problems:
        raise AssertionError(f"{label}: " + "; ".join(problems))
    return out


# --------------------------------------------------------------------------------------
# Tight gates of the plain fp32 engines (FCX_PRECISION_F32 without FCX_OPT_F32_MATH)
# --------------------------------------------------------------------------------------
EPS32 = 2.0 ** -23


def bits_equal32(a, b):
    """bits_equal for float32 arrays, through uint32 views (-0.0 != +0.0, NaN matches NaN)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32, (a.dtype, b.dtype)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        raise AssertionError(f"shape {a.shape} != {b.shape}")
    na, nb = np.isnan(a), np.isnan(b)
    return (na & nb) | (~na & ~nb & (a.view(np.uint32) == b.view(np.uint32)))


def assert_tight_f32(case32, got, t, label, report=True):
    """assert_tight for the plain fp32 engine: every cell of every output of an fp32 case
    (fcx.synthetic.as_dtype(case, "float32"); for device-resident runs its host twin) in one of the
    same gates, eps = eps32 = 2**-23.  The reference is not an oracle build but tests/f32_expect.py,
    the float32 restatement of fcx_physics.h at R = float and of the kernel's loop glue, pinned bit
    for bit to the header's host build by tests/test_f32_expect.py; its three transcendental sites
    take the CORRECTLY ROUNDED single exp and log (the double function rounded once).  got = the
    device's float32 outputs; classes from gate_of (it refuses what it refuses for fp64);
    "bit-identical" = equal uint32 views (-0.0 != +0.0), NaN cells equal NaN cells.

    exact         bit-identical to f32_expect.expected(case32, t).  RBBR, RSDR, the TSUR average,
                  HSEN/UMOM/VMOM of RCO, every 'zero', their averages.
    seeded-exact  bit-identical to expected(..., qsur = the device's own QSUR arrays).
                  MEVA/UMOM/VMOM of CCLM and MOM5, HLAT over such a MEVA, their averages.
    construction  from the device's own stored values, for EVERY such field whatever its class,
                  no tolerance: HLAT == MEVA_dev * float32(L), and every type-0 average ==
                  acc = float32(0); acc = acc + x_s * FARE_s in type order in float32.
    derived-bound per cell against expected() with the correctly rounded sites, the scale terms
                  in numpy float64 from the inputs, as assert_tight:
                  QSUR (CCLM)       |d| <= 8 eps32 |ref|
                  HSEN (CCLM, MOM5) |d| <= 4 eps32 |F c_p T_a EF| + 4 eps32 |ref|
                  MEVA (RCO)        |d| <= 6 eps32 |rho_a c_aw vel q_w| + 4 eps32 |ref|

    The caps are assert_tight's, and its derivation carries over unit for unit (eps -> eps32)
    under one ASSUMPTION: the device's single-precision exp and log are within 1 ulp.  That is the
    figure of the HIP math API's accuracy table for expf and logf; the ROCm installation this was
    written against carries neither that table nor a figure in its headers, so it is stated here
    and not cited from a file.  The reference side is better than assert_tight's (a correctly
    rounded site, 0.5 ulp, where glibc's is within 1), so two site results differ by at most
    1.5 eps32 relative, inside the 2 eps the derivation uses.  Its one side condition, "the error
    of pow_exner's argument y log x is below 1e-2 eps absolute", holds in float32: x = ps/pa in
    (1, 1.02) gives log x < 0.02, whose ulp is 2^-29 = 1.9e-9; two logs within 1 ulp differ by
    that, times y = 0.2856: 5.3e-10, and the product's rounding (|y log x| < 0.0057, ulp 4.7e-10)
    can move it by one more ulp: 1.0e-9 < 1e-2 eps32 = 1.2e-9.  The caps are never fitted to a
    device output; the measured worst ratios go into the report.

    Returns and writes (f32_gate_<label>.json, also when it fails) the report of assert_tight and
    raises an AssertionError that lists every failing field with its gate and cell count."""
    import f32_expect

    assert set(got) == set(case32.outputs), f"{label}: outputs {sorted(set(got) ^ set(case32.outputs))} on one side only"
    gates = {k: gate_of(case32, k) for k in case32.outputs}  # raises for an unclassified field
    for k, v in got.items():
        assert np.asarray(v).dtype == np.float32, f"{label}: {k} is {np.asarray(v).dtype}, not the device's float32"
    expect = f32_expect.expected
    ref = expect(case32, t)
    dev = {id(case32.lf.field[k]): np.asarray(got[k]) for k in got}

    def value(k):
        v = dev.get(id(case32.lf.field[k]))
        v = np.asarray(_host(case32.lf.field[k])) if v is None else v
        assert v.dtype == np.float32, (k, v.dtype)
        return v

    seeded = None
    if SEEDED in gates.values():
        seeded = expect(case32, t, qsur={k: got[k] for k in got if k[2] == "QSUR"})
    out, problems = {}, []

    def fail(rec, key, gate, ok, what):
        idx = np.nonzero(~ok)[0]
        rec["failed_cells"][gate] = rec["failed_cells"].get(gate, 0) + int(idx.size)
        g = np.asarray(got[key])
        problems.append(f"{key} [{gate}] {what}: {idx.size} of {ok.size} cells, first {idx[:6].tolist()}, "
                        f"got {g[idx[:3]].tolist()}")

    for key, gate in gates.items():
        s, g, name = key
        x, r = np.asarray(got[key]), ref[key]
        same = bits_equal32(x, r)
        rec = {"gate": gate, "cells": int(x.size), "bit_identical_share": float(same.mean()) if x.size else 1.0,
               "worst_ratio": 0.0, "failed_cells": {}}
        covered = np.zeros(x.shape, dtype=bool)
        if gate == EXACT:
            covered[:] = True
            if not same.all():
                fail(rec, key, gate, same, "differs from the float32 restatement")
        elif gate == SEEDED:
            covered[:] = True
            ok = bits_equal32(x, seeded[key])
            rec["bit_identical_share"] = float(ok.mean()) if x.size else 1.0
            if not ok.all():
                fail(rec, key, gate, ok, "differs from the float32 restatement seeded with the device's QSUR")
        elif gate == BOUND:
            covered[:] = True
            x64, r64 = x.astype(np.float64), r.astype(np.float64)
            cap = _bound_cap(case32, key, r64, eps=EPS32)
            d = np.abs(x64 - r64)
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(d == 0.0, 0.0, d / cap)
            ratio = np.where(np.isnan(x64) & np.isnan(r64), 0.0, ratio)
            ratio = np.where(np.isnan(ratio), np.inf, ratio)  # NaN on one side only
            ok = ratio <= 1.0
            rec["worst_ratio"] = float(ratio.max(initial=0.0))
            if not ok.all():
                fail(rec, key, gate, ok, f"over its cap (worst ratio {rec['worst_ratio']:.3g})")
        # by construction, from the device's own values, in float32
        if s >= 1 and name == "HLAT" and _method(case32, s, g, name) in ("water", "ice"):
            covered[:] = True
            L = np.float32(_LV if _method(case32, s, g, name) == "water" else _LS)
            built = value((s, 1, "MEVA")) * L
            ok = bits_equal32(x, built)
            if not ok.all():
                fail(rec, key, BUILT, ok, f"is not MEVA_dev * float32({L})")
        if s == 0:
            covered[:] = True
            acc = np.zeros(x.shape, np.float32)
            for i in range(1, case32.num_surface_types + 1):
                acc = acc + value((i, g, name)) * np.asarray(_host(case32.lf.field[(i, g, "FARE")]))
            ok = bits_equal32(x, acc)
            if not ok.all():
                fail(rec, key, BUILT, ok, "is not the in-order float32 sum of x_s * FARE_s of the device's x_s")
        assert covered.all(), f"{label}: {key} has cells in no gate"
        out["%d:%d:%s" % key] = rec
    if report:
        write_report("f32_gate_" + "".join(c if c.isalnum() or c in "-_." else "_" for c in label), out)
    if problems:
        raise AssertionError(f"{label}: " + "; ".join(problems))
    return out
