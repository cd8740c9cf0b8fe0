#!/usr/bin/env python3
"""Writes tests/golden/cr_math.npz: correctly rounded values of the three transcendental sites
of the fp64 engine (csrc/fcx_physics.h), for tests of FCX_OPT_CR_MATH.

The file is a table of CELLS.  A cell holds the inputs of all three sites (TSUR, FICE, PSUR,
PATM), so that a test can write the table into a synthetic case and know the correctly rounded
site value of every cell; per site it holds the argument the formula forms from the inputs in
double (the reference's operation order) and the correctly rounded result for that argument,
from a 300-bit mpmath evaluation:

  tsur, fice, psur, patm                 inputs (float64)
  qsur_arg, qsur_res                     alpha (ts - t1) / (ts - t2),      RN(exp(arg))
  rco_arg,  rco_res                      c_1 (ts - 273.15) / (ts - c_2),   RN(exp(arg))
  exner_x,  exner_y (scalar), exner_res  ps / pa, R_d / c_p,               RN(x ** y)
  qsur_libm_ok, rco_libm_ok, exner_libm_ok   whether the generating machine's math.exp /
                                         math.pow returned that value (for reference only)
  kind                                   bits: 1 the cell is a hard case of QSUR, 2 of RCO MEVA,
                                         4 of the Exner power; a site whose bit is clear has
                                         an ordinary draw there (the ranges of fcx/synthetic.py)
  qsur_dist, rco_dist, exner_dist        float32; for a hard case of the site: distance of the
                                         exact result from the nearest rounding midpoint, in
                                         ulps (NaN elsewhere)

Hard cases: --draws (default 10**7) random inputs per site from the site's physical range,
screened at 128 bits; those whose exact result lies nearest a midpoint between two doubles are
kept: --hard (default 1000) for QSUR and for RCO MEVA, and twice as many for the Exner power.
An evaluation with an error above that distance cannot round them without more precision.
The temperature sites share TSUR, so a cell is hard for one of them; the Exner power reads
PSUR and PATM only, so every hard temperature cell is a hard Exner cell too.  That is how a
thousand hard cases per site and 1,680 cells that are ordinary for every site (2,680 that are
ordinary for a temperature site) fit the 300 KB a fixture may take, at ten float64 columns per
cell.  The cells are shuffled, so any slice of the table mixes the kinds.

Needs mpmath; run on a development machine only.  Tests read the file, never mpmath.
"""
import argparse
import math
import multiprocessing as mpc
import os
import sys

import numpy as np
from mpmath import libmp, mp, mpf

SEED = 20231015
CHUNK = 100000
SCREEN_PREC = 128
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "golden", "cr_math.npz")

K_RD, K_CP = 287.05, 1005.0
EXNER_Y = K_RD / K_CP


def qsur_arg(ts, fice):
    aw, ai, t1, t2w, t2i = 17.2693882, 21.8745584, 273.16, 35.86, 7.66
    alpha = aw + (ai - aw) * fice
    t2 = t2w + (t2i - t2w) * fice
    return alpha * (ts - t1) / (ts - t2)


def rco_arg(ts):
    return 17.269 * (ts - 273.15) / (ts - 35.86)


def draw_bottom(r, n, physical):
    """TSUR, FICE.  ordinary: fcx/synthetic.py bottom_fields; physical: fractional ice too."""
    u = r.random(n)
    if physical:
        fice = np.where(u < 0.6, 0.0, np.where(u < 0.8, 1.0, r.random(n)))
    else:
        fice = (u < 0.2).astype(np.float64)
    ts = np.where(fice == 0.0, r.uniform(271.0, 303.0, n),
                  np.where(fice == 1.0, r.uniform(255.0, 273.15, n), r.uniform(255.0, 290.0, n)))
    return ts, fice


def draw_pressure(r, n):
    ps = r.uniform(95000.0, 105000.0, n)
    return ps, ps - r.uniform(50.0, 1500.0, n)


def midpoint_dist(v):
    """ulps between the mpf tuple v and the nearest midpoint of two 53-bit numbers."""
    man, bc = v[1], v[3]
    sh = bc - 53
    if sh <= 0:
        return 0.5
    rem = man & ((1 << sh) - 1)
    return abs(rem - (1 << (sh - 1))) / (1 << sh)


def screen(job):
    site, chunk, keep = job
    r = np.random.Generator(np.random.PCG64([SEED, 100 + site, chunk]))
    if site == 1:
        ts, fice = draw_bottom(r, CHUNK, True)
        arg = qsur_arg(ts, fice)
        d = [midpoint_dist(libmp.mpf_exp(libmp.from_float(float(a)), SCREEN_PREC, "n")) for a in arg]
        cols = (ts, fice)
    elif site == 2:
        ts = r.uniform(255.0, 303.0, CHUNK)
        arg = rco_arg(ts)
        d = [midpoint_dist(libmp.mpf_exp(libmp.from_float(float(a)), SCREEN_PREC, "n")) for a in arg]
        cols = (ts,)
    else:
        ps, pa = draw_pressure(r, CHUNK)
        x = ps / pa
        y = libmp.from_float(EXNER_Y)
        d = [midpoint_dist(libmp.mpf_pow(libmp.from_float(float(a)), y, SCREEN_PREC, "n")) for a in x]
        cols = (ps, pa)
    d = np.array(d)
    idx = np.argsort(d, kind="stable")[:keep]
    return d[idx], tuple(c[idx] for c in cols)


def hard_cases(pool, site, draws, keep):
    jobs = [(site, c, keep) for c in range((draws + CHUNK - 1) // CHUNK)]
    ds, cols = [], None
    for d, c in pool.imap(screen, jobs):
        ds.append(d)
        cols = [[x] for x in c] if cols is None else [a + [x] for a, x in zip(cols, c)]
    d = np.concatenate(ds)
    cols = [np.concatenate(c) for c in cols]
    idx = np.argsort(d, kind="stable")[:keep]
    return d[idx], [c[idx] for c in cols]


def rn_exp(a):
    return np.array([float(mp.exp(mpf(float(x)))) for x in a])


def rn_pow(x, y):
    return np.array([float(mp.power(mpf(float(a)), mpf(y))) for a in x])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--draws", type=int, default=10**7)
    ap.add_argument("--hard", type=int, default=1000)
    ap.add_argument("--ordinary", type=int, default=1680)
    ap.add_argument("--procs", type=int, default=os.cpu_count() or 1)
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    mp.prec = 300
    with mpc.Pool(a.procs) as pool:
        hard = {s: hard_cases(pool, s, a.draws, a.hard * (2 if s == 3 else 1)) for s in (1, 2, 3)}
    for s in (1, 2, 3):
        d = hard[s][0]
        print("site %d: %d draws, kept %d, midpoint distance %.3g .. %.3g ulp" % (s, a.draws, len(d), d[0], d[-1]))
    n = 2 * a.hard + a.ordinary
    r = np.random.Generator(np.random.PCG64([SEED, 99]))
    ts, fice = draw_bottom(r, n, False)
    ps, pa = draw_pressure(r, n)
    kind = np.zeros(n, np.uint8)
    dq, dr, de = (np.full(n, np.nan, np.float32) for _ in range(3))
    h = a.hard
    ts[0:h], fice[0:h] = hard[1][1]
    kind[0:h], dq[0:h] = 1, hard[1][0]
    # a hard RCO cell keeps its TSUR; its FICE follows the temperature as in synthetic.py
    ts[h:2 * h] = hard[2][1][0]
    fice[h:2 * h] = (ts[h:2 * h] < 271.0).astype(np.float64)
    kind[h:2 * h], dr[h:2 * h] = 2, hard[2][0]
    # the hard Exner pairs, dealt over the hard temperature cells in a shuffled order (the
    # nearest ones not all with QSUR's)
    deal = r.permutation(2 * h)
    ps[0:2 * h], pa[0:2 * h] = hard[3][1][0][deal], hard[3][1][1][deal]
    kind[0:2 * h] |= 4
    de[0:2 * h] = hard[3][0][deal]
    order = r.permutation(n)
    ts, fice, ps, pa, kind, dq, dr, de = (x[order] for x in (ts, fice, ps, pa, kind, dq, dr, de))
    qa, ra, ex = qsur_arg(ts, fice), rco_arg(ts), ps / pa
    qr, rr, er = rn_exp(qa), rn_exp(ra), rn_pow(ex, EXNER_Y)
    q_ok = np.array([math.exp(x) for x in qa]) == qr
    r_ok = np.array([math.exp(x) for x in ra]) == rr
    e_ok = np.array([math.pow(x, EXNER_Y) for x in ex]) == er
    for name, ok in (("QSUR exp", q_ok), ("RCO exp", r_ok), ("Exner pow", e_ok)):
        print("%s: libm correctly rounded in all but %d of %d cells" % (name, int((~ok).sum()), n))
    np.savez_compressed(a.out, tsur=ts, fice=fice, psur=ps, patm=pa, qsur_arg=qa, qsur_res=qr, rco_arg=ra,
                        rco_res=rr, exner_x=ex, exner_y=np.float64(EXNER_Y), exner_res=er, qsur_libm_ok=q_ok,
                        rco_libm_ok=r_ok, exner_libm_ok=e_ok, kind=kind, qsur_dist=dq, rco_dist=dr, exner_dist=de)
    print("wrote %s: %d cells, %d bytes" % (os.path.normpath(a.out), n, os.path.getsize(a.out)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
