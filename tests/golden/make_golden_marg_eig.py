#!/usr/bin/env python
"""Generates tests/golden/marg_eig_cases.npz — the hostile 15 x 15 spectra of tests/marg_eig_cases.py with their eigenpairs from
mpmath.eigsy at 60 digits, the sweep count and the error figures of the float64 restatement of the kernels' algorithm, and the bars the
GPU test holds the device to (16 x the restatement's worst figure per measure, at least 64 u).  float64 arrays only; layout in the
docstring of tests/marg_eig_cases.py.  The tests do not need mpmath.

The generator asserts the conditions the tests rely on: no floor decision hangs on round-off (every exact eigenvalue at least
1e3 u |A|max away from 1e-8, but in the two exact cases), the exact cases take zero sweeps, the restatement meets every assertion of
the GPU test, and it runs into the 60-sweep cap on rank8 and rank1.

Run in the build container only:  python tests/golden/make_golden_marg_eig.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import marg_eig_cases as mc  # noqa: E402

DIGITS = 60


def eigsy(dH):
    """(lam ascending, vec rows rounded to double with the largest |component| positive) of (dH + dH^T) / 2 at DIGITS digits"""
    import mpmath
    mpmath.mp.dps = DIGITS
    if not np.any(dH):
        return np.zeros(15), np.eye(15)
    M = mpmath.matrix(15, 15)
    for r in range(15):
        for c in range(15):
            M[r, c] = (mpmath.mpf(float(dH[r, c])) + mpmath.mpf(float(dH[c, r]))) / 2
    E, Q = mpmath.eigsy(M)
    order = sorted(range(15), key=lambda k: E[k])
    lam = np.array([float(E[k]) for k in order])
    vec = np.array([[float(Q[r, k]) for r in range(15)] for k in order])
    for k in range(15):
        if vec[k, np.argmax(np.abs(vec[k]))] < 0.0:
            vec[k] = -vec[k]
    return lam, vec


def main():
    cases = mc.build_cases()
    assert [c[0] for c in cases] == mc.NAMES
    N = len(cases)
    dH, dg = np.array([c[1] for c in cases]), np.array([c[2] for c in cases])
    lam, vec, sweeps, vals = np.zeros((N, 15)), np.zeros((N, 15, 15)), np.zeros(N), np.full((N, len(mc.MEASURES)), np.nan)
    figs = []
    for i, (name, H, g) in enumerate(cases):
        lam[i], vec[i] = eigsy(H)
        J, R, sweeps[i] = mc.restate(H, g)
        amax = np.abs(0.5 * (H + H.T)).max()
        if name in mc.EXACT:
            assert sweeps[i] == 0, name
        else:
            mc.assert_floor_margin(name, H, lam[i])
        fig = mc.measures(name, H, g, lam[i], vec[i], J, R)
        figs.append(fig)
        vals[i] = [fig[m] for m in mc.MEASURES]
        print("%-14s sweeps %2d kept %2d  " % (name, sweeps[i], mc.kept_of(lam[i]).sum())
              + "  ".join("%s %.1e" % (m, fig[m]) for m in mc.MEASURES + ["eig_rel"]) + ("  exact %.1f ulp" % fig["exact_ulp"] if "exact_ulp" in fig else ""))
    for name in ("rank8", "rank1"):
        assert sweeps[mc.case_index(name)] == mc.SWEEP_CAP, name
    i, j = mc.case_index("skew"), mc.case_index("skew_sym")
    assert np.array_equal(0.5 * (dH[i] + dH[i].T), dH[j]) and not np.array_equal(dH[i], dH[i].T) and np.array_equal(dg[i], dg[j])
    bars = mc.bars_from(vals)
    for i, name in enumerate(mc.NAMES):
        mc.check_bars(name, figs[i], bars)
    print("bars: " + "  ".join("%s %.2e" % (m, b) for m, b in zip(mc.MEASURES, bars)))
    np.savez_compressed(mc.PATH, dH=dH, dg=dg, lam=lam, vec=vec, sweeps=sweeps, restate=vals, bars=bars)
    print("wrote", mc.PATH, os.path.getsize(mc.PATH), "bytes")
    assert os.path.getsize(mc.PATH) < 150 * 1000


if __name__ == "__main__":
    main()
