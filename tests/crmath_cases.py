"""The fixture tests/golden/crmath_cases.npz (tests/golden/make_golden_crmath.py: arguments of csrc/liw_crmath.hpp's functions with
their correctly rounded results from a 500-bit reference) and the conditions tests/test_crmath.py (the host compile of the header)
and tests/test_gpu_crmath.py (the device compile) both put on a build's results.

A helper module, not a conftest."""
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "crmath_cases.npz")
SIN, COS, ATAN2 = 0, 1, 2
EXP_MASK, SIGN = np.uint64(0x7FF0000000000000), np.uint64(1 << 63)
TINY_ATAN2 = 2.0 ** -969   # below it the low word of cr_atan2's double-double quotient is subnormal: within an ulp, not correctly rounded

_cache = {}


def load():
    """dict(op, a, b, want uint64 bit patterns, frac, family (names per record), families, dropped), loaded once and read-only"""
    if not _cache:
        with np.load(PATH) as z:
            d = {k: z[k] for k in ("op", "a", "b", "want", "frac")}
            names = [str(s) for s in z["families"]]
            d["family"] = np.array(names)[z["family"]]
            d["families"], d["dropped"] = names, int(z["dropped"])
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache.update(d)
    return _cache


def f64(u):
    return np.ascontiguousarray(u, dtype=np.uint64).view(np.float64)


def u64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def ordinal(u):
    """bit patterns of finite doubles -> integers in the order of the doubles, one apart for neighbours (-0 and +0 both 0)"""
    u = np.asarray(u, dtype=np.uint64)
    mag = (u & ~SIGN).astype(np.int64)
    return np.where((u & SIGN) != 0, -mag, mag)


def ulp_error(got, want, frac):
    """|got - exact| in ulp of the correctly rounded `want`, from the fixture's frac = (exact - want) / ulp"""
    return np.abs((ordinal(got) - ordinal(want)).astype(np.float64) - frac)


def is_nan(u):
    u = np.asarray(u, dtype=np.uint64)
    return ((u & EXP_MASK) == EXP_MASK) & ((u & np.uint64(0x000FFFFFFFFFFFFF)) != 0)


def main_domain_failures(d, got, sel):
    """indices among sel (a boolean mask over the records of a main-domain family) whose result misses its bar: the bits of the
    correctly rounded result — except where an atan2 result is below 2^-969 in magnitude: there strictly under 1 ulp from the
    exact value."""
    idx = np.nonzero(sel)[0]
    want, g = d["want"][idx], np.asarray(got, dtype=np.uint64)[idx]
    ok = g == want
    loose = (d["op"][idx] == ATAN2) & (np.abs(f64(want)) < TINY_ATAN2)
    with np.errstate(invalid="ignore"):
        near = ~is_nan(g) & (ulp_error(g, want, d["frac"][idx]) < 1.0) & ((g & SIGN) == (want & SIGN))
    return idx[~(ok | (loose & near))]


def special_failures(d, got, sel):
    """fallback_special records whose result is not what IEEE 754 / C Annex F ask of the plain functions: NaN in gives NaN out, sin and
    cos of an infinity are NaN, atan2 of zeros and of infinite arguments are exactly Python's math.atan2 (the fixture's value)"""
    bad = []
    for i in np.nonzero(sel)[0]:
        want, g = int(d["want"][i]), int(np.asarray(got, dtype=np.uint64)[i])
        if is_nan(np.uint64(want)):
            if not is_nan(np.uint64(g)):
                bad.append(i)
        elif g != want:
            bad.append(i)
    return np.array(bad, dtype=np.int64)


def describe(d, got, idx, limit=6):
    rows = []
    for i in list(idx)[:limit]:
        a, b, w, g = (float(f64(np.uint64(v))) for v in (d["a"][i], d["b"][i], d["want"][i], np.asarray(got, dtype=np.uint64)[i]))
        rows.append("%s(%s%s) = %s, correctly rounded %s" % (("sin", "cos", "atan2")[int(d["op"][i])], a.hex(), ", " + b.hex() if d["op"][i] == ATAN2 else "",
                                                              g.hex(), w.hex()))
    return "%d records, e.g. %s" % (len(idx), "; ".join(rows))


def host_build(tmpdir):
    """compile tests/cpp/crmath_driver.cpp against the header as the library's host code is compiled (no contraction) -> run(op, a, b
    uint64 arrays) -> uint64 results"""
    src = os.path.join(ROOT, "tests", "cpp", "crmath_driver.cpp")
    exe = os.path.join(str(tmpdir), "crmath_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", exe])

    def run(op, a, b):
        text = "".join("%d %x %x\n" % (int(o), int(x), int(y)) for o, x, y in zip(op, a, b))
        r = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
        out = r.stdout.split()
        assert len(out) == len(op), r.stderr
        return np.array([int(v, 16) for v in out], dtype=np.uint64)
    return run


def sin_of_pi_and_cos_of_half_pi():
    """two values known from the literature, independent of the generator: sin(fl(pi)) = pi - fl(pi) and cos(fl(pi/2)) = pi/2 - fl(pi/2)
    to second order, i.e. the second word of pi (pi/2) in double-double: 0x1.1a62633145c07p-53 (p-54)"""
    return [(SIN, math.pi, float.fromhex("0x1.1a62633145c07p-53")), (COS, math.pi / 2, float.fromhex("0x1.1a62633145c07p-54")),
            (SIN, -math.pi, float.fromhex("-0x1.1a62633145c07p-53")), (COS, -math.pi / 2, float.fromhex("0x1.1a62633145c07p-54"))]
