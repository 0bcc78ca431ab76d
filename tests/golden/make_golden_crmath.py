#!/usr/bin/env python
"""Generates tests/golden/crmath_cases.npz — arguments of csrc/liw_crmath.hpp's cr_sin / cr_cos / cr_atan2 with the correctly rounded
result of each, from mpmath at 500 bits (fixed seeds; the tests do not import mpmath).  Arrays, one entry per record:
  op uint8 (0 sin, 1 cos, 2 atan2(a, b)), a / b / want uint64 (the bit patterns of the doubles; b = 0 for ops 0 and 1),
  frac float64 = (exact - want) / ulp, in [-0.5, 0.5] (0 where the result is exact, infinite or NaN): a result `got` is
  |steps(got - want) - frac| ulp from the exact value, family uint8 (index into `families`);
and `families` (names), `dropped` (main-domain candidates left out because the exact value lies within 2^-40 ulp of a rounding
boundary, which no double-double evaluation can be asked to decide; the generator fails above 0.1 %).

Families.  Main domain (the header's own arithmetic answers; the bar is the correctly rounded result):
  uniform         sin and cos of x uniform in +-0.25, +-pi, +-1e3, +-2^20
  near_multiple   sin and cos of the doubles nearest k pi/2, |k| <= 8, and of their +-1 .. +-40 ulp neighbours, all enumerated (k = 0:
                  zero and the 40 smallest subnormals of either sign)
  big_multiple    sin and cos of the double nearest k pi/2, |k| <= 300 000
  quadrant_switch sin and cos within 2 ulp of (2 m + 1) pi/4, -8 <= m <= 7: where the reduction's n = rint(x 2/pi) changes
  tiny            sin of +-2^u, u uniform in [-1070, -20]
  edges           sin and cos at |x| = 0.25, 0.5 (the halvings' thresholds) and 2^20 (the domain's end) and one step either side
                  (the step above 2^20 is fallback_finite), at +-0, the largest subnormal and the smallest normal
  atan2_random    random direction, radius 2^+-30
  atan2_axis      within 2^-60 .. 2^-5 of the four axes
  atan2_scale     magnitudes 2^-1000 .. 2^990, signs free
  atan2_seam      the four axes with a signed zero, and the +-pi seam: s = +-tiny, c < 0
  atan2_guard     magnitudes on the inner side of cr_atan2's 1e+-300 guards
Fallback (the plain library function answers: host libm on the host, the device library on the device):
  fallback_finite  sin and cos of 2^20 < |x| <= 1e15, atan2 on the outer side of the 1e+-300 guards (want: correctly rounded)
  fallback_special sin / cos of +-inf and NaN, atan2(+-0, +-0), atan2 with an infinite or NaN argument (want: Python's math result)

Run in the build container only:  python tests/golden/make_golden_crmath.py
"""
import math
import os
import random
import struct
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "crmath_cases.npz")
SIN, COS, ATAN2 = 0, 1, 2
PREC = 500
DROP_BELOW = 2.0 ** -40   # ulp
FAMILIES = ["uniform", "near_multiple", "big_multiple", "quadrant_switch", "tiny", "edges", "atan2_random", "atan2_axis", "atan2_scale",
            "atan2_seam", "atan2_guard", "fallback_finite", "fallback_special"]
INF, NAN = float("inf"), float("nan")
TWO20 = 1048576.0


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(u):
    return struct.unpack("<d", struct.pack("<Q", int(u)))[0]


def step(x, k):
    """the double k steps above (k > 0) or below x"""
    for _ in range(abs(k)):
        x = math.nextafter(x, INF if k > 0 else -INF)
    return x


def atan2_in_main_domain(s, c):
    """cr_atan2's own guard: finite, below 1e300, not both zero, not both at most 1e-300"""
    return abs(s) < 1e300 and abs(c) < 1e300 and not (s == 0.0 and c == 0.0) and (abs(s) > 1e-300 or abs(c) > 1e-300)


# ---------------------------------------------------------------------------------------------------------------- the cases
def build_cases():
    """[(family, op, a, b)] in file order, before any drop; needs no mpmath"""
    out = []

    def sincos(fam, x):
        out.append((fam, SIN, x, 0.0))
        out.append((fam, COS, x, 0.0))

    rng = random.Random(20261)
    for lim in (0.25, math.pi, 1e3, TWO20):
        for _ in range(100):
            sincos("uniform", rng.uniform(-lim, lim))
    for k in range(-8, 9):
        for d in range(-40, 41):
            sincos("near_multiple", step(k * math.pi / 2, d))
    rng = random.Random(20262)
    for _ in range(250):
        sincos("big_multiple", rng.randint(-300000, 300000) * math.pi / 2)
    for m in range(-8, 8):
        for d in range(-2, 3):
            sincos("quadrant_switch", step((2 * m + 1) * math.pi / 4, d))
    rng = random.Random(20263)
    for _ in range(250):
        out.append(("tiny", SIN, rng.choice([-1.0, 1.0]) * 2.0 ** rng.uniform(-1070, -20), 0.0))
    for sgn in (1.0, -1.0):
        for x0 in (0.25, 0.5, TWO20):
            for d in (-1, 0, 1):
                x = sgn * step(x0, d)
                sincos("edges" if abs(x) <= TWO20 else "fallback_finite", x)
        for x in (0.0, 2.0 ** -1022 - 2.0 ** -1074, 2.0 ** -1022):
            sincos("edges", sgn * x)
    rng = random.Random(20264)
    for _ in range(250):
        t, r = rng.uniform(-math.pi, math.pi), 2.0 ** rng.uniform(-30, 30)
        out.append(("atan2_random", ATAN2, r * math.sin(t), r * math.cos(t)))
    for _ in range(250):
        t = rng.choice([0.0, math.pi / 2, math.pi, -math.pi / 2, -math.pi]) + rng.choice([-1, 1]) * 2.0 ** rng.uniform(-60, -5)
        out.append(("atan2_axis", ATAN2, math.sin(t), math.cos(t)))
    for _ in range(250):
        out.append(("atan2_scale", ATAN2, rng.choice([-1, 1]) * 2.0 ** rng.uniform(-1000, 990), rng.choice([-1, 1]) * 2.0 ** rng.uniform(-1000, 990)))
    for r in (1.0, 2.0 ** -30, 2.0 ** 30, 0.3):
        for z in (0.0, -0.0):
            out.extend([("atan2_seam", ATAN2, z, r), ("atan2_seam", ATAN2, z, -r), ("atan2_seam", ATAN2, r, z), ("atan2_seam", ATAN2, -r, z)])
        for tiny in (2.0 ** -1074, 2.0 ** -1022, 2.0 ** -600, 3e-300, 2.0 ** -80, 2.0 ** -53):
            for sgn in (1.0, -1.0):
                out.append(("atan2_seam", ATAN2, sgn * tiny, -r))
    # either side of the guards: |s|, |c| < 1e300, and not both <= 1e-300
    big = [step(1e300, -1), 1e300, step(1e300, 1), 1.6e308]
    small = [step(1e-300, -1), 1e-300, step(1e-300, 1)]
    for sb in (1.0, -1.0):
        for v in big:
            for other in (1.0, -0.37e300, step(1e300, -1), 2.0 ** -300):
                for s, c in ((sb * v, other), (other, sb * v)):
                    out.append(("atan2_guard" if atan2_in_main_domain(s, c) else "fallback_finite", ATAN2, s, c))
        for v in small:
            for other in (0.4e-300, -1e-300, step(1e-300, 1), 2.0 ** -1074, -(2.0 ** -1030), 0.0):
                for s, c in ((sb * v, other), (other, sb * v)):
                    out.append(("atan2_guard" if atan2_in_main_domain(s, c) else "fallback_finite", ATAN2, s, c))
    rng = random.Random(20265)
    for _ in range(100):
        sincos("fallback_finite", rng.choice([-1.0, 1.0]) * math.exp(rng.uniform(math.log(TWO20 * 1.0000001), math.log(1e15))))
    for x in (INF, -INF, NAN):
        sincos("fallback_special", x)
    for s in (0.0, -0.0):
        for c in (0.0, -0.0):
            out.append(("fallback_special", ATAN2, s, c))
    for s, c in ((INF, INF), (INF, -INF), (-INF, INF), (-INF, -INF), (INF, 1.0), (-INF, -2.5), (INF, 0.0), (1.0, INF), (-1.0, INF), (1.0, -INF),
                 (-1.0, -INF), (0.0, -INF), (-0.0, -INF), (0.0, INF), (-0.0, INF), (NAN, 1.0), (1.0, NAN), (NAN, NAN), (INF, NAN)):
        out.append(("fallback_special", ATAN2, s, c))
    for fam, op, a, b in out:   # every atan2 record sits in the family its guard sends it to
        if op == ATAN2 and fam not in ("fallback_special",):
            assert (fam != "fallback_finite") == atan2_in_main_domain(a, b), (fam, a, b)
    return out


# ------------------------------------------------------------------------------------------------------------ the reference
def exact(op, a, b):
    """the exact value as an mpf at PREC bits (finite arguments; atan2 of a zero first argument is taken for +0)"""
    import mpmath
    mpmath.mp.prec = PREC
    if op == SIN:
        return mpmath.sin(mpmath.mpf(a))
    if op == COS:
        return mpmath.cos(mpmath.mpf(a))
    return mpmath.atan2(mpmath.mpf(abs(a) if a == 0.0 else a), mpmath.mpf(b))


def round_nearest(v):
    """an mpf -> the nearest double, ties to even, subnormals included (Fraction -> float rounds once)"""
    sign, man, exp, _ = v._mpf_
    f = Fraction(int(man)) * (Fraction(2) ** int(exp))
    return float(-f if sign else f)


def record(op, a, b):
    """(want, frac, boundary distance in ulp) of one case with finite arguments that are not both zero"""
    import mpmath
    v = exact(op, a, b)
    want = round_nearest(v)
    if v == want:
        frac, dist = 0.0, 0.5
    else:
        toward = math.nextafter(want, INF if v > want else -INF)
        ulp = abs(mpmath.mpf(toward) - mpmath.mpf(want))
        frac = float((v - mpmath.mpf(want)) / ulp)
        dist = float(abs(v - (mpmath.mpf(toward) + mpmath.mpf(want)) / 2) / ulp)
    if op == ATAN2 and a == 0.0:   # mpmath has no signed zero: atan2(-0, c) = -atan2(+0, c)
        want, frac = math.copysign(want, a), math.copysign(frac, a) if frac else 0.0
    elif op == SIN and a == 0.0:
        want = a
    return want, frac, dist


def special(op, a, b):
    try:
        return [math.sin, math.cos][op](a) if op != ATAN2 else math.atan2(a, b)
    except ValueError:   # Python raises for sin / cos of an infinity; IEEE 754 says NaN
        return NAN


def main():
    cases = build_cases()
    rows, dropped, main_total, closest = [], 0, 0, 1.0
    for fam, op, a, b in cases:
        if fam == "fallback_special":
            rows.append((fam, op, a, b, special(op, a, b), 0.0))
            continue
        want, frac, dist = record(op, a, b)
        if fam != "fallback_finite":
            main_total += 1
            closest = min(closest, dist)
            if dist < DROP_BELOW:
                dropped += 1
                continue
        rows.append((fam, op, a, b, want, frac))
    print("%d candidates, %d in the main domain; dropped %d within 2^-40 ulp of a rounding boundary (closest kept or dropped: 2^%.1f ulp)"
          % (len(cases), main_total, dropped, math.log2(max(closest, 1e-300))))
    if dropped > 1e-3 * main_total:
        sys.exit("more than 0.1 % of the main-domain cases dropped")
    u64 = lambda col: np.array([bits(r[col]) for r in rows], dtype=np.uint64)
    np.savez_compressed(PATH, op=np.array([r[1] for r in rows], dtype=np.uint8), a=u64(2), b=u64(3), want=u64(4),
                        frac=np.array([r[5] for r in rows], dtype=np.float64), family=np.array([FAMILIES.index(r[0]) for r in rows], dtype=np.uint8),
                        families=np.array(FAMILIES), dropped=np.array(dropped, dtype=np.int64))
    for f in FAMILIES:
        print("  %-16s %5d" % (f, sum(1 for r in rows if r[0] == f)))
    print("wrote", PATH, len(rows), "records,", os.path.getsize(PATH), "bytes")
    assert os.path.getsize(PATH) <= 256 * 1024


if __name__ == "__main__":
    main()
