// liw_crmath.hpp — sin, cos and atan2 of a double evaluated in double-double arithmetic and rounded once, for device code whose
// results are compared with the host's libm bit for bit where that is possible: the device library's sin / cos / atan2 are off by
// up to an ulp or two, glibc's by at most 0.55 ulp, so the correctly rounded value is what glibc returns in all but a fraction of
// a per cent of the arguments.  Used by the tracking glue (k_lfe_track_begin): a last-bit difference in the de-skew twist or the
// predicted pose is amplified by every free-running solve that follows.
//   sincos_dd: x - n pi/2 with n = rint(x 2/pi) and pi/2 carried as four doubles, as a double-double r, |r| <= pi/4: the
//   products n P_i are error-free, the terms down to 2^-53 |x| are summed exactly and what is left, below 2^-105 |x|, is added in
//   double-double: the absolute error of r is about 2^-209 |x| <= 2^-189, while no double at all is closer than 2^-62 to a
//   multiple of pi/2 (the known worst case of this reduction), so r keeps its 2^-104 relative error however close x comes to one.
//   Then r is halved at most twice to |r| <= 0.25, the Taylor series runs to r^27 in double-double, the halvings are undone by
//   double-angle steps (the cosine stays above 0.7 there: no cancellation) and n & 3 picks the quadrant.  The relative error of
//   the sine and of the cosine is below 2^-98 everywhere, which a rounding to 53 bits cannot see unless the exact value lies within
//   2^-45 ulp of a rounding boundary.  Arguments beyond 2^20, infinities and NaN go to the plain functions.
//   cr_atan2: one Newton correction of the plain atan2 with the double-double sine and cosine of that estimate:
//   y + (s C - c S) / (c C + s S).  Where |result| < 2^-969 the low word of the quotient is subnormal and the result is within an
//   ulp, not correctly rounded.
// Tested on the host and on the device against a 500-bit reference (tests/test_crmath.py, tests/test_gpu_crmath.py).
// fma() is called explicitly (error-free products); the translation unit may have contraction off.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define LIW_CR_HD __host__ __device__
#else
#define LIW_CR_HD
#endif

namespace liw_cr {

struct DD { double h, l; };

LIW_CR_HD inline DD two_sum(double a, double b) { const double s = a + b, bb = s - a; return DD{s, (a - (s - bb)) + (b - bb)}; }
LIW_CR_HD inline DD quick_two_sum(double a, double b) { const double s = a + b; return DD{s, b - (s - a)}; }
LIW_CR_HD inline DD two_prod(double a, double b) { const double p = a * b; return DD{p, fma(a, b, -p)}; }
LIW_CR_HD inline DD add(const DD& a, const DD& b) {
    DD s = two_sum(a.h, b.h);
    const DD t = two_sum(a.l, b.l);
    s.l += t.h;
    s = quick_two_sum(s.h, s.l);
    s.l += t.l;
    return quick_two_sum(s.h, s.l);
}
LIW_CR_HD inline DD neg(const DD& a) { return DD{-a.h, -a.l}; }
LIW_CR_HD inline DD sub(const DD& a, const DD& b) { return add(a, neg(b)); }
LIW_CR_HD inline DD mul(const DD& a, const DD& b) {
    DD p = two_prod(a.h, b.h);
    p.l += a.h * b.l + a.l * b.h;
    return quick_two_sum(p.h, p.l);
}
LIW_CR_HD inline DD mul_d(const DD& a, double b) {
    DD p = two_prod(a.h, b);
    p.l += a.l * b;
    return quick_two_sum(p.h, p.l);
}
LIW_CR_HD inline DD div(const DD& a, const DD& b) {   // three quotient digits
    const double q1 = a.h / b.h;
    DD r = sub(a, mul_d(b, q1));
    const double q2 = r.h / b.h;
    r = sub(r, mul_d(b, q2));
    const double q3 = r.h / b.h;
    const DD q = quick_two_sum(q1, q2);
    return add(q, DD{q3, 0.0});
}
LIW_CR_HD inline DD div_d(const DD& a, double b) { return div(a, DD{b, 0.0}); }

// double-double sine and cosine of the double x, |x| <= 2^20
LIW_CR_HD inline void sincos_dd(double x, DD& s, DD& c) {
    // pi/2 = P0 + P1 + P2 + P3 to 2^-218; n < 2^20: what is missing from n pi/2 is below 2^-197
    const double P0 = 0x1.921fb54442d18p+0, P1 = 0x1.1a62633145c07p-54, P2 = -0x1.f1976b7ed8fbcp-110, P3 = 0x1.4cf98e804177dp-164;
    const double n = rint(x * 0x1.45f306dc9c883p-1);
    DD r = DD{x, 0.0};
    if (n != 0.0) {
        const DD a0 = two_prod(n, P0), a1 = two_prod(n, P1), a2 = two_prod(n, P2);
        const double t = x - a0.h;                        // exact (Sterbenz): a0.h / 2 <= x <= 2 a0.h for every n != 0
        const DD u = two_sum(-a0.l, -a1.h);               // the two terms of order 2^-53 |x|, exactly
        const DD v = two_sum(t, u.h);                     // v.h + v.l + u.l = x - n (P0 + P1) + a1.l exactly
        DD w = add(two_sum(v.l, u.l), two_sum(-a1.l, -a2.h));   // all below 2^-105 |x|: double-double is 2^-209 |x| here
        w = add(w, two_sum(-a2.l, -(n * P3)));
        r = add(DD{v.h, 0.0}, w);
    }
    int k = 0;
    while (fabs(r.h) > 0.25) { r.h *= 0.5; r.l *= 0.5; ++k; }   // exact, at most twice
    const DD r2 = mul(r, r);
    DD ts = r, tc = DD{1.0, 0.0};
    DD ss = r, cc = tc;
#pragma unroll 1
    for (int i = 1; i <= 13; ++i) {
        tc = neg(div_d(mul(tc, r2), (double)((2 * i - 1) * (2 * i))));
        ts = neg(div_d(mul(ts, r2), (double)((2 * i) * (2 * i + 1))));
        cc = add(cc, tc);
        ss = add(ss, ts);
    }
#pragma unroll 1
    for (int i = 0; i < k; ++i) {   // sin 2a = 2 sin a cos a, cos 2a = 1 - 2 sin^2 a
        const DD sc = mul(ss, cc), s2 = mul(ss, ss);
        ss = DD{2.0 * sc.h, 2.0 * sc.l};
        cc = sub(DD{1.0, 0.0}, DD{2.0 * s2.h, 2.0 * s2.l});
    }
    const int q = (int)n & 3;   // x = r + n pi/2
    s = (q & 1) ? cc : ss;
    c = (q & 1) ? ss : cc;
    if (q == 2 || q == 3) s = neg(s);
    if (q == 1 || q == 2) c = neg(c);
}

LIW_CR_HD inline double cr_sin(double x) {
    if (!(fabs(x) <= 1048576.0) || x == 0.0) return sin(x);
    DD s, c;
    sincos_dd(x, s, c);
    return s.h + s.l;
}
LIW_CR_HD inline double cr_cos(double x) {
    if (!(fabs(x) <= 1048576.0)) return cos(x);
    DD s, c;
    sincos_dd(x, s, c);
    return c.h + c.l;
}
// atan2(s, c) for finite arguments that are not both zero; anything else goes to the plain function
LIW_CR_HD inline double cr_atan2(double s, double c) {
    const double y = atan2(s, c);
    if (!(fabs(s) < 1e300 && fabs(c) < 1e300) || (s == 0.0 && c == 0.0) || !(fabs(s) > 1e-300 || fabs(c) > 1e-300) || y == 0.0) return y;
    DD S, C;
    sincos_dd(y, S, C);
    const DD num = sub(mul_d(C, s), mul_d(S, c)), den = add(mul_d(C, c), mul_d(S, s));
    const DD d = div(num, den);   // tan(true - y) = true - y to second order: |true - y| is a few ulp
    return add(DD{y, 0.0}, d).h;
}

}  // namespace liw_cr
