// liw_crmath.hpp — sin, cos and atan2 of a double evaluated in double-double arithmetic and rounded once, for device code whose
// results are compared with the host's libm bit for bit where that is possible: the device library's sin / cos / atan2 are off by
// up to an ulp or two, glibc's by at most 0.55 ulp, so the correctly rounded value is what glibc returns in all but a fraction of
// a per cent of the arguments.  Used by the tracking glue (k_lfe_track_begin): a last-bit difference in the de-skew twist or the
// predicted pose is amplified by every free-running solve that follows.
//   cr_sincos: |x| scaled by 2^-k to at most 0.25, Taylor series to x^27 in double-double, k double-angle steps (the error grows
//   by 4 per step from 2^-104; arguments beyond 2^20 go to the plain functions).  cr_atan2: one Newton correction of the plain
//   atan2 with the double-double sine and cosine of that estimate: y + (s C - c S) / (c C + s S).
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
    int k = 0;
    double r = x;
    while (fabs(r) > 0.25) { r *= 0.5; ++k; }   // exact
    const DD rr = DD{r, 0.0}, r2 = two_prod(r, r);
    DD ts = rr, tc = DD{1.0, 0.0};
    s = rr;
    c = tc;
#pragma unroll 1
    for (int i = 1; i <= 13; ++i) {
        tc = neg(div_d(mul(tc, r2), (double)((2 * i - 1) * (2 * i))));
        ts = neg(div_d(mul(ts, r2), (double)((2 * i) * (2 * i + 1))));
        c = add(c, tc);
        s = add(s, ts);
    }
#pragma unroll 1
    for (int i = 0; i < k; ++i) {   // sin 2a = 2 sin a cos a, cos 2a = 1 - 2 sin^2 a
        const DD sc = mul(s, c), ss = mul(s, s);
        s = DD{2.0 * sc.h, 2.0 * sc.l};
        c = sub(DD{1.0, 0.0}, DD{2.0 * ss.h, 2.0 * ss.l});
    }
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
