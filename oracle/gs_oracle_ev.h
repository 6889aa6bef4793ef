/*
 * gs_oracle_ev.h -- CPU ORACLE (test infrastructure, NOT product code): the running-error arithmetic shared by the error
 * budgets of the oracle (gso_project_bwd_budget in gs_oracle.c, gso_shade_bwd_budget in gs_oracle_shade.c).
 */
#ifndef GS_ORACLE_EV_H
#define GS_ORACLE_EV_H
#include <math.h>

/* Running-error arithmetic of the budget (gso_project_bwd_budget): a value (double) and a bound `e` of the absolute error
 * an fp32 evaluation of it may carry, in units of the fp32 unit roundoff 2^-24.  Every operation propagates the errors of
 * its operands to first order (plus the second-order product term) and adds one rounding of its own, sized by the
 * ABSOLUTE values of the operands: a sum or difference a +- b is charged |a| + |b|, not |a +- b|, so cancellation cannot
 * hide error, and an implementation that sums in another order, contracts a product into the sum or uses a
 * one-ulp reciprocal stays within a small multiple of the bound.  Exact inputs carry e = 0; products with an exact zero stay
 * exactly zero with e = 0 (a Gaussian whose cotangents are all zero gets budget 0).                                        */
typedef struct { double v, e; } gso_ev;
#define GSO_EPS (1.0 / 16777216.0)                      /* 2^-24 */
static inline double ev_me(double m, double e) { return m == 0.0 || e == 0.0 ? 0.0 : m * e; }      /* magnitude * error, 0 * inf = 0 */
static inline gso_ev ev_in(double v) { gso_ev r = { v, 0.0 }; return r; }
static inline gso_ev ev_err(double v, double e) { gso_ev r = { v, e }; return r; }
static inline gso_ev ev_scale(gso_ev a, double c) { gso_ev r = { a.v * c, ev_me(fabs(c), a.e) }; return r; }   /* exact factor (+-1, 2, 0.5) */
static inline gso_ev ev_mul(gso_ev a, gso_ev b)
{
    gso_ev r; r.v = a.v * b.v;
    if ((a.v == 0.0 && a.e == 0.0) || (b.v == 0.0 && b.e == 0.0)) { r.e = 0.0; return r; }      /* an exact zero (0 * inf stays out) */
    r.e = ev_me(fabs(a.v), b.e) + ev_me(fabs(b.v), a.e) + ev_me(a.e, b.e) * GSO_EPS + fabs(r.v);
    return r;
}
static inline gso_ev ev_add(gso_ev a, gso_ev b)
{
    gso_ev r; r.v = a.v + b.v;
    r.e = a.e + b.e + ((a.v == 0.0 && a.e == 0.0) || (b.v == 0.0 && b.e == 0.0) ? 0.0 : fabs(a.v) + fabs(b.v));
    return r;
}
static inline gso_ev ev_sub(gso_ev a, gso_ev b) { return ev_add(a, ev_scale(b, -1.0)); }
static inline gso_ev ev_div(gso_ev a, gso_ev b)
{
    gso_ev r; r.v = a.v / b.v;
    if (a.v == 0.0 && a.e == 0.0) { r.e = 0.0; return r; }
    const double den = fabs(b.v) - b.e * GSO_EPS;       /* the smallest the divisor may be */
    r.e = den > 0.0 ? (a.e + ev_me(fabs(r.v), b.e)) / den + fabs(r.v) : INFINITY;
    return r;
}
static inline gso_ev ev_sqrt(gso_ev a)                  /* a.v >= 0; not first order: the argument may be as uncertain as it is large */
{
    gso_ev r; r.v = sqrt(a.v);
    const double E = a.e * GSO_EPS, lo = a.v > E ? a.v - E : 0.0;
    const double up = sqrt(a.v + E) - r.v, dn = r.v - sqrt(lo);
    r.e = (up > dn ? up : dn) / GSO_EPS + r.v;
    return r;
}
static inline gso_ev ev_dot2(gso_ev a0, gso_ev b0, gso_ev a1, gso_ev b1) { return ev_add(ev_mul(a0, b0), ev_mul(a1, b1)); }
static inline gso_ev ev_dot3(gso_ev a0, gso_ev b0, gso_ev a1, gso_ev b1, gso_ev a2, gso_ev b2)
{
    return ev_add(ev_dot2(a0, b0, a1, b1), ev_mul(a2, b2));
}
static inline gso_ev ev_clamp(gso_ev x, gso_ev lo, gso_ev hi) { return x.v > hi.v ? hi : (x.v < lo.v ? lo : x); }

#endif
