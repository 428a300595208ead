// h9g_expr.h -- the layer expressions of the HYDROLOGY substep, each stated
// once.  hydrology_pair (h9g_pair.h) evaluates the same reference expression
// under several lane mappings (a lane's own slots, the helper lanes, the
// one-column wave's task rounds) and in its exact lambdas; every one of them
// calls these functions, so "the same expressions on the same operands: no
// bit changes" holds by construction (which also lists the few
// expressions that keep a copy, and why).  Line numbers cite the reference's
// HYDROLOGY.f90.
//
// Plain functions of their operands: no store, no lane map, no policy but
// the math policy M where they divide by a reciprocal.  A flag argument is
// or-ed into, never cleared.  An operand that a site reads from the store is
// passed where the site read it: by value where the read came first, as a
// callable where it came in the middle of the expression (the order of the
// reads is part of what the compiler schedules from).
#pragma once
#include "h9g_step.h"

namespace h9k {

// the conductivity phase's dsmpdw quotient by Markstein (dsmpdw_fast): at
// L = 8 (round 5: -0.3%), not at L = 10 (+0.8%)
template <int L>
constexpr bool hk_mdiv() { return L <= 8; }

// :605-608 s1 before its clamp, RN(0.5a / 0.5b) = RN(a / b) (the halvings are
// exact for normal a, b) with a = theta(i) + theta(ip), b = ts(i) + ts(ip),
// from y = PF_ITS = RN(1/b) by Markstein's correction: q0 = RN(a y),
// e = a - b q0 (exact), RN(q0 + e y) = RN(a / b) when nothing under- or
// overflows.  a, b in [2^-60, 2^60) keeps q and e normal; other operands set
// bad, for the exact form (hk_exact divides).  (The IEEE division took 11
// VALU in a chain of 9; tools/markstein_check.c.)
H9K_HD float s1_quot_mk(float sa, float sb, float its, bool &bad) {
  const float q0 = sa * its;
  const float s1 = __builtin_fmaf(__builtin_fmaf(-sb, q0, sa), its, q0);
  const uint32_t ua = __builtin_bit_cast(uint32_t, sa) - 0x21800000u;   // 2^-60
  const uint32_t ub = __builtin_bit_cast(uint32_t, sb) - 0x21800000u;
  bad |= (ua > ub ? ua : ub) >= 0x5d800000u - 0x21800000u;             // 2^60
  return s1;
}
// :605-609 s1 = MIN(1, .)
H9K_HD float s1_mk(float sa, float sb, float its, bool &bad) { return MINC(one, s1_quot_mk(sa, sb, its, bad)); }

// :626-627, :866-868 node saturation MIN(1, MAX(q, 0.01)), q = theta / ts
H9K_HD float sat_node(float q) {
  const float s = MAXX(q, 0.01f);
  return MINC(one, s);
}
// :742-744 the aquifer node's, from q = theta(L) / ts(L)
H9K_HD float sat_node_aq(float q) { return sat_node(0.5f * (one + q)); }

// :610-620 hk and dhkdw from pk = s1^(2b+2)
H9K_HD void hk_dhk(float s1, float pk, float hks, float bsw, float its, float &hk, float &dhkdw) {
  const float s2 = hks * pk;
  hk = s1 * s2;
  dhkdw = (2.0f * bsw + 3.0f) * s2 * its;
}
// :562-565, :586-588, :633-634, :748-749 MAX(smpmin, psi * pw): smp from
// pw = s_node^(-b), zq from pw = MAX(vol_eq / ts, 0.01)^(-b)
H9K_HD float smp_of(float psi, float pw) {
  const float sm = psi * pw;
  return MAXC(smpmin, sm);
}
// :636, :753 dsmpdw = -b smp / (s ts), divided
H9K_HD float dsmpdw_div(float bsw, float sm, float s, float ts) { return (-bsw) * sm / (s * ts); }
// ... by mk_div where hk_mdiv<L>() (bad: outside mk_div's range, for the exact form)
template <int L>
H9K_HD float dsmpdw_fast(float bsw, float sm, float s, float ts, bool &bad) {
  if constexpr (hk_mdiv<L>())
    return mk_div((-bsw) * sm, s * ts, bad);
  else
    return dsmpdw_div(bsw, sm, s, ts);
}

// :557-558, :584-585 vol_eq kept in [0, ts]
H9K_HD float vol_clamp(float v, float ts) {
  v = MAXF(v, 0.0f);
  v = MINF(ts, v);
  return v;
}
// :554-558 vol_eq with the water table below the layer, c3 = PF_C3
H9K_HD float vol_eq_below(float c3, float ts, float tempi, float temp0) { return vol_clamp(c3 * (tempi - temp0), ts); }
// :581-583 vol_eq of the aquifer node before vol_clamp, d0 = zw - zi(L)
H9K_HD float vol_aq(float pte, float d0, float temp0) { return pte / d0 * (1.0f - temp0); }
// :535-542 vol_eq with the water table inside the layer (tempi = 1), branch-
// free: PTE / (zw - zlo) from recip64, the division by dz(i) from its stored
// reciprocal.  pte() and rdz() read PF_PTE and 1/dz(i).  A lane where inl
// holds flags a quotient that needs the IEEE division; the exact form
// (eq_exact) divides by zw - zlo.
template <class M, class P, class R>
H9K_HD float vol_eq_in_fast(M &m, P pte, float ts, float temp0, float zw, float zlo, float zhi, R rdz, bool inl,
                            bool &bad) {
  const float d0 = zw - zlo;
  const float q1 = m.div_d(pte(), d0, recip64(d0));
  const bool bq = m.div_bad(q1);
  const float voleq1 = q1 * (one - temp0);
  float vin = m.div_d(voleq1 * (zw - zlo) + ts * (zhi - zw), zhi - zlo, rdz());
  bad |= inl && (bq | m.div_bad(vin));
  vin = MINF(ts, vin);
  vin = MAXF(vin, zero);
  return vin;
}

// :663-670, :689-696, :765-772 the numerators of an interface's qout, dqodw1,
// dqodw2 (= qin, dqidw0, dqidw1 of the next row): num = (smp(i+1) - smp(i)) -
// (zq(i+1) - zq(i)); dsi, dsn = dsmpdw of layers i and i+1
H9K_HD float flux_num(float smp_n, float smp_i, float zq_n, float zq_i) { return (smp_n - smp_i) - (zq_n - zq_i); }
H9K_HD float flux_q(float hk, float num) { return -hk * num; }
H9K_HD float flux_d1(float hk, float num, float dsi, float dhk) { return -(-hk * dsi + num * dhk); }
H9K_HD float flux_d2(float hk, float num, float dsn, float dhk) { return -(hk * dsn + num * dhk); }

// :813-826 the forward sweep's row head: BET(i) and the numerator of dwat2(i),
// i >= 2 (row 1 takes bm and rm themselves)
H9K_HD float row_bet(float am, float bm, float gam) { return bm - am * gam; }
H9K_HD float row_x(float am, float rm, float dprev) { return rm - am * dprev; }

}  // namespace h9k
