// h9g_spin.h -- the per-cell test of h9g_spinup (include/h9g.h): a cell's
// keys, their drift between two cycle ends and the decision.  Host and device
// (h9g_spin_kernel in h9g_spin.hip; the host build of tests/csrc/host_spin.cpp).
//
// Everything is double from the f32 state, one IEEE operation per statement
// (the build has no contraction), so a numpy restatement gives the same bits:
//   W   = h2osoi_liq(1) + ... + h2osoi_liq(L) in that order, then + wa
//   d_w = |W_k - W_{k-1}|,  d_z = |zwt_k - zwt_{k-1}|
//   d_p = 0 if pm_k == pm_{k-1}, else |pm_k - pm_{k-1}| / |pm_{k-1}|
// Every comparison is written `drift <= tolerance`: false for a NaN drift.
#pragma once
#include "h9g_rows.h"

namespace h9k {

constexpr int SPIN_KEYS = 3;     // rows of the previous keys: W, zwt, pm
// a cell's entry of cell_cycle besides a settling cycle k > 0
enum : int { SPIN_ACTIVE = 0, SPIN_NEVER = -1, SPIN_STOPPED = -2 };

struct SpinKey { double w, zwt, pm; };
struct SpinTol { int min_cycles; double water, zwt, plant; };

// st: state rows of stride n (h9g_rows.h), cell c, L layers
H9K_HD SpinKey spin_key(const float *st, size_t n, size_t c, int L) {
  SpinKey k;
  double w = 0.0;
  for (int i = 0; i < L; i++) w = w + (double)st[(size_t)i * n + c];   // (the h2o rows start the state)
  k.w = w + (double)st[(size_t)scalar_row(L, SC_WA) * n + c];
  k.zwt = (double)st[(size_t)scalar_row(L, SC_ZWT) * n + c];
  k.pm = (double)st[(size_t)scalar_row(L, SC_PM) * n + c];
  return k;
}

// drift from `a` (cycle k-1) to `b` (cycle k): the key's fields hold d_w, d_z, d_p
H9K_HD SpinKey spin_drift(const SpinKey &a, const SpinKey &b) {
  SpinKey d;
  const double dw = b.w - a.w, dz = b.zwt - a.zwt;
  d.w = __builtin_fabs(dw);
  d.zwt = __builtin_fabs(dz);
  if (b.pm == a.pm) {
    d.pm = 0.0;
  } else {
    const double dp = b.pm - a.pm;
    d.pm = __builtin_fabs(dp) / __builtin_fabs(a.pm);
  }
  return d;
}

H9K_HD bool spin_settled(const SpinKey &d, int k, const SpinTol &t) {
  return k >= t.min_cycles && d.w <= t.water && d.zwt <= t.zwt && d.pm <= t.plant;
}

// the running maximum of a drift: a NaN is not counted
H9K_HD double spin_max(double m, double d) { return d > m ? d : m; }

// Soil mask of HYBRID9.f90:122-123 from the parameter rows (as H9K_TS_SUM).
H9K_HD bool spin_soil(const float *par, size_t n, size_t c, int L) {
  float sum = 0.0f;
  for (int i = 0; i < L; i++) sum = sum + par[(size_t)par_row(L, 0, i) * n + c];
  return sum > SOIL_TRUNC;
}

}  // namespace h9k
