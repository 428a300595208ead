// h9g_stat.h -- the day statistics of h9g_get_daystats (include/h9g.h): the
// summary of a run of consecutive days of one cell's day records, how a day is
// folded into it and how the summary of the days that follow is appended.
// Host and device (h9g_daystat_kernel in h9g_stat.hip; the host build of
// tests/csrc/host_stat.cpp).
//
// Every quantity is one IEEE operation on the f32 records (the build has no
// contraction), every extreme a strict comparison in day order and every count
// an integer, so the 17 rows do not depend on how the year is cut into
// segments, and a numpy restatement gives the same bits:
//   q[d]  = (double)R[d][0] - (double)R[d-1][0]          (R[-1][0] = 0)
//   e[d]  = the same from row 1
//   q7[d] = (double)R[d][0] - (double)R[d-7][0], d >= 6  (R[-1][0] = 0)
// A NaN candidate is skipped: `v == v` guards every update, and the running
// extreme starts as NaN ("none yet"), which `!(m >= v)` / `!(m <= v)` replace
// with the first candidate and a later equal value never does.
#pragma once
#include <stdint.h>

#include "../../include/h9g.h"
#include "h9g_geo.h"

namespace h9k {

constexpr int STAT_NREC = 7;     // H9G_NDAYREC

struct DayStat {
  // counts over the segment's days
  int len;                       // days in the segment
  int ndays;                     // ... none of whose seven values is NaN
  int q_days, dry_days, wet_days, green_days;
  // the dry-spell monoid: the dry runs at the segment's two ends and the
  // longest inside it (the whole segment is dry when lead == len)
  int lead, trail, best;
  // extremes with the 0-based day of their first occurrence (-1: none)
  int q_max_day, w_min_day, lai_max_day;
  double q_max, q7_min, e_max;   // NaN: none
  float w_min, w_max, theta1_min, zwt_min, lai_max;
};

H9K_HD void stat_init(DayStat &s) {
  s.len = s.ndays = s.q_days = s.dry_days = s.wet_days = s.green_days = 0;
  s.lead = s.trail = s.best = 0;
  s.q_max_day = s.w_min_day = s.lai_max_day = -1;
  s.q_max = s.q7_min = s.e_max = __builtin_nan("");
  s.w_min = s.w_max = s.theta1_min = s.zwt_min = s.lai_max = __builtin_nanf("");
}

// The strict-comparison rule: v replaces m when m is none or v is beyond it.
template <typename T>
H9K_HD void stat_max(T &m, T v) {
  if (v == v && !(m >= v)) m = v;
}
template <typename T>
H9K_HD void stat_min(T &m, T v) {
  if (v == v && !(m <= v)) m = v;
}
template <typename T>
H9K_HD void stat_max_at(T &m, int &at, T v, int d) {
  if (v == v && !(m >= v)) {
    m = v;
    at = d;
  }
}
template <typename T>
H9K_HD void stat_min_at(T &m, int &at, T v, int d) {
  if (v == v && !(m <= v)) {
    m = v;
    at = d;
  }
}

// Folds day d (0-based day of the year) in behind the segment's days.  rec: the
// day's record; s0_prev, s1_prev: (double) rows 0 and 1 of day d-1 (0 for d =
// 0); s0_prev7: (double) row 0 of day d-7 (0 for d = 6; not read for d < 6).
H9K_HD void stat_day(DayStat &s, int d, const float rec[STAT_NREC], double s0_prev, double s0_prev7, double s1_prev,
                     const h9g_daystat_opts &o) {
  bool valid = true;
  for (int r = 0; r < STAT_NREC; r++) valid = valid && rec[r] == rec[r];
  s.ndays += valid ? 1 : 0;
  const double s0 = (double)rec[0], s1 = (double)rec[1];
  const double q = s0 - s0_prev, e = s1 - s1_prev;
  stat_max_at(s.q_max, s.q_max_day, q, d);
  if (d >= 6) {
    const double q7 = s0 - s0_prev7;
    stat_min(s.q7_min, q7);
  }
  s.q_days += q >= (double)o.q_thr ? 1 : 0;
  stat_max(s.e_max, e);
  stat_min_at(s.w_min, s.w_min_day, rec[2], d);
  stat_max(s.w_max, rec[2]);
  stat_min(s.theta1_min, rec[3]);
  const bool dry = rec[3] < o.theta_thr;           // (false for a NaN: it ends a run)
  s.dry_days += dry ? 1 : 0;
  if (dry) {
    if (s.lead == s.len) s.lead = s.lead + 1;
    s.trail = s.trail + 1;
    if (s.trail > s.best) s.best = s.trail;
  } else {
    s.trail = 0;
  }
  s.len = s.len + 1;
  stat_min(s.zwt_min, rec[4]);
  s.wet_days += rec[4] <= o.zwt_thr ? 1 : 0;
  stat_max_at(s.lai_max, s.lai_max_day, rec[6], d);
  s.green_days += rec[6] >= o.lai_thr ? 1 : 0;
}

// a: a segment; b: the segment of the days that follow it.  a becomes both.
// Associative; a summary with no day (stat_init) is its identity on either side.
H9K_HD void stat_merge(DayStat &a, const DayStat &b) {
  const int across = a.trail + b.lead;
  int best = a.best > b.best ? a.best : b.best;
  if (across > best) best = across;
  const int lead = a.lead == a.len ? a.len + b.lead : a.lead;
  const int trail = b.trail == b.len ? a.trail + b.len : b.trail;
  a.best = best;
  a.lead = lead;
  a.trail = trail;
  a.len += b.len;
  a.ndays += b.ndays;
  a.q_days += b.q_days;
  a.dry_days += b.dry_days;
  a.wet_days += b.wet_days;
  a.green_days += b.green_days;
  stat_max_at(a.q_max, a.q_max_day, b.q_max, b.q_max_day);
  stat_min(a.q7_min, b.q7_min);
  stat_max(a.e_max, b.e_max);
  stat_min_at(a.w_min, a.w_min_day, b.w_min, b.w_min_day);
  stat_max(a.w_max, b.w_max);
  stat_min(a.theta1_min, b.theta1_min);
  stat_min(a.zwt_min, b.zwt_min);
  stat_max_at(a.lai_max, a.lai_max_day, b.lai_max, b.lai_max_day);
}

// The 17 rows of include/h9g.h's table.
H9K_HD void stat_rows(const DayStat &s, double out[H9G_NDAYSTAT]) {
  out[0] = (double)s.ndays;
  out[1] = s.q_max;
  out[2] = (double)s.q_max_day;
  out[3] = s.q7_min;
  out[4] = (double)s.q_days;
  out[5] = s.e_max;
  out[6] = (double)s.w_min;
  out[7] = (double)s.w_min_day;
  out[8] = (double)s.w_max;
  out[9] = (double)s.theta1_min;
  out[10] = (double)s.dry_days;
  out[11] = (double)s.best;
  out[12] = (double)s.zwt_min;
  out[13] = (double)s.wet_days;
  out[14] = (double)s.lai_max;
  out[15] = (double)s.lai_max_day;
  out[16] = (double)s.green_days;
}

// Days [lo, hi) of slice w when a year of nt days is cut into nseg slices.
H9K_HD void stat_slice(int nt, int nseg, int w, int &lo, int &hi) {
  lo = (int)((long long)nt * w / nseg);
  hi = (int)((long long)nt * (w + 1) / nseg);
}

// Whether the thresholds are acceptable (include/h9g.h: no NaN, reserved 0).
H9K_HD bool stat_opts_ok(const h9g_daystat_opts *o) {
  return o && o->q_thr == o->q_thr && o->theta_thr == o->theta_thr && o->zwt_thr == o->zwt_thr &&
         o->lai_thr == o->lai_thr && o->reserved[0] == 0 && o->reserved[1] == 0 && o->reserved[2] == 0 &&
         o->reserved[3] == 0;
}

}  // namespace h9k
