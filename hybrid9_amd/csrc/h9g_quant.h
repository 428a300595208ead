// h9g_quant.h -- the order statistics of h9g_get_dayquant (include/h9g.h): the
// candidate of a day, its monotone key, and MSB-first radix selection of
// several ranks at once over repeated passes through a cell's days.  Host and
// device (h9g_dayquant_kernel in h9g_quant.hip; the host build of
// tests/csrc/host_quant.cpp).
//
// A candidate is one IEEE subtraction of two widened f32 (series 0 and 1) or a
// widened f32 (series 2..6); a NaN candidate is skipped.  Its key is the
// double's bits mapped so that unsigned order is the total order (-inf < ...
// < -0 < +0 < ... < +inf).  Series 2..6 may take the f32's 32-bit key instead:
// widening is monotone and one to one on what is not NaN, so the selected
// value is the same double.
//
// Selection: pass k counts, per rank, the candidates whose bits above digit k
// equal the rank's prefix, by digit k (B bits); the bin that holds the rank
// extends the prefix (quant_step).  After 64/B (32/B) passes the prefix is
// x_(j)'s key, `cnt` the candidates equal to it and `rem` the rank among
// them.  x_(j+1) is the same value where rem + 1 < cnt or j = m - 1, else the
// smallest key above (one more pass, quant_succ).  Every count is an integer
// sum and the successor a minimum: the cut of the days into slices and the
// order of the slices cannot matter.
#pragma once
#include <stdint.h>

#include "../../include/h9g.h"
#include "h9g_geo.h"

namespace h9k {

constexpr int QUANT_NREC = 7;    // H9G_NDAYREC

H9K_HD uint64_t quant_key(double v) {
  uint64_t u;
  __builtin_memcpy(&u, &v, 8);
  return u ^ ((u >> 63) ? ~0ull : (1ull << 63));
}
H9K_HD uint32_t quant_key(float v) {
  uint32_t u;
  __builtin_memcpy(&u, &v, 4);
  return u ^ ((u >> 31) ? ~0u : (1u << 31));
}
H9K_HD double quant_value(uint64_t k) {
  const uint64_t u = k ^ ((k >> 63) ? (1ull << 63) : ~0ull);
  double v;
  __builtin_memcpy(&v, &u, 8);
  return v;
}
H9K_HD double quant_value(uint32_t k) {
  const uint32_t u = k ^ ((k >> 31) ? (1u << 31) : ~0u);
  float v;
  __builtin_memcpy(&v, &u, 4);
  return (double)v;
}

// Series 0 and 1 are differences of the year's running sums (row = series);
// series 2..6 are rows 2..6 as recorded.
H9K_HD bool quant_is_diff(int series) { return series < 2; }

// The candidate of a day from its record value `v` and, for series 0 and 1, the
// value `prev` of the day before (0.0f on a year's day 0): its key, and whether
// it counts (not NaN).
H9K_HD bool quant_cand(bool diff, float v, float prev, uint64_t &key) {
  const double x = diff ? (double)v - (double)prev : (double)v;
  key = quant_key(x);
  return x == x;
}
H9K_HD bool quant_cand(bool, float v, float, uint32_t &key) {   // (series 2..6 only)
  key = quant_key(v);
  return v == v;
}

template <typename K>
struct QuantRank {
  K prefix;          // the bits found so far, right-aligned; after the last pass x_(j)'s key
  uint32_t rem;      // the rank among the candidates that match the prefix
  uint32_t cnt;      // candidates that match the prefix (after pass 0 and later)
};

template <typename K>
H9K_HD void quant_init(QuantRank<K> &r) {
  r.prefix = 0;
  r.rem = 0;
  r.cnt = 0;
}

template <typename K, int B>
struct QuantShape {
  static constexpr int KB = (int)sizeof(K) * 8;
  static constexpr int NB = 1 << B;          // bins a pass counts into
  static constexpr int NP = KB / B;          // passes
  static_assert(KB % B == 0, "the digit width divides the key");
};

// Whether `key` matches the rank's prefix in pass `pass`, and its digit there.
template <typename K, int B>
H9K_HD bool quant_digit(K key, K prefix, int pass, int &digit) {
  const int shift = QuantShape<K, B>::KB - B * (pass + 1);
  digit = (int)((key >> shift) & (K)(QuantShape<K, B>::NB - 1));
  return pass == 0 || (key >> (shift + B - 1) >> 1) == prefix;
}

// j = floor(p * (m - 1)): one IEEE multiply (m >= 1).
H9K_HD uint32_t quant_target(double p, uint32_t m) {
  const double g = p * (double)(m - 1u);
  return (uint32_t)g;                          // (g >= 0: the conversion truncates, which is floor)
}

// After a pass: hist(b), b = 0 .. 2^B - 1, the rank's matching candidates by
// digit.  The bin that holds the rank extends the prefix.
template <typename K, int B, typename H>
H9K_HD void quant_step(QuantRank<K> &r, H hist) {
  uint32_t rem = r.rem, cnt = 0;
  int bin = QuantShape<K, B>::NB - 1;
  bool found = false;
  for (int b = 0; b < QuantShape<K, B>::NB; b++) {
    const uint32_t c = hist(b);
    if (!found) {
      if (rem < c) {
        bin = b;
        cnt = c;
        found = true;
      } else {
        rem -= c;
      }
    }
  }
  r.prefix = (K)((r.prefix << (B - 1) << 1) | (K)bin);
  r.rem = found ? rem : 0u;
  r.cnt = cnt;
}

// Whether x_(j+1) needs the successor pass's answer (else it is x_(j) again).
template <typename K>
H9K_HD bool quant_needs_succ(const QuantRank<K> &r, uint32_t j, uint32_t m) {
  return m > 0 && j + 1u < m && r.rem + 1u >= r.cnt;
}

// Days [lo, hi) of slice w when a year of nt days is cut into nseg slices.
H9K_HD void quant_slice(int nt, int nseg, int w, int &lo, int &hi) {
  lo = (int)((long long)nt * w / nseg);
  hi = (int)((long long)nt * (w + 1) / nseg);
}

// Whether the options are acceptable (include/h9g.h).
H9K_HD bool quant_opts_ok(const h9g_dayquant_opts *o) {
  if (!o || o->series < 0 || o->series >= QUANT_NREC || o->nq < 1 || o->nq > H9G_NQUANT_MAX ||
      (o->pooled != 0 && o->pooled != 1) || o->reserved != 0)
    return false;
  for (int i = 0; i < o->nq; i++)
    if (!(o->p[i] >= 0.0 && o->p[i] <= 1.0)) return false;
  return true;
}

}  // namespace h9k
