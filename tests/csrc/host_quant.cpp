// TEST INFRASTRUCTURE ONLY: the host (CPU) build of the day quantiles
// (hybrid9_amd/csrc/h9g_quant.h: a day's candidate and key, the digit of a
// pass, the step that extends a rank's prefix, the successor rule), the lines
// h9g_dayquant_kernel runs per cell, used by tests/test_dayquant_host.py
// against the contract of include/h9g.h restated twice in Python
// (hybrid9_amd.day_order_stats, tests/dayquant_helpers.py).  Never linked into
// the product library.  With -DHOST_QUANT_MAIN a stand-alone program for a
// sanitizer build (its records are made here; no Python).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../hybrid9_amd/csrc/h9g_quant.h"

using namespace h9k;

namespace {

struct Span {
  int n, nyears, ntmax;
  const int *nt;
  const float *rec;                 // (nyears, ntmax, 7, n)
  std::vector<int> edge;            // slice edges, days; clipped to each year's length
  bool rev;                         // slices visited last to first
  float at(int y, int d, int r, size_t c) const {
    return rec[(((size_t)y * ntmax + d) * QUANT_NREC + r) * (size_t)n + c];
  }
};

// One streaming pass of cell c over years [y0, y1): every slice of every year
// on its own, as a wave of the kernel reads it (the day before a slice's first
// read from the records), f(key) for every candidate that counts.
template <typename K, typename F>
void stream(const Span &s, size_t c, int series, int y0, int y1, F f) {
  const bool diff = quant_is_diff(series);
  const int ns = (int)s.edge.size() - 1;
  for (int y = y0; y < y1; y++)
    for (int i = 0; i < ns; i++) {
      const int k = s.rev ? ns - 1 - i : i;
      const int lo = s.edge[k] < s.nt[y] ? s.edge[k] : s.nt[y], hi = s.edge[k + 1] < s.nt[y] ? s.edge[k + 1] : s.nt[y];
      float prev = diff && lo > 0 && lo < hi ? s.at(y, lo - 1, series, c) : 0.0f;
      for (int d = lo; d < hi; d++) {
        const float v = s.at(y, d, series, c);
        K key;
        if (quant_cand(diff, v, prev, key)) f(key);
        prev = v;
      }
    }
}

template <typename K, int B>
void select(const Span &s, const h9g_dayquant_opts &o, double *out) {
  using S = QuantShape<K, B>;
  const size_t nn = (size_t)s.n, rows = (size_t)(1 + 2 * o.nq);
  const int nres = o.pooled ? 1 : s.nyears;
  for (int res = 0; res < nres; res++)
    for (size_t c = 0; c < nn; c++) {
      const int y0 = o.pooled ? 0 : res, y1 = o.pooled ? s.nyears : res + 1;
      double *dst = out + (size_t)res * rows * nn + c;
      for (int i = 0; i < o.nq; i++) {
        QuantRank<K> rk;
        quant_init(rk);
        uint32_t m = 0, jt = 0;
        for (int pass = 0; pass < S::NP; pass++) {
          uint32_t hist[S::NB] = {};
          stream<K>(s, c, o.series, y0, y1, [&](K key) {
            int dg;
            if (quant_digit<K, B>(key, rk.prefix, pass, dg)) hist[dg]++;
          });
          if (pass == 0) {
            for (int b = 0; b < S::NB; b++) m += hist[b];
            jt = m ? quant_target(o.p[i], m) : 0u;
            rk.rem = jt;
          }
          quant_step<K, B>(rk, [&](int b) { return hist[b]; });
        }
        K succ = ~(K)0;
        stream<K>(s, c, o.series, y0, y1, [&](K key) {
          if (key > rk.prefix && key < succ) succ = key;
        });
        const double x = m ? quant_value(rk.prefix) : nan("");
        dst[0] = (double)m;
        dst[(size_t)(1 + 2 * i) * nn] = x;
        dst[(size_t)(2 + 2 * i) * nn] = quant_needs_succ(rk, jt, m) ? quant_value(succ) : x;
      }
    }
}

template <typename K>
int select_b(int bits, const Span &s, const h9g_dayquant_opts &o, double *out) {
  switch (bits) {
    case 2: select<K, 2>(s, o, out); return 0;
    case 4: select<K, 4>(s, o, out); return 0;
    case 8: select<K, 8>(s, o, out); return 0;
    default: return -1;
  }
}

}  // namespace

// records (nyears, ntmax, 7, n), ntmax = max nt.  Every year is cut at
// cuts[0..ncuts) (strictly increasing days > 0; those past a year's end leave
// empty slices); rev != 0 visits the slices last to first.  bits: the digit
// width (2, 4, 8: those the kernel is built with); key64 != 0: the 64-bit key
// for series 2..6 too.  out (nres, 1 + 2 nq, n).  -1 for arguments the product
// refuses (quant_opts_ok) or a bad cut.
extern "C" int h9k_host_quant(int n, int nyears, const int *nt, const float *rec, int ncuts, const int *cuts, int rev,
                              int bits, int key64, const h9g_dayquant_opts *opts, double *out) {
  if (n < 1 || nyears < 1 || !nt || !rec || ncuts < 0 || !out || !quant_opts_ok(opts)) return -1;
  Span s{n, nyears, 0, nt, rec, {}, rev != 0};
  for (int y = 0; y < nyears; y++) {
    if (nt[y] < 1) return -1;
    if (nt[y] > s.ntmax) s.ntmax = nt[y];
  }
  s.edge.push_back(0);
  for (int i = 0; i < ncuts; i++) {
    if (cuts[i] <= s.edge.back()) return -1;
    s.edge.push_back(cuts[i]);
  }
  if (s.edge.back() < s.ntmax) s.edge.push_back(s.ntmax);
  if (key64 || quant_is_diff(opts->series)) return select_b<uint64_t>(bits, s, *opts, out);
  return select_b<uint32_t>(bits, s, *opts, out);
}

// The kernel's cut of a year into nseg slices (quant_slice) as a list of cuts
// (duplicates and the ends dropped); returns their number.
extern "C" int h9k_host_quant_cuts(int nt, int nseg, int *cuts) {
  int m = 0;
  for (int w = 1; w < nseg; w++) {
    int lo, hi;
    quant_slice(nt, nseg, w, lo, hi);
    if (lo > (m ? cuts[m - 1] : 0) && lo < nt) cuts[m++] = lo;
  }
  return m;
}

// Whether the options pass the product's check (no device involved).
extern "C" int h9k_host_quant_opts_ok(const h9g_dayquant_opts *opts) { return quant_opts_ok(opts) ? 1 : 0; }

#if defined(HOST_QUANT_MAIN)
// Records of 8 cells x 3 years (365, 366, 365 days) with ties, NaN tails, -0
// and +inf, every series, per year and pooled, through every digit width, both
// keys and several cuts: all must give the bits of one slice with 4-bit digits.
// Exit status 0 if they do.
int main() {
  const int n = 8, nyears = 3, nt[3] = {365, 366, 365}, ntmax = 366;
  std::vector<float> rec((size_t)nyears * ntmax * QUANT_NREC * n, nanf(""));
  uint32_t x = 12345u;
  for (int y = 0; y < nyears; y++)
    for (int d = 0; d < nt[y]; d++)
      for (int r = 0; r < QUANT_NREC; r++)
        for (int c = 0; c < n; c++) {
          x = x * 1664525u + 1013904223u;
          float v = (float)((x >> 8) % 7u) * 0.25f - 0.5f;       // few distinct values: many ties
          if (v == 0.0f && (x >> 20) % 2u) v = -0.0f;
          if (r < 2) v = (float)d * 0.5f + v;
          if (c == 2 && d == 100) v = INFINITY;
          if (c == 3 && d >= 200) v = nanf("");
          if (c == 5) v = nanf("");
          if (c == 6 && (d >= 1 || y > 0)) v = nanf("");
          rec[(((size_t)y * ntmax + d) * QUANT_NREC + r) * n + c] = v;
        }
  int bad = 0, runs = 0;
  for (int series = 0; series < QUANT_NREC; series++)
    for (int pooled = 0; pooled < 2; pooled++) {
      h9g_dayquant_opts o;
      memset(&o, 0, sizeof(o));
      o.series = series;
      o.pooled = pooled;
      const double p[7] = {0.0, 0.05, 0.5, 0.95, 1.0, 0.5, 0.2};
      o.nq = 7;
      memcpy(o.p, p, sizeof(p));
      const size_t len = (size_t)(pooled ? 1 : nyears) * (1 + 2 * o.nq) * n;
      std::vector<double> a(len), b(len);
      if (h9k_host_quant(n, nyears, nt, rec.data(), 0, nullptr, 0, 4, 0, &o, a.data())) return 2;
      for (int bits : {2, 4, 8})
        for (int key64 = 0; key64 < 2; key64++)
          for (int nseg : {1, 8, 16, 366})
            for (int rev = 0; rev < 2; rev++) {
              std::vector<int> cuts((size_t)nseg);
              const int m = h9k_host_quant_cuts(ntmax, nseg, cuts.data());
              if (h9k_host_quant(n, nyears, nt, rec.data(), m, cuts.data(), rev, bits, key64, &o, b.data())) return 2;
              bad += memcmp(a.data(), b.data(), sizeof(double) * len) != 0;
              runs++;
            }
    }
  printf("host_quant: %d of %d runs differ from one slice\n", bad, runs);
  return bad ? 1 : 0;
}
#endif
