// TEST INFRASTRUCTURE ONLY: the host (CPU) build of the day statistics
// (hybrid9_amd/csrc/h9g_stat.h: a segment's summary, folding a day in, appending
// the summary of the days that follow), the lines h9g_daystat_kernel runs per
// cell, used by tests/test_daystat_host.py against the table of include/h9g.h
// restated twice in Python (tests/daystat_helpers.py, hybrid9_amd.day_stats).
// Never linked into the product library.  With -DHOST_STAT_MAIN a stand-alone
// program for a sanitizer build (its records are made here; no Python).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../hybrid9_amd/csrc/h9g_stat.h"

using namespace h9k;

// One year's records (nt, 7, n), cut at cuts[0..ncuts): strictly increasing
// days in (0, nt); the slices are [0, cuts[0]), [cuts[0], cuts[1]), ...,
// [cuts[ncuts-1], nt).  Every slice is summarised on its own, as a wave of the
// kernel does (its S[d-1] and S[d-7] read from the records before the slice),
// and the summaries are merged in order.  tree != 0: merged pairwise, right
// to left, instead of left to right (the same rows if stat_merge is
// associative).  out (17, n).
extern "C" int h9k_host_stat(int n, int nt, const float *rec, int ncuts, const int *cuts, int tree,
                             const h9g_daystat_opts *opts, double *out) {
  if (n < 1 || nt < 1 || ncuts < 0 || !rec || !out || !stat_opts_ok(opts)) return -1;
  for (int i = 0; i < ncuts; i++)
    if (cuts[i] <= (i ? cuts[i - 1] : 0) || cuts[i] >= nt) return -1;
  const size_t nn = (size_t)n;
  std::vector<int> edge;
  edge.push_back(0);
  for (int i = 0; i < ncuts; i++) edge.push_back(cuts[i]);
  edge.push_back(nt);
  for (size_t c = 0; c < nn; c++) {
    auto at = [&](int d, int r) { return rec[((size_t)d * STAT_NREC + r) * nn + c]; };
    std::vector<DayStat> seg(edge.size() - 1);
    for (size_t k = 0; k + 1 < edge.size(); k++) {
      DayStat &s = seg[k];
      stat_init(s);
      for (int d = edge[k]; d < edge[k + 1]; d++) {
        float v[STAT_NREC];
        for (int r = 0; r < STAT_NREC; r++) v[r] = at(d, r);
        const double p0 = d > 0 ? (double)at(d - 1, 0) : 0.0, p1 = d > 0 ? (double)at(d - 1, 1) : 0.0;
        const double p7 = d > 6 ? (double)at(d - 7, 0) : 0.0;
        stat_day(s, d, v, p0, p7, p1, *opts);
      }
    }
    DayStat all;
    if (tree) {
      all = seg.back();
      for (size_t k = seg.size() - 1; k-- > 0;) {
        DayStat a = seg[k];
        stat_merge(a, all);
        all = a;
      }
    } else {
      stat_init(all);                     // (the identity, then every slice in order)
      for (const DayStat &s : seg) stat_merge(all, s);
    }
    double rows[H9G_NDAYSTAT];
    stat_rows(all, rows);
    for (int r = 0; r < H9G_NDAYSTAT; r++) out[(size_t)r * nn + c] = rows[r];
  }
  return 0;
}

// The kernel's cut of a year into nseg slices (stat_slice) as a list of cuts
// (duplicates and the ends dropped); returns their number.
extern "C" int h9k_host_stat_cuts(int nt, int nseg, int *cuts) {
  int m = 0;
  for (int w = 1; w < nseg; w++) {
    int lo, hi;
    stat_slice(nt, nseg, w, lo, hi);
    if (lo > (m ? cuts[m - 1] : 0) && lo < nt) cuts[m++] = lo;
  }
  return m;
}

#if defined(HOST_STAT_MAIN)
// Hand-made records of 8 cells x 366 days with NaN tails, a run across every
// cut and ties, through one slice, the kernel's cuts and single days: the rows
// must agree.  Exit status 0 if they do.
int main() {
  const int n = 8, nt = 366;
  std::vector<float> rec((size_t)nt * STAT_NREC * n);
  uint32_t x = 12345u;
  for (int d = 0; d < nt; d++)
    for (int r = 0; r < STAT_NREC; r++)
      for (int c = 0; c < n; c++) {
        x = x * 1664525u + 1013904223u;
        float v = (float)((x >> 8) % 7u) * 0.25f;            // few distinct values: many ties
        if (r < 2) v = (float)d * 0.5f + v;
        if (c == 3 && d >= 200) v = nanf("");
        if (c == 5) v = nanf("");
        if (c == 6 && d >= 3) v = nanf("");
        rec[((size_t)d * STAT_NREC + r) * n + c] = v;
      }
  h9g_daystat_opts o;
  memset(&o, 0, sizeof(o));
  o.q_thr = 0.5f;
  o.theta_thr = 0.8f;
  o.zwt_thr = 0.6f;
  o.lai_thr = 0.7f;
  std::vector<double> a((size_t)H9G_NDAYSTAT * n), b(a.size());
  if (h9k_host_stat(n, nt, rec.data(), 0, nullptr, 0, &o, a.data())) return 2;
  int bad = 0;
  for (int nseg : {4, 8, 16, 366}) {
    std::vector<int> cuts((size_t)nseg);
    const int m = h9k_host_stat_cuts(nt, nseg, cuts.data());
    for (int tree = 0; tree < 2; tree++) {
      if (h9k_host_stat(n, nt, rec.data(), m, cuts.data(), tree, &o, b.data())) return 2;
      bad += memcmp(a.data(), b.data(), sizeof(double) * a.size()) != 0;
    }
  }
  printf("host_stat: %d of 8 cuts differ from one slice\n", bad);
  return bad ? 1 : 0;
}
#endif
