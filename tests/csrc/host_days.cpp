// TEST INFRASTRUCTURE ONLY: the host (CPU) build of cell_year_pair with the
// day kernels' policies EvapProf and DaysEt (hybrid9_amd/csrc/h9g_pair.h), one
// lane doing every layer (FlatStore / SplitAll, as tests/csrc/host_evap.cpp),
// used by tests/test_days_host.py to pin the day records (include/h9g.h
// H9G_NDAYREC) against the oracle's per-substep trace without a GPU, and by
// tests/test_gpu_days.py as what the day kernels must store.  Built a second
// time with -DH9G_FORCE_RERUN=5, where the exact replay from the day snapshot
// runs in about every other eligible substep: the records are taken after the
// day's last substep and must not see it.  Never linked into the product
// library.
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>
// exact re-runs: count, substeps replayed
static long long g_exact[2];
#define H9G_EXACT_HOOK(k0, ns)                                          \
  do {                                                                  \
    __atomic_add_fetch(&g_exact[0], 1, __ATOMIC_RELAXED);               \
    __atomic_add_fetch(&g_exact[1], (ns) - (k0) + 1, __ATOMIC_RELAXED); \
  } while (0)
#include "../../hybrid9_amd/csrc/h9g_geo.h"
#include "../../hybrid9_amd/csrc/h9g_step.h"
#include "../../hybrid9_amd/csrc/h9g_pair.h"
#include "../../hybrid9_amd/csrc/h9g_rows.h"

using namespace h9k;
static const uint64_t E2[32] = H9M_EXP2F_TAB_INIT;
static const double L2[32] = H9M_POWF_LOG2_TAB_INIT;

constexpr int NM = 12;   // H9G_NMONTHS (include/h9g.h)
constexpr int ND = 7;    // H9G_NDAYREC
constexpr int MAXD = 366;
static_assert(ND == DaysEt::NREC, "the day record");

static int diy(int y) { return y % 4 ? 365 : (y % 100 ? 366 : (y % 400 ? 365 : 366)); }

// ann (nyears, 12+L, n), mon (nyears, 12, 12+L, n; may be null: no monthly
// recording) and days (nyears, 366, 7, n) come in as NaN.  A cell that stops
// keeps the year's days before its STOP day; DaysEt::stop makes the rest NaN
// (the year's buffer starts out as -1: every day must be written).
template <int L, class G>
static int run_cells(const G &g, int n, int nisurf, int grow_on, int year0, int nyears, const float *par,
                     const float *forc, float *st, float *ann, float *mon, float *days, int *err) {
  const h9m::Tabs T = {E2, L2};
  constexpr int R = Rows<L>::ANNUAL;
  int ndays = 0;
  for (int y = 0; y < nyears; y++) ndays += diy(year0 + y);
  int first = 0;
  std::vector<float> prow((size_t)Rows<L>::PAR * n), srow((size_t)Rows<L>::STATE * n);
  par_rows_from_packed(L, n, par, prow.data());
  state_rows_from_packed(L, n, st, srow.data());
#pragma omp parallel for schedule(dynamic, 4)
  for (int c = 0; c < n; c++) {
    float store[FlatStore<L>::N], zt[zt_size<L>()];
    fill_zt<L>(g, zt);
    FlatStore<L> cs{store, zt};
    const SplitAll sp;
    St<L> s;
    H9K_LOAD_LANE(L, cs, s, prow.data(), n, c, srow.data(), n, c)
    H9K_LOAD_SCALARS(L, s, srow.data(), n, c)
    H9K_TS_SUM(L, cs, ts_sum)
    if (!(ts_sum > SOIL_TRUNC)) continue;
    cell_inv_pair<L, G>(g, cs);
    int d0 = 0;
    for (int y = 0; y < nyears; y++) {
      const int nt = diy(year0 + y);
      float a[R], m[NM * R];
      std::vector<float> dr((size_t)nt * ND, -1.0f);
      for (float &v : m) v = -1.0f;                  // (every value must be stored by its month end)
      int eday = 0, estep = 0;
      float ev = 0;
      const int code = cell_year_pair<L, G, SplitAll, FlatStore<L>, true, EvapProf, DaysEt>(
          g, cs, sp, s, forc + (size_t)d0 * n + c, (size_t)n, (size_t)ndays * n, nt, nisurf, grow_on, a, 1, eday, estep,
          ev, T, 0, EvapProf{zero, g.dt()}, DaysEt{mon ? m : nullptr, 1, dr.data(), a});
      for (int r = 0; r < nt * ND; r++) days[((size_t)y * MAXD * ND + r) * n + c] = dr[r];
      if (code) {
        err[4 * c] = code; err[4 * c + 1] = y; err[4 * c + 2] = eday; err[4 * c + 3] = estep;
#pragma omp atomic write
        first = code;
        break;
      }
      for (int r = 0; r < R; r++) ann[((size_t)y * R + r) * n + c] = a[r];
      if (mon)
        for (int r = 0; r < NM * R; r++) mon[((size_t)y * NM * R + r) * n + c] = m[r];
      d0 += nt;
    }
    H9K_STORE_CELL(L, s, cs, srow.data(), n, c, grow_on, SC_N)
  }
  state_packed_from_rows(L, n, srow.data(), st);
  return first;
}

// use_const_geo: 1 = the built-in layer sets and NISURF 24|48 as compile-time
// geometry (GeoC), 0 = runtime geometry (GeoR).
extern "C" int h9k_host_days(int n, int L, int nisurf, int grow_on, int year0, int nyears, int use_const_geo,
                             const float *zi, const float *par, const float *forc, float *st, float *ann,
                             float *mon, float *days, int *err) {
  const bool cg = use_const_geo != 0;
#define RP(LL, G) return run_cells<LL>(G, n, nisurf, grow_on, year0, nyears, par, forc, st, ann, mon, days, err)
  if (L == 8) {
    if (cg && nisurf == 48) RP(8, (GeoC<8, 48>()));
    if (cg && nisurf == 24) RP(8, (GeoC<8, 24>()));
    RP(8, make_geo_r<8>(zi, nisurf));
  }
  if (cg && nisurf == 48) RP(10, (GeoC<10, 48>()));
  if (cg && nisurf == 24) RP(10, (GeoC<10, 24>()));
  RP(10, make_geo_r<10>(zi, nisurf));
#undef RP
}

// Exact re-runs since the last call: out[0] runs, out[1] substeps replayed.
extern "C" void h9k_days_exact(long long *out) {
  out[0] = __atomic_exchange_n(&g_exact[0], 0, __ATOMIC_RELAXED);
  out[1] = __atomic_exchange_n(&g_exact[1], 0, __ATOMIC_RELAXED);
}
