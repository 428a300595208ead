// TEST INFRASTRUCTURE ONLY: a host (CPU) build of cell_focus
// (hybrid9_amd/csrc/h9g_pair.h), the shadow run behind the daily diagnostics
// line (h9g_set_daily / h9g_get_daily), used by tests/test_daily_host.py to
// pin it against the reference golden and the oracle's trace without a GPU,
// and by tests/test_gpu_daily.py as what the device build must equal.
// Layouts as tests/csrc/host_kernel.cpp: the oracle's packed parameters and
// state, forcing (7, ndays, n); out (ndays, 11, n).  Never linked into the
// product library.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../hybrid9_amd/csrc/h9g_geo.h"
#include "../../hybrid9_amd/csrc/h9g_step.h"
#include "../../hybrid9_amd/csrc/h9g_pair.h"
#include "../../hybrid9_amd/csrc/h9g_rows.h"

using namespace h9k;
static const uint64_t E2[32] = H9M_EXP2F_TAB_INIT;
static const double L2[32] = H9M_POWF_LOG2_TAB_INIT;

static int diy(int y) { return y % 4 ? 365 : (y % 100 ? 366 : (y % 400 ? 365 : 366)); }

// failed (may be null): cells that had stopped when the run starts.
template <int L, class G>
static int run_focus_cells(const G &g, int n, int nisurf, int grow_on, int year0, int nyears, const float *par,
                           const float *forc, const float *st, const int *failed, float *out, int *code_out) {
  const h9m::Tabs T = {E2, L2};
  int ndays = 0;
  FocusYear yrs[64];
  for (int y = 0; y < nyears; y++) {
    yrs[y].forc = forc + (size_t)ndays * n;
    yrs[y].nt = diy(year0 + y);
    ndays += yrs[y].nt;
  }
  int first = 0;
  // the oracle's packed blocks as rows of n (h9g_rows.h), as the device reads them
  std::vector<float> prow((size_t)Rows<L>::PAR * n), srow((size_t)Rows<L>::STATE * n);
  par_rows_from_packed(L, n, par, prow.data());
  state_rows_from_packed(L, n, st, srow.data());
#pragma omp parallel for schedule(dynamic, 1)
  for (int c = 0; c < n; c++) {
    float store[FlatStore<L>::N], zt[zt_size<L>()];
    fill_zt<L>(g, zt);
    FlatStore<L> cs{store, zt};
    St<L> s;
    H9K_LOAD_LANE(L, cs, s, prow.data(), n, c, srow.data(), n, c)
    H9K_LOAD_SCALARS(L, s, srow.data(), n, c)
    H9K_TS_SUM(L, cs, ts_sum)
    code_out[c] = 0;
    if (!(ts_sum > SOIL_TRUNC) || (failed && failed[c])) {
      nan_rows(out, ndays * DAILY_ROWS, n, c);
      continue;
    }
    cell_inv_pair<L, G>(g, cs);
    const int code = cell_focus<L, G>(g, cs, s, srow[(size_t)Rows<L>::H2O_MA * n + c], yrs, nyears, (size_t)c, (size_t)n,
                                      (size_t)ndays * n, nisurf, grow_on, out + c, (size_t)n, T);
    code_out[c] = code;
    if (code) {
#pragma omp atomic write
      first = code;
    }
  }
  return first;
}

// use_const_geo: 1 = the built-in layer sets and NISURF 24|48 as compile-time
// geometry (GeoC), 0 = runtime geometry (GeoR).  nyears <= 64.
extern "C" int h9k_host_focus(int n, int L, int nisurf, int grow_on, int year0, int nyears, int use_const_geo,
                              const float *zi, const float *par, const float *forc, const float *st,
                              const int *failed, float *out, int *code_out) {
  const bool cg = use_const_geo != 0;
  if (nyears < 1 || nyears > 64) return -1;
#define RF(LL, G) return run_focus_cells<LL>(G, n, nisurf, grow_on, year0, nyears, par, forc, st, failed, out, code_out)
  if (L == 8) {
    if (cg && nisurf == 48) RF(8, (GeoC<8, 48>()));
    if (cg && nisurf == 24) RF(8, (GeoC<8, 24>()));
    RF(8, make_geo_r<8>(zi, nisurf));
  }
  if (cg && nisurf == 48) RF(10, (GeoC<10, 48>()));
  if (cg && nisurf == 24) RF(10, (GeoC<10, 24>()));
  RF(10, make_geo_r<10>(zi, nisurf));
#undef RF
}
