// h9g_plain.hip -- the plain year kernels' translation unit: the year kernels
// of h9g_year.h as they are, behind h9g_plain_launch.  A unit of its own, as
// h9g_mon.hip and h9g_et.hip, so that no change to the host runtime compiles
// them again (hybrid9_amd/build.py).  The measurement builds' device globals
// are read and written here, beside the kernels that use them.
#include "h9g_year.h"

#if defined(H9G_COUNT_EXACT) || defined(H9G_COUNT_BRANCH)
#include <string.h>

#include <algorithm>
#include <vector>
#endif

int h9g_plain_launch(Shape shape, const h9g_config *cfg, hipStream_t stream, const KArgs &a) {
  return launch_shape<V_PLAIN>(shape, *cfg, stream, a, nullptr);
}

#if defined(H9G_COUNT_EXACT)
int h9g_exact_report(void) {
  unsigned long long cnt = 0;
  HIPCHK(hipMemcpyFromSymbol(&cnt, HIP_SYMBOL(h9g_exact_count), sizeof(cnt)));
  fprintf(stderr, "h9g exact re-runs (lanes, cumulative): %llu\n", cnt);
  std::vector<unsigned> w(1 << 16);
  HIPCHK(hipMemcpyFromSymbol(w.data(), HIP_SYMBOL(h9g_exact_wave), sizeof(unsigned) << 16));
  std::vector<std::pair<unsigned, int>> top;
  for (int i = 0; i < (1 << 16); i++)
    if (w[i]) top.push_back({w[i], i});
  std::sort(top.rbegin(), top.rend());
  fprintf(stderr, "h9g exact re-runs: %zu waves;", top.size());
  for (size_t k = 0; k < top.size() && k < 8; k++) fprintf(stderr, " w%d:%u", top[k].second, top[k].first);
  fprintf(stderr, "\n");
  return 0;
}
#endif

#if defined(H9G_COUNT_BRANCH)
int h9g_branch_report(void) {
  // waves entering each H9G_BR site per wave-substep since the last sync, and their mean active lanes
  static const char *names[BR_N] = {"substep", "theta", "qb", "eq_exact", "aqpow", "aq_s", "hk_exact", "tri_flux",
                                    "tri_sweep", "recharge", "baseflow", "watmin", "rerun", "powf_redo",
                                    "div_redo", "expf_redo", "powf_fix", "div_fix", "inl", "any_aq", "jwt_col",
                                    "visit2", "snap", "eb_exact", "day"};
  unsigned long long c[64];
  HIPCHK(hipMemcpyFromSymbol(c, HIP_SYMBOL(h9g_branch_count), sizeof(c)));
  const double ws = c[BR_SUBSTEP] ? (double)c[BR_SUBSTEP] : 1.0;
  fprintf(stderr, "h9g branch counts (wave entries per wave-substep, mean lanes):");
  for (int k = 0; k < BR_N; k++)
    if (c[k]) fprintf(stderr, " %s=%.4g/%.1f", names[k], c[k] / ws, (double)c[32 + k] / c[k]);
  fprintf(stderr, "\n");
  memset(c, 0, sizeof(c));
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(h9g_branch_count), c, sizeof(c)));
  return 0;
}
#endif

#if defined(H9G_DUMP_AQ)
int h9g_aq_set(unsigned *bits, const float *base, hipStream_t stream) {
  HIPCHK(hipMemcpyToSymbolAsync(HIP_SYMBOL(h9g_aq_bits), &bits, sizeof(void *), 0, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemcpyToSymbolAsync(HIP_SYMBOL(h9g_aq_base), &base, sizeof(void *), 0, hipMemcpyHostToDevice, stream));
  return 0;
}
#endif
