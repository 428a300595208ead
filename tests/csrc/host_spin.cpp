// TEST INFRASTRUCTURE ONLY: the host (CPU) build of the spin-up test
// (hybrid9_amd/csrc/h9g_spin.h: a cell's keys, their drift over a cycle and
// the decision), the lines h9g_spin_kernel runs per cell, used by
// tests/test_spinup_host.py against the rule restated in numpy
// (tests/spinup_helpers.py).  Never linked into the product library.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../hybrid9_amd/csrc/h9g_geo.h"
#include "../../hybrid9_amd/csrc/h9g_step.h"
#include "../../hybrid9_amd/csrc/h9g_pair.h"
#include "../../hybrid9_amd/csrc/h9g_rows.h"
#include "../../hybrid9_amd/csrc/h9g_spin.h"

using namespace h9k;

// prev, cur: packed states (include/h9g.h) of n cells one cycle apart.  keys
// (2, 3, n): W, zwt, pm of prev and of cur; drift (3, n): d_w, d_z, d_p;
// met (n): the decision at cycle k; maxima (3): over every cell, as the
// kernel accumulates them.
extern "C" int h9k_host_spin(int n, int L, const float *prev, const float *cur, int k, int min_cycles,
                             double tol_water, double tol_zwt, double tol_plant, double *keys, double *drift,
                             int *met, double *maxima) {
  if (n < 1 || (L != 8 && L != 10)) return -1;
  const size_t nn = (size_t)n, srows = (size_t)state_rows(L);
  std::vector<float> a(srows * nn), b(srows * nn);
  state_rows_from_packed(L, nn, prev, a.data());
  state_rows_from_packed(L, nn, cur, b.data());
  const SpinTol tol = {min_cycles, tol_water, tol_zwt, tol_plant};
  maxima[0] = maxima[1] = maxima[2] = 0.0;
  for (size_t c = 0; c < nn; c++) {
    const SpinKey ka = spin_key(a.data(), nn, c, L), kb = spin_key(b.data(), nn, c, L);
    const SpinKey d = spin_drift(ka, kb);
    const double kv[6] = {ka.w, ka.zwt, ka.pm, kb.w, kb.zwt, kb.pm}, dv[3] = {d.w, d.zwt, d.pm};
    for (int j = 0; j < 6; j++) keys[(size_t)j * nn + c] = kv[j];
    for (int j = 0; j < 3; j++) {
      drift[(size_t)j * nn + c] = dv[j];
      maxima[j] = spin_max(maxima[j], dv[j]);
    }
    met[c] = spin_settled(d, k, tol) ? 1 : 0;
  }
  return 0;
}

// The soil mask as the kernel reads it from packed parameters (h9g_set_params' order).
extern "C" void h9k_host_spin_soil(int n, int L, const float *par, int *soil) {
  std::vector<float> rows((size_t)par_rows(L) * n);
  par_rows_from_packed(L, (size_t)n, par, rows.data());
  for (int c = 0; c < n; c++) soil[c] = spin_soil(rows.data(), (size_t)n, (size_t)c, L) ? 1 : 0;
}
