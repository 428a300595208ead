// TEST INFRASTRUCTURE ONLY: the layer expressions (hybrid9_amd/csrc/h9g_expr.h)
// on the host, for tests/test_expr.py: the fast forms next to the exact forms
// that hydrology_pair's exact lambdas state (hk_exact, eq_exact), here with
// plain divisions.  Never linked into the product library.
#include <stdint.h>
#include "../../hybrid9_amd/csrc/h9g_expr.h"

using namespace h9k;

// s1 of layers with theta(i), theta(ip), ts(i), ts(ip): the Markstein quotient
// from PF_ITS = one / (ts + tsp) (cell_inv_pair) and its flag, unclamped and
// clamped, against hk_exact's 0.5f * (th + thp) / (0.5f * (ts + tsp)).
extern "C" void h9k_expr_s1(int n, const float *th, const float *thp, const float *ts, const float *tsp,
                            float *fast, float *fast_min, int *flag, float *exact, float *exact_min) {
  for (int k = 0; k < n; k++) {
    const float its = one / (ts[k] + tsp[k]);
    bool b0 = false, b1 = false;
    fast[k] = s1_quot_mk(th[k] + thp[k], ts[k] + tsp[k], its, b0);
    fast_min[k] = s1_mk(th[k] + thp[k], ts[k] + tsp[k], its, b1);
    flag[k] = (b0 ? 1 : 0) | (b1 ? 2 : 0);
    const float s1 = 0.5f * (th[k] + thp[k]) / (0.5f * (ts[k] + tsp[k]));
    exact[k] = s1;
    exact_min[k] = MINC(one, s1);
  }
}

// vol_eq with the water table zw inside the layer (zlo, zhi): the branch-free
// form and its flag against eq_exact's, which divides by zw - zlo and by
// zhi - zlo = dz(i).
extern "C" void h9k_expr_vol_in(int n, const float *pte, const float *ts, const float *temp0, const float *zw,
                                const float *zlo, const float *zhi, float *fast, int *flag, float *exact) {
  MathFast m{};
  for (int k = 0; k < n; k++) {
    bool b = false;
    const float dz = zhi[k] - zlo[k];
    fast[k] = vol_eq_in_fast(m, [&]() { return pte[k]; }, ts[k], temp0[k], zw[k], zlo[k], zhi[k],
                             [&]() { return 1.0 / (double)dz; }, true, b);
    flag[k] = b;
    const float tempi = one;
    const float voleq1 = pte[k] / (zw[k] - zlo[k]) * (tempi - temp0[k]);
    float v = (voleq1 * (zw[k] - zlo[k]) + ts[k] * (zhi[k] - zw[k])) / (zhi[k] - zlo[k]);
    v = MINF(ts[k], v);
    v = MAXF(v, zero);
    exact[k] = v;
  }
}
