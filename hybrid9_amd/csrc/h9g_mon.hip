// h9g_mon.hip -- the monthly kernels' translation unit: the year kernels of
// h9g_year.h instantiated with the Months policy (h9g_pair.h) under the
// monthly kernels' names, behind h9g_mon_launch.  A unit of its own so that it
// compiles beside h9g_plain.hip (hybrid9_amd/build.py), not after it.
#include "h9g_year.h"

// The cell order: the cells that start a decade stopped (err0) run none
// of its years; all their recorded rows of the decade (`rows` of n: months
// or day records, h9g_nan_stopped_rows) are NaN.
__global__ void __launch_bounds__(256) h9g_stopped_mon_kernel(int n, int rows, const int *__restrict__ err0,
                                                              float *__restrict__ mon) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n || err0[c] == 0) return;
  for (int r = 0; r < rows; r++) mon[(size_t)r * n + c] = __builtin_nanf("");
}

int h9g_nan_stopped_rows(int n, int rows, const int *err0, float *dst, hipStream_t stream) {
  h9g_stopped_mon_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(n, rows, err0, dst);
  return 0;
}

int h9g_mon_launch(Shape shape, const h9g_config *cfg, hipStream_t stream, const KArgs &a, float *mon) {
  return launch_shape<V_MON>(shape, *cfg, stream, a, mon);
}
