// h9g_et.hip -- the evapotranspiration (ET) kernels' translation unit: the
// year kernels of h9g_year.h instantiated with the EvapProf and MonthsEt
// policies (h9g_pair.h) under the ET kernels' names, behind h9g_et_launch.
// A unit of its own so that it compiles beside h9g_plain.hip and h9g_mon.hip
// (hybrid9_amd/build.py), not after them.
#include "h9g_year.h"

// mon: the base of the launch's monthly rows, or null (no monthly recording).
int h9g_et_launch(Shape shape, const h9g_config *cfg, hipStream_t stream, const KArgs &a, float *mon) {
  return launch_shape<V_ET>(shape, *cfg, stream, a, mon);
}
