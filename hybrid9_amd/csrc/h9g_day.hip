// h9g_day.hip -- the day-record kernels' translation unit: the year kernels of
// h9g_year.h instantiated with the EvapProf and DaysEt policies (h9g_pair.h)
// under the day kernels' names, behind h9g_day_launch.  A unit of its own so
// that it compiles beside h9g_plain.hip, h9g_mon.hip and h9g_et.hip
// (hybrid9_amd/build.py), not after them.
#include "h9g_year.h"

// mon: the base of the launch's monthly rows, or null (no monthly recording);
// day: the base of its day rows, or null (nothing recorded).
int h9g_day_launch(Shape shape, const h9g_config *cfg, hipStream_t stream, const KArgs &a, float *mon, float *day) {
  return launch_shape<V_DAY>(shape, *cfg, stream, a, mon, day);
}
