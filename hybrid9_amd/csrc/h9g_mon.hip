// h9g_mon.hip -- the monthly kernels' translation unit: h9g.hip's year
// kernel code instantiated with the Months policy (h9g_pair.h) under the
// monthly kernels' names, and h9g_mon_launch.  A unit of its own so that it
// compiles beside h9g.hip (hybrid9_amd/build.py), not after it.
#define H9G_MONTHLY_UNIT 1
// (the math tables' device copies: one per unit)
#define c_exp2tab c_exp2tab_mon
#define c_log2tab c_log2tab_mon
#include "h9g.hip"
