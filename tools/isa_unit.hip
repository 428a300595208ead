// isa_unit.hip -- tools/isa_pair.sh: device code of single year kernels alone
// (ISA study): the config-2 pair and one-column kernels, or with
// -DH9G_ISA_L10 the L = 10 pair kernels.
#include "../hybrid9_amd/csrc/h9g_year.h"

#if defined(H9G_ISA_L10)
template __global__ void h9g_pair_kernel<10, GeoC<10, 24>>(const KArgs, const GeoC<10, 24>);
template __global__ void h9g_pair2_kernel<10, GeoC<10, 24>>(const KArgs, const GeoC<10, 24>);
template __global__ void h9g_pair11_kernel<10, GeoC<10, 24>>(const KArgs, const GeoC<10, 24>);
#else
template __global__ void h9g_pair1_kernel<8, GeoC<8, 48>>(const KArgs, const GeoC<8, 48>);
template __global__ void h9g_pair_kernel<8, GeoC<8, 48>>(const KArgs, const GeoC<8, 48>);
#endif
