// fcx_kernels_wide.hip -- the F32Wide instantiations of the cell kernels (FCX_OPT_F32_MATH:
// float arrays, double arithmetic, one rounding per stored value) as a translation unit of
// their own, compiled beside fcx_kernels.hip.  The kernels are the templates of that file,
// instantiated with the precision F32Wide; nothing is written twice.  This unit holds the
// wide siblings of every fp32 instantiation (cells_kernel: generic and VAR 1-3, one type,
// several, register averages, merged and separate grids, 4 cells and 1 cell per lane;
// cells_atmos_kernel with crossing records, with halo tiles and, for several types, with the
// register averages; cells_atmos_group_kernel for one type and for several;
// kWideCpl = 2 cells per lane) and the three launchers the other unit calls
// (launch_wide_fused / _cells / _group).
#define FCX_KERNELS_WIDE_TU 1
#include "fcx_kernels.hip"
