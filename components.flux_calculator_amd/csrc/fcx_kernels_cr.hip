// fcx_kernels_cr.hip -- the F64Cr instantiations of the cell kernels (FCX_OPT_CR_MATH: double
// arrays, double arithmetic, the exp of QSUR and of RCO's MEVA and the Exner power correctly
// rounded by fcx_crmath.h) as a translation unit of their own, compiled beside fcx_kernels.hip
// and fcx_kernels_wide.hip.  The kernels are the templates of fcx_kernels.hip, instantiated
// with the precision F64Cr; nothing is written twice.  This unit holds the sibling of every
// fp64 instantiation (cells_kernel: generic and VAR 1-3, one type, several, register
// averages, merged and separate grids, 2 cells and 1 cell per lane, the record form;
// cells_atmos_kernel with crossing records, halo tiles, dense records, remap records and the
// register averages; cells_atmos_group_kernel for one type and for several) and the four
// launchers the other unit calls (launch_cr_fused / _cells / _rec / _group).
#define FCX_KERNELS_CR_TU 1
#include "fcx_kernels.hip"
