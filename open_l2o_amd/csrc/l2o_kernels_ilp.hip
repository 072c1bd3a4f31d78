// l2o_kernels_ilp.hip -- the max-ilp translation unit of libl2o_hip.so: the kernels listed in l2o_ilp_kernels.h, compiled with
// -mllvm -amdgpu-sched-strategy=max-ilp (csrc/Makefile).  That header pulls in the templates it instantiates and what they
// need; no C-ABI entry point, no other kernel is emitted here.
#define L2O_TU_ILP 1
#include "l2o_ilp_kernels.h"
