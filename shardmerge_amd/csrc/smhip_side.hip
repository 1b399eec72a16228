// smhip_side.hip - explicit instantiation of one group of kernels, selected with -DSM_SIDE_GROUP=<g>
// (SM_SIDE_KERNELS_<g>: groups 0..2 in sm_pipeline.hpp, 7..16 in sm_delta_host.hpp; groups 3..6: the transform kernels for run-time planned lengths, 7: the delta and geometric merges, 8: the task-vector statistics, 9: the low-rank extraction, 10: the pairwise fusion, 11: the PCB merge, 12: the TSV merge, 13: the WIDEN merge, 14: the CABS merge, 15: the Iso-C merge, 16: the delta pack).
#include "smhip_device.hpp"

namespace smhip {
#define SM_INST(...) template __global__ void sm_kernel<__VA_ARGS__>(const typename __VA_ARGS__::Params);
#if SM_SIDE_GROUP == 0
SM_SIDE_KERNELS_0(SM_INST)
#elif SM_SIDE_GROUP == 1
SM_SIDE_KERNELS_1(SM_INST)
#elif SM_SIDE_GROUP == 2
SM_SIDE_KERNELS_2(SM_INST)
#elif SM_SIDE_GROUP == 3
SM_INST(KF1<DynPlan>) SM_INST(KF1Q<DynPlan>) SM_INST(KI2<DynPlan>) SM_INST(KPair1d<DynPlan>)
#elif SM_SIDE_GROUP == 4
SM_INST(KF2<DynPlan>) SM_INST(KF2Q<DynPlan>) SM_INST(KF2S<DynPlan>) SM_INST(KF2SQ<DynPlan>)
#elif SM_SIDE_GROUP == 5
SM_INST(KI1x1<DynPlan>) SM_INST(KI1x2<DynPlan>) SM_INST(KI1x1Q<DynPlan>) SM_INST(KI1x2Q<DynPlan>)
#elif SM_SIDE_GROUP == 6
SM_INST(KF1B<DynPlan>) SM_INST(KI2B<DynPlan>)
#elif SM_SIDE_GROUP == 7
SM_SIDE_KERNELS_7(SM_INST)
#elif SM_SIDE_GROUP == 8
SM_SIDE_KERNELS_8(SM_INST)
#elif SM_SIDE_GROUP == 9
SM_SIDE_KERNELS_9(SM_INST)
#elif SM_SIDE_GROUP == 10
SM_SIDE_KERNELS_10(SM_INST)
#elif SM_SIDE_GROUP == 11
SM_SIDE_KERNELS_11(SM_INST)
#elif SM_SIDE_GROUP == 12
SM_SIDE_KERNELS_12(SM_INST)
#elif SM_SIDE_GROUP == 13
SM_SIDE_KERNELS_13(SM_INST)
#elif SM_SIDE_GROUP == 14
SM_SIDE_KERNELS_14(SM_INST)
#elif SM_SIDE_GROUP == 15
SM_SIDE_KERNELS_15(SM_INST)
#elif SM_SIDE_GROUP == 16
SM_SIDE_KERNELS_16(SM_INST)
#else
#error "SM_SIDE_GROUP must be 0..16"
#endif
}  // namespace smhip
