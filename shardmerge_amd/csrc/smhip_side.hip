// smhip_side.hip - explicit instantiation of one group of kernels, selected with -DSM_SIDE_GROUP=<g>: the kernels
// SM_SIDE_KERNELS_<g> of the header SM_SIDE_HEADER_<g> (the groups: the end of smhip_device.hpp).
#include "smhip_device.hpp"

#if !defined(SM_SIDE_GROUP) || SM_SIDE_GROUP < 0 || SM_SIDE_GROUP >= SM_SIDE_GROUPS
#error "SM_SIDE_GROUP must be 0 .. SM_SIDE_GROUPS - 1"
#endif

#define SM_PASTE_(a, b) a##b
#define SM_PASTE(a, b) SM_PASTE_(a, b)
#include SM_PASTE(SM_SIDE_HEADER_, SM_SIDE_GROUP)

namespace smhip {
#define SM_INST(...) template __global__ void sm_kernel<__VA_ARGS__>(const typename __VA_ARGS__::Params);
SM_PASTE(SM_SIDE_KERNELS_, SM_SIDE_GROUP)(SM_INST)
}  // namespace smhip
