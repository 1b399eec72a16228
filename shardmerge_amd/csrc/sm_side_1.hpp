// sm_side_1.hpp - group 1 of smhip_side.hip (smhip_device.hpp) draws on two headers
#pragma once
#include "sm_kernels.hpp"
#include "sm_select.hpp"

#define SM_SIDE_KERNELS_1(X) SM_KERNELS_R1(X) SM_KERNELS_SELECT(X)
