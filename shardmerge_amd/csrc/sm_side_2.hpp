// sm_side_2.hpp - group 2 of smhip_side.hip (smhip_device.hpp) draws on two headers
#pragma once
#include "sm_merge.hpp"
#include "sm_lora.hpp"

#define SM_SIDE_KERNELS_2(X) SM_KERNELS_MERGE(X) SM_KERNELS_LORA(X)
