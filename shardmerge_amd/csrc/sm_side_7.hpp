// sm_side_7.hpp - group 7 of smhip_side.hip (smhip_device.hpp) draws on the headers of eight operators
#pragma once
#include "sm_ties.hpp"
#include "sm_dare.hpp"
#include "sm_breadcrumbs.hpp"
#include "sm_geo.hpp"
#include "sm_sphere.hpp"
#include "sm_sce.hpp"
#include "sm_della.hpp"
#include "sm_consensus.hpp"

#define SM_SIDE_KERNELS_7(X) SM_KERNELS_TIES(X) SM_KERNELS_DARE(X) SM_KERNELS_CRUMBS(X) SM_KERNELS_GEO(X) SM_KERNELS_SPHERE(X) \
    SM_KERNELS_SCE(X) SM_KERNELS_DELLA(X) SM_KERNELS_CONSENSUS(X)
