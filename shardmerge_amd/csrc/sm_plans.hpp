// sm_plans.hpp - the static plans: the lengths whose transform kernels are compiled straight-line, one translation
// unit per plan (smhip_inst.hip), and which the host planner (sm_pipeline.hpp) knows by the same list.
#pragma once
#include "fft_engine.hpp"

namespace smhip {

// lengths that get straight-line kernels (powers of two, the 7 * 2^k of Llama-3 / Mixtral MLPs,
// the 3/5/7 * 2^k hidden and MLP sizes of other common models, and 256 / 512: the row blocks of the
// split column lengths 11008 = 43 * 256 (Llama-2-7B), 18944 = 37 * 512 (Qwen2-7B), 4544 = 71 * 64 and 4672 = 73 * 64
// (Falcon-7B: as run-time plans its 64-point blocks took 9 + 12 ms per 4544^2 pair merge): a run-time planned length
// runs the same code with its register arrays in scratch memory, 5120^2: 5.4 ms against 0.7);
// must agree with plan_shape() (sm_pipeline.hpp)
// (checked at dispatch: a mismatch silently falls back to the DynPlan kernel)
// experiment knobs for the 8192-point plan (override with -D on the hipcc line)
#ifndef SM_R14336
#define SM_R14336 16, 16, 8, 7
#endif
#ifndef SM_R7168
#define SM_R7168 32, 32, 7          // measured on MI355X as the folded column plan: 16,16,4,7 is 8 % slower
#endif
#ifndef SM_T8192
#define SM_T8192 256
#define SM_W8192 4
#define SM_R8192 32, 16, 16
#endif
// third parameter: complex (float2) LDS exchanges; plan_uses_cx() must agree
#define SM_STATIC_PLANS(X)                 \
    X(SPlan<1024, 64, false, 4, 32, 32>)       \
    X(SPlan<2048, 64, false, 4, 16, 16, 8>)    \
    X(SPlan<4096, 128, false, 4, 16, 16, 16>)  \
    X(SPlan<8192, SM_T8192, false, SM_W8192, SM_R8192>)  \
    X(SPlan<16384, 512, false, 4, 32, 32, 16>)\
    X(SPlan<14336, 512, false, 4, SM_R14336>) \
    X(SPlan<28672, 1024, false, 4, 16, 16, 16, 7>) \
    X(SPlan<3072, 128, false, 4, 16, 16, 4, 3>)    \
    X(SPlan<3584, 128, false, 4, 16, 32, 7>)       \
    X(SPlan<5120, 256, false, 4, 16, 16, 4, 5>)    \
    X(SPlan<6144, 256, false, 4, 16, 16, 8, 3>)    \
    X(SPlan<7168, 256, false, 4, SM_R7168>)    \
    X(SPlan<12288, 512, false, 4, 16, 16, 16, 3>)  \
    X(SPlan<13824, 512, false, 4, 32, 16, 3, 3, 3>) \
    X(SPlan<27648, 1024, false, 4, 32, 32, 3, 3, 3>) \
    X(SPlan<2304, 128, false, 4, 16, 16, 3, 3>) \
    X(SPlan<256, 64, false, 4, 8, 8, 4>)            \
    X(SPlan<512, 64, false, 4, 32, 16>)             \
    X(SPlan<64, 64, false, 4, 8, 8>)                \
    X(SPlan<128, 64, false, 4, 16, 8>)

// measured on MI355X (8192^2): the complex exchange halves occupancy and brings spills back -
// 1.6x slower than split exchanges, so no plan uses it for now
inline bool plan_uses_cx(int N) { (void)N; return false; }

}  // namespace smhip
