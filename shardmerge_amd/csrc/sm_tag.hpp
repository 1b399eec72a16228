// sm_tag.hpp - the kernel tag macros.  A tag names one kernel: its parameter struct, its profile name, the call of its
// body, its largest work-group (max_threads) and the waves per SIMD its registers are budgeted for; sm_kernel<Tag>
// (smhip_device.hpp) is the __global__ entry point and Backend::launch<Tag> starts it.  Each header states the tags of
// the kernels it defines at its end, and after them the list of what it gives to the groups of smhip_side.hip.
#pragma once
#include "fft_engine.hpp"

namespace smhip {

// a kernel with explicit launch bounds (work-group size limit, waves per SIMD the registers are budgeted for)
#define SM_KERNEL_TAG_LB(Tag, ParamsT, NAME, CALL, MAXT, WAVES)                      \
    struct Tag {                                                                     \
        using Params = ParamsT;                                                      \
        static constexpr int waves = WAVES;                                          \
        static constexpr int max_threads = MAXT;                                     \
        static const char* name() { return NAME; }                                   \
        template <class Ex> static SM_HD void run(Ex& ex, const Params& p) { CALL; } \
    };
// the default: any work-group size, at most 128 VGPRs
#define SM_KERNEL_TAG(Tag, ParamsT, NAME, CALL) SM_KERNEL_TAG_LB(Tag, ParamsT, NAME, CALL, 1024, 4)

// the transform kernels exist once per static plan plus once for DynPlan
template <class P, int GROUPS> constexpr int fft_max_threads() {
    if constexpr (P::is_static) return (GROUPS * P::T < 256) ? 256 : (GROUPS * P::T > 1024 ? 1024 : GROUPS * P::T);
    else return 1024;
}
#ifndef SM_W3_MAX_THREADS
#define SM_W3_MAX_THREADS 256
#endif
#define SM_FFT_KERNEL_TAG(Tag, ParamsT, NAME, CALL, GROUPS, WAVES)                   \
    template <class P> struct Tag {                                                  \
        using Params = ParamsT;                                                      \
        static constexpr int waves = (WAVES < 4 && P::is_static && fft_max_threads<P, GROUPS>() <= SM_W3_MAX_THREADS) ? WAVES : 4; \
        static constexpr int max_threads = waves < 4 ? fft_max_threads<P, GROUPS>() : 1024; \
        static const char* name() { return NAME; }                                   \
        template <class Ex> static SM_HD void run(Ex& ex, const Params& p) { CALL; } \
    };
// row passes of a row length without a plan (sm_bluestein.hpp); P is the plan of the convolution length
// (one transform per work-group and two of them back to back: compiled for two waves per SIMD - 256 VGPRs - where
//  the work-group allows it; at 128 the 16384-point convolution kept 700 bytes per lane in scratch)
#define SM_BLUE_KERNEL_TAG(Tag, ParamsT, NAME, CALL)                                 \
    template <class P> struct Tag {                                                  \
        using Params = ParamsT;                                                      \
        static constexpr int max_threads = fft_max_threads<P, 1>();                  \
        static constexpr int waves = max_threads > 512 ? 4 : 2;                      \
        static const char* name() { return NAME; }                                   \
        template <class Ex> static SM_HD void run(Ex& ex, const Params& p) { CALL; } \
    };

}  // namespace smhip
