// smhip_device.hpp - DeviceExec (one real gfx950 work-group per block) and the
// generic __global__ entry point; shared by smhip_hip.hip, smhip_side.hip and smhip_inst.hip.
// Each kernel's tag stands at the end of the header that defines the kernel; which header each
// translation unit compiles from is listed at the end of this file.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "fft_engine.hpp"        // (static_for)

namespace smhip {

struct DeviceExec {
    template <class S> struct State { using value_type = S; S s; };
    __device__ __forceinline__ int bid() const { return blockIdx.x; }
    __device__ __forceinline__ int nthreads() const { return blockDim.x; }
    __device__ __forceinline__ int nblocks() const { return gridDim.x; }
    __device__ __forceinline__ float* lds() {
        extern __shared__ __attribute__((aligned(16))) float sm_dyn_lds[];
        return sm_dyn_lds;
    }
    template <class S> __device__ __forceinline__ void init(State<S>&) {}
    template <class S, class F> __device__ __forceinline__ void each(State<S>& st, F&& f) { f((int)threadIdx.x, st.s); }
    __device__ __forceinline__ void sync() { __syncthreads(); }
    __device__ __forceinline__ void lds_atomic_add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
    __device__ __forceinline__ uint32_t lds_atomic_add_ret(uint32_t* p, uint32_t v) { return atomicAdd(p, v); }
    __device__ __forceinline__ uint32_t global_atomic_add_ret_u32(uint32_t* p, uint32_t v) { return atomicAdd(p, v); }
    __device__ __forceinline__ void global_atomic_add(unsigned long long* p, unsigned long long v) { atomicAdd(p, v); }
    __device__ __forceinline__ void global_atomic_add_u32(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
    __device__ __forceinline__ void global_atomic_or_u32(uint32_t* p, uint32_t v) { atomicOr(p, v); }

    // dst(lane)[i] = src(lane + DELTA)[i], i < N dwords, inside the 64-lane wave (lanes past its end keep their own)
    template <int DELTA, int N, class S, class Src, class Dst>
    __device__ __forceinline__ void wave_shift_down(State<S>& st, Src src, Dst dst) {
        const uint32_t* a = src(st.s);
        uint32_t* b = dst(st.s);
#pragma unroll
        for (int i = 0; i < N; ++i) b[i] = (uint32_t)__shfl_down((int)a[i], DELTA, 64);
    }
    // Lanes t and t ^ 1 trade one float each, NP times: of the pair (a, b) that get(s, k) names, the even lane gives
    // its b and takes the partner's a into it, the odd lane gives its a and takes the partner's b into it (one select,
    // one quad-permute DPP move, two selects; no LDS).  get(S&, integral_constant<int, k>) -> {float& a, float& b}.
    template <int NP, class S, class Get>
    __device__ __forceinline__ void lane_pair_trade(State<S>& st, Get get) {
        const bool odd = (threadIdx.x & 1u) != 0;
        static_for<0, NP>([&](auto k_c) {
            auto pr = get(st.s, k_c);
            const float give = odd ? pr.a : pr.b;
            const float got = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, give), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
            pr.a = odd ? got : pr.a;
            pr.b = odd ? pr.b : got;
        });
    }
    // sum NV doubles (State::red) over the work-group; f(total) runs on thread 0.
    // Uses the first LDS_SCRATCH_FLOATS of LDS; ends with a barrier.
    template <int NV, class S, class F>
    __device__ __forceinline__ void block_sum(State<S>& st, F&& f) {
        double v[NV];
#pragma unroll
        for (int q = 0; q < NV; ++q) v[q] = st.s.red[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int q = 0; q < NV; ++q) v[q] += __shfl_down(v[q], off, 64);
        }
        double* scratch = (double*)lds();
        const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
        const int nw = (blockDim.x + 63) >> 6;
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < NV; ++q) scratch[wave * NV + q] = v[q];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double tot[NV];
#pragma unroll
            for (int q = 0; q < NV; ++q) tot[q] = 0.0;
            for (int w = 0; w < nw; ++w) {
#pragma unroll
                for (int q = 0; q < NV; ++q) tot[q] += scratch[w * NV + q];
            }
            f((const double*)tot);
        }
        __syncthreads();
    }
};

// Each kernel tag states its largest work-group (max_threads) and the waves per SIMD it
// is compiled for.  Default (1024, 4): at most 128 VGPRs.  The forward row pass is the
// one kernel that measured faster on MI355X with 3 waves per SIMD (168 VGPRs, no scratch
// spills, -10..-17 % time); the column passes lose 30 % that way and stay at 4.
template <class K>
__global__ void __launch_bounds__(K::max_threads, K::waves) sm_kernel(const typename K::Params p) {
    DeviceExec ex;
    K::run(ex, p);
}

// Every kernel is instantiated in exactly one translation unit and smhip_hip.hip holds host code only (it declares
// them all extern, and the Makefile fails the build if main.o defines one).  A kernel unit includes this header and the
// header its kernels come from, never the host orchestration (sm_pipeline.hpp, sm_delta_host.hpp, sm_capi.inc), and
// the Makefile rebuilds a unit when a file it includes changes: the build parallelises, a change to the host
// orchestration recompiles main.o alone, and a change to one operator's header that operator's group and main.o.
// The static-plan transform kernels: smhip_inst.hip, one translation unit per plan of SM_STATIC_PLANS (sm_plans.hpp).
#define SM_FFT_KERNELS_OF(X, ...)                      \
    X(KF1<__VA_ARGS__>) X(KF2<__VA_ARGS__>) X(KI1x1<__VA_ARGS__>) X(KI1x2<__VA_ARGS__>) X(KI2<__VA_ARGS__>) X(KF2S<__VA_ARGS__>) \
    X(KF1Q<__VA_ARGS__>) X(KF2Q<__VA_ARGS__>) X(KF2SQ<__VA_ARGS__>) X(KI1x1Q<__VA_ARGS__>) X(KI1x2Q<__VA_ARGS__>) \
    X(KPair1d<__VA_ARGS__>) X(KF1B<__VA_ARGS__>) X(KI2B<__VA_ARGS__>)
// Every other kernel: smhip_side.hip, one translation unit per group g (-DSM_SIDE_GROUP=<g>).  It includes
// SM_SIDE_HEADER_<g> and instantiates SM_SIDE_KERNELS_<g>, which that header states after its kernels' tags.
// (3 - 6 and 17 - 20 are SM_FFT_KERNELS_OF(X, DynPlan), the transforms of run-time planned lengths; the row passes
//  among them take a minute or more each to compile and stand one to a group.)
#define SM_SIDE_HEADER_0 "sm_aten_norm.hpp"      // the torch.norm emulation
#define SM_SIDE_HEADER_1 "sm_side_1.hpp"         // the selection and reduction kernels, the _r1 column passes
#define SM_SIDE_HEADER_2 "sm_side_2.hpp"         // the blend, norm, layout and element-wise kernels, the LoRA / DoRA update
#define SM_SIDE_HEADER_3 "sm_kernels.hpp"        // DynPlan: the forward row pass
#define SM_SIDE_HEADER_4 "sm_kernels.hpp"        // DynPlan: the forward column passes
#define SM_SIDE_HEADER_5 "sm_kernels.hpp"        // DynPlan: the inverse column passes
#define SM_SIDE_HEADER_6 "sm_bluestein.hpp"      // DynPlan: the forward row pass of a length without a plan
#define SM_SIDE_HEADER_7 "sm_side_7.hpp"         // the delta and geometric merges: TIES ... Consensus, a sub-list each
#define SM_SIDE_HEADER_8 "sm_stats.hpp"          // the task-vector statistics
#define SM_SIDE_HEADER_9 "sm_extract.hpp"        // the low-rank extraction
#define SM_SIDE_HEADER_10 "sm_fusion.hpp"        // the pairwise fusion
#define SM_SIDE_HEADER_11 "sm_pcb.hpp"           // the PCB merge
#define SM_SIDE_HEADER_12 "sm_tsv.hpp"           // the TSV merge
#define SM_SIDE_HEADER_13 "sm_widen.hpp"         // the WIDEN merge
#define SM_SIDE_HEADER_14 "sm_cabs.hpp"          // the CABS merge
#define SM_SIDE_HEADER_15 "sm_iso.hpp"           // the Iso-C merge
#define SM_SIDE_HEADER_16 "sm_dpack.hpp"         // the delta pack
#define SM_SIDE_HEADER_17 "sm_kernels.hpp"       // DynPlan: the folded forward row pass
#define SM_SIDE_HEADER_18 "sm_kernels.hpp"       // DynPlan: the inverse row pass
#define SM_SIDE_HEADER_19 "sm_kernels.hpp"       // DynPlan: the 1-D pair merge
#define SM_SIDE_HEADER_20 "sm_bluestein.hpp"     // DynPlan: the inverse row pass of a length without a plan
#define SM_SIDE_HEADER_21 "sm_emr.hpp"           // EMR-Merging: the unified model, a task's mask, its apply
#define SM_SIDE_HEADER_22 "sm_emr_fused.hpp"     // EMR-Merging: the unified model and every task's mask in one pass, their fold
// A new group: its SM_SIDE_HEADER_<g> and SM_SIDE_KERNELS_<g>, one more entry in SM_SIDE_KERNELS_ALL, and SM_SIDE_GROUPS
// (the Makefile reads it).
#define SM_SIDE_GROUPS 23
#define SM_SIDE_KERNELS_ALL(X)                                                                                       \
    SM_SIDE_KERNELS_0(X) SM_SIDE_KERNELS_1(X) SM_SIDE_KERNELS_2(X) SM_SIDE_KERNELS_3(X) SM_SIDE_KERNELS_4(X) SM_SIDE_KERNELS_5(X)     \
    SM_SIDE_KERNELS_6(X) SM_SIDE_KERNELS_7(X) SM_SIDE_KERNELS_8(X) SM_SIDE_KERNELS_9(X) SM_SIDE_KERNELS_10(X) SM_SIDE_KERNELS_11(X)   \
    SM_SIDE_KERNELS_12(X) SM_SIDE_KERNELS_13(X) SM_SIDE_KERNELS_14(X) SM_SIDE_KERNELS_15(X) SM_SIDE_KERNELS_16(X) SM_SIDE_KERNELS_17(X) \
    SM_SIDE_KERNELS_18(X) SM_SIDE_KERNELS_19(X) SM_SIDE_KERNELS_20(X) SM_SIDE_KERNELS_21(X) SM_SIDE_KERNELS_22(X)

}  // namespace smhip
