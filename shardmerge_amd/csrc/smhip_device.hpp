// smhip_device.hpp - DeviceExec (one real gfx950 work-group per block) and the
// generic __global__ entry point; shared by smhip_hip.hip, smhip_side.hip and smhip_inst.hip.
// Each kernel's tag stands at the end of the header that defines the kernel; what each
// translation unit instantiates is listed at the end of this file.
#pragma once
#include <hip/hip_runtime.h>

#include "sm_pipeline.hpp"

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
// them all extern, and the Makefile fails the build if main.o defines one): the build parallelises and a change to the
// host orchestration does not recompile a single kernel.
// The static-plan transform kernels: smhip_inst.hip, one translation unit per plan of SM_STATIC_PLANS (sm_pipeline.hpp).
#define SM_FFT_KERNELS_OF(X, ...)                      \
    X(KF1<__VA_ARGS__>) X(KF2<__VA_ARGS__>) X(KI1x1<__VA_ARGS__>) X(KI1x2<__VA_ARGS__>) X(KI2<__VA_ARGS__>) X(KF2S<__VA_ARGS__>) \
    X(KF1Q<__VA_ARGS__>) X(KF2Q<__VA_ARGS__>) X(KF2SQ<__VA_ARGS__>) X(KI1x1Q<__VA_ARGS__>) X(KI1x2Q<__VA_ARGS__>) \
    X(KPair1d<__VA_ARGS__>) X(KF1B<__VA_ARGS__>) X(KI2B<__VA_ARGS__>)
// Every other kernel: smhip_side.hip, one translation unit per group g (-DSM_SIDE_GROUP=<g>) of SM_SIDE_KERNELS_<g>,
// which the header that defines the group's kernels states after their tags.  The groups:
//    0  the torch.norm emulation (sm_aten_norm.hpp)
//    1  the selection and reduction kernels of the spectral pipeline (sm_kernels.hpp)
//    2  its blend, norm, layout and element-wise kernels (sm_kernels.hpp) and the LoRA / DoRA update (sm_lora.hpp)
//    3 - 6  the transform kernels for run-time planned lengths, SM_FFT_KERNELS_OF(X, DynPlan) in four parts
//       (sm_kernels.hpp; 6, the row passes of a length without a plan: sm_bluestein.hpp)
//    7  the delta and geometric merges: TIES, DARE, Breadcrumbs, Model Stock / SLERP / NuSLERP, the Karcher-mean merges,
//       SCE, DELLA and Consensus (sm_ties.hpp .. sm_consensus.hpp, a sub-list each)
//    8  the task-vector statistics (sm_stats.hpp)       9  the low-rank extraction (sm_extract.hpp)
//   10  the pairwise fusion (sm_fusion.hpp)            11  the PCB merge (sm_pcb.hpp)
//   12  the TSV merge (sm_tsv.hpp)                     13  the WIDEN merge (sm_widen.hpp)
//   14  the CABS merge (sm_cabs.hpp)                   15  the Iso-C merge (sm_iso.hpp)
//   16  the delta pack (sm_dpack.hpp)
// A new group: its SM_SIDE_KERNELS_<g>, one more entry in SM_SIDE_KERNELS_ALL, and SM_SIDE_GROUPS (the Makefile reads it).
#define SM_SIDE_KERNELS_2(X) SM_KERNELS_MERGE(X) SM_KERNELS_LORA(X)
#define SM_SIDE_KERNELS_7(X) SM_KERNELS_TIES(X) SM_KERNELS_DARE(X) SM_KERNELS_CRUMBS(X) SM_KERNELS_GEO(X) SM_KERNELS_SPHERE(X) \
    SM_KERNELS_SCE(X) SM_KERNELS_DELLA(X) SM_KERNELS_CONSENSUS(X)
#define SM_SIDE_GROUPS 17
#define SM_SIDE_KERNELS_ALL(X)                                                                                       \
    SM_SIDE_KERNELS_0(X) SM_SIDE_KERNELS_1(X) SM_SIDE_KERNELS_2(X) SM_SIDE_KERNELS_3(X) SM_SIDE_KERNELS_4(X) SM_SIDE_KERNELS_5(X)     \
    SM_SIDE_KERNELS_6(X) SM_SIDE_KERNELS_7(X) SM_SIDE_KERNELS_8(X) SM_SIDE_KERNELS_9(X) SM_SIDE_KERNELS_10(X) SM_SIDE_KERNELS_11(X)   \
    SM_SIDE_KERNELS_12(X) SM_SIDE_KERNELS_13(X) SM_SIDE_KERNELS_14(X) SM_SIDE_KERNELS_15(X) SM_SIDE_KERNELS_16(X)

}  // namespace smhip
