// kf_kernels.hip -- gfx950 kernels of the covariance / gain recursion of the time-varying KalmanFilter (bodies:
// kf_cov_bodies.h) and of the steady-state Riccati solve of the SteadyKalmanFilter (k_kf_dare<NX>, k_kf_dare_wide<NX>, the
// same families; body: kf_dare_bodies.h, whose square-root form is k_kf_dare_psd<NX>, k_kf_dare_psd_wide<NX>).  One
// wavefront per workgroup, persistent grid, the same split as the MovingHorizonEstimator:
//   k_kf_cov<NX>,      NX = 4, 8, 12, 16: max(nx̂, nym) <= 16, four estimators per wavefront (one per DPP row, MheDevWave);
//   k_kf_cov_wide<NX>, NX = 24, 32: 16 < max(nx̂, nym) <= 32, one estimator per wavefront, the NX^3 products on the
//                      matrix cores through the LDS staging buffer of Ops::mm_staged.
#include <hip/hip_runtime.h>

#include "kf_cov_bodies.h"
#include "kf_cov_launch.h"
#include "kf_dare_bodies.h"
#include "kf_dare_launch.h"
#include "kf_dare_psd_bodies.h"
#include "mhe_devwave.h"
#include "mhe_dispatch.h"
#include "mhe_wide_devwave.h"
#include "mpcqp_launch.h"

namespace mpcqp {
namespace kf {

using mhe::MheDevWave;
using WideWave = mhe::MheWideMfmaWave;

// the wave of a kernel: 16-lane rows, or the whole wavefront with the staging buffer of its products in the dynamic LDS
template <class W>
__device__ __forceinline__ W make_wave() {
    if constexpr (std::is_same<W, WideWave>::value) {
        WideWave w;
        w.lane = (int)threadIdx.x;
        w.stage = mpcqp_smem;
        return w;
    } else {
        return MheDevWave{(int)threadIdx.x};
    }
}

// launch(Cols<NX>, dynamic LDS bytes) for the register columns of the arguments, on their persistent grid: `launch` picks
// its narrow or its wide kernel by NX > mhe::RL
template <class F>
static hipError_t launch_for(int NX, F launch) {
    const hipError_t e = mhe::dispatch_nx<mhe::NX_NARROW | mhe::NX_WIDE>(NX, [&](auto nx) {
        launch(nx, decltype(nx)::value > mhe::RL ? mhe::stage_doubles() * sizeof(double) : (size_t)0);
    });
    return e != hipSuccess ? e : hipGetLastError();
}

template <int NX>
__global__ __launch_bounds__(64) void k_kf_cov(CovArgs a, int mode) {
    MheDevWave w = make_wave<MheDevWave>();
    kf_cov_body<MheDevWave, NX>(w, a, mode, (int)blockIdx.x);
}
// (registers: five rows of NX doubles, 320 at NX = 32 -- one wavefront per SIMD)
template <int NX>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8))) void k_kf_cov_wide(CovArgs a, int mode) {
    WideWave w = make_wave<WideWave>();
    kf_cov_body<WideWave, NX>(w, a, mode, (int)blockIdx.x);
}

hipError_t launch_kf_cov(const CovArgs& a, int mode, hipStream_t st) {
    if (!kf_cov_args_ok(a)) return hipErrorInvalidValue;
    return launch_for(a.NX, [&](auto nx, size_t lds) {
        constexpr int NX = decltype(nx)::value;
        if constexpr (NX > mhe::RL) hipLaunchKernelGGL(k_kf_cov_wide<NX>, dim3(a.nwaves), dim3(WAVE), lds, st, a, mode);
        else hipLaunchKernelGGL(k_kf_cov<NX>, dim3(a.nwaves), dim3(WAVE), lds, st, a, mode);
    });
}

// The grid: registers allow two wavefronts per SIMD for the 16-lane kernels (eight per CU), one for the wide ones (four per
// CU; their 16.5 KB of staging would allow nine).
int kf_cov_waves_for(int device, int B, int NX) {
    int cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    const bool wide = NX > mhe::RL;
    const int groups = wide ? B : (B + mhe::GPW - 1) / mhe::GPW;
    const int cap = cus * (wide ? 4 : 8);
    return groups < cap ? groups : cap;
}

// ---- steady-state gain from Q̂ and R̂ (once per model, not per period).  Seven rows of NX doubles stay in registers over
// the iterations: the wide kernels spill (lib/isa_resources.txt), which a solve per model swap can afford.
template <int NX>
__global__ __launch_bounds__(64) void k_kf_dare(DareArgs a) {
    MheDevWave w = make_wave<MheDevWave>();
    kf_dare_body<MheDevWave, NX>(w, a, (int)blockIdx.x);
}
template <int NX>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8))) void k_kf_dare_wide(DareArgs a) {
    WideWave w = make_wave<WideWave>();
    kf_dare_body<WideWave, NX>(w, a, (int)blockIdx.x);
}

hipError_t launch_kf_dare(const DareArgs& a, hipStream_t st) {
    if (!kf_dare_args_ok(a)) return hipErrorInvalidValue;
    return launch_for(a.NX, [&](auto nx, size_t lds) {
        constexpr int NX = decltype(nx)::value;
        if constexpr (NX > mhe::RL) hipLaunchKernelGGL(k_kf_dare_wide<NX>, dim3(a.nwaves), dim3(WAVE), lds, st, a);
        else hipLaunchKernelGGL(k_kf_dare<NX>, dim3(a.nwaves), dim3(WAVE), lds, st, a);
    });
}

// the grid of the covariance kernels: what is not resident at once queues behind what is
int kf_dare_waves_for(int device, int B, int NX) { return kf_cov_waves_for(device, B, NX); }

// ---- the second pass: the square-root form of the same iteration for the estimators the first pass left broken down (a
// semidefinite Q̂) or whose Q̂ is numerically singular.  The same grid and the same seven rows; every wavefront reads and
// factors the Q̂ of its estimators and their status words, and one without a candidate votes once and moves on.  (Spills:
// lib/isa_resources.txt -- accepted as above.)
template <int NX>
__global__ __launch_bounds__(64) void k_kf_dare_psd(DareArgs a) {
    MheDevWave w = make_wave<MheDevWave>();
    kf_dare_psd_body<MheDevWave, NX>(w, a, (int)blockIdx.x);
}
template <int NX>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8))) void k_kf_dare_psd_wide(DareArgs a) {
    WideWave w = make_wave<WideWave>();
    kf_dare_psd_body<WideWave, NX>(w, a, (int)blockIdx.x);
}

hipError_t launch_kf_dare_psd(const DareArgs& a, hipStream_t st) {
    if (!kf_dare_args_ok(a) || !a.path) return hipErrorInvalidValue;
    return launch_for(a.NX, [&](auto nx, size_t lds) {
        constexpr int NX = decltype(nx)::value;
        if constexpr (NX > mhe::RL) hipLaunchKernelGGL(k_kf_dare_psd_wide<NX>, dim3(a.nwaves), dim3(WAVE), lds, st, a);
        else hipLaunchKernelGGL(k_kf_dare_psd<NX>, dim3(a.nwaves), dim3(WAVE), lds, st, a);
    });
}

}  // namespace kf
}  // namespace mpcqp
