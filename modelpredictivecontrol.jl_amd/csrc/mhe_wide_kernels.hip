// mhe_wide_kernels.hip -- gfx950 kernels of the batched linear MovingHorizonEstimator for 16 < max(nx̂, nym) <= 32
// (bodies: mhe_bodies.h, wave interface: mhe_wide_devwave.h).  One wavefront per workgroup, ONE estimator per wavefront,
// persistent grid.  Register columns NX = 24 or 32 (the dimension rounded up to a multiple of eight: two sizes of large
// kernels instead of four).
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "mhe_bodies.h"
#include "mhe_dispatch.h"
#include "mhe_wide_devwave.h"
#include "mhe_wide_launch.h"
#include "mpcqp_launch.h"

// 1: the NX^3 products run on the matrix cores, staged through LDS (Ops::mm_staged); 0: on wave-uniform broadcasts
// (v_readlane + v_fma_f64).  The A/B of DESIGN 4.3 is this switch; the slower form is not built into the library.
#ifndef MPCQP_MHE_WIDE_MFMA
#define MPCQP_MHE_WIDE_MFMA 1
#endif

namespace mpcqp {
namespace mhe {

#if MPCQP_MHE_WIDE_MFMA
using WideWave = MheWideMfmaWave;
__device__ __forceinline__ WideWave make_wave(double* stage) { WideWave w; w.lane = (int)threadIdx.x; w.stage = stage; return w; }
static constexpr size_t kStageDoubles = stage_doubles();
#else
using WideWave = MheWideDevWave;
__device__ __forceinline__ WideWave make_wave(double*) { WideWave w; w.lane = (int)threadIdx.x; return w; }
static constexpr size_t kStageDoubles = 0;
#endif

template <int NX>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8))) void k_mhe_wide_setup(Dims d, Raw in, double* cst) {
    WideWave w = make_wave(mpcqp_smem);
    setup_body<WideWave, NX>(w, d, in, cst, (int)blockIdx.x);
}
template <int NX>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8))) void k_mhe_wide_cov(Dims d, Args a, int mode, const double* P0, double* Pout) {
    WideWave w = make_wave(mpcqp_smem);
    cov_body<WideWave, NX>(w, d, a, mode, P0, Pout, (int)blockIdx.x);
}
// one wavefront per SIMD (512 registers): a row of the largest block is 64 of them
template <int NX, unsigned CM>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(1, 8))) void k_mhe_wide_step(Dims d, Args a) {
    WideWave w = make_wave(mpcqp_smem + step_lds_doubles(NX));
    step_body<WideWave, NX, CM>(w, d, a, (int)blockIdx.x, mpcqp_smem);
}

static size_t wide_step_lds_bytes(int NX) { return (step_lds_doubles(NX) + kStageDoubles) * sizeof(double); }

// k<NX> for the register columns of the handle (wide family: 24, 32) on its persistent grid
template <class F>
static hipError_t launch_for(const Dims& d, F launch) {
    const hipError_t e = dispatch_nx<NX_WIDE>(d.NX, launch);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_wide_setup(const Dims& d, const Raw& in, double* cst, hipStream_t st) {
    const size_t lds = kStageDoubles * sizeof(double);
    return launch_for(d, [&](auto nx) {
        hipLaunchKernelGGL(k_mhe_wide_setup<decltype(nx)::value>, dim3(d.nwaves), dim3(WAVE), lds, st, d, in, cst);
    });
}
hipError_t launch_wide_cov(const Dims& d, const Args& a, int mode, const double* P0, double* Pout, hipStream_t st) {
    const size_t lds = kStageDoubles * sizeof(double);
    return launch_for(d, [&](auto nx) {
        hipLaunchKernelGGL(k_mhe_wide_cov<decltype(nx)::value>, dim3(d.nwaves), dim3(WAVE), lds, st, d, a, mode, P0, Pout);
    });
}
template <unsigned CM>
static hipError_t launch_wide_step_as(const Dims& d, const Args& a, hipStream_t st) {
    hipError_t err = hipSuccess;
    const hipError_t e = dispatch_nx<NX_WIDE>(d.NX, [&](auto nx) {
        constexpr int NX = decltype(nx)::value;
        const size_t lds = wide_step_lds_bytes(NX);
        err = ensure_lds((const void*)k_mhe_wide_step<NX, CM>, lds);       // (above 64 KB with the staging buffer at NX = 32)
        if (err != hipSuccess) return;
        hipLaunchKernelGGL((k_mhe_wide_step<NX, CM>), dim3(d.nwaves), dim3(WAVE), lds, st, d, a);
        err = hipGetLastError();
    });
    return e != hipSuccess ? e : err;
}
hipError_t launch_wide_step(const Dims& d, const Args& a, hipStream_t st) {
    if ((d.cls & ~CLS_X) == 0) return launch_wide_step_as<1u>(d, a, st);
    if (d.cls & CLS_S) return launch_wide_step_as<15u>(d, a, st);      // soft constraints: all classes + the slack variable
    return launch_wide_step_as<7u>(d, a, st);
}

// The grid: one wavefront per estimator up to what a CU holds.  Registers allow one wavefront per SIMD (four per CU);
// LDS allows 160 KB / (3 NX x 512 B + staging) -- 3 at NX = 24, 2 at NX = 32 with the staging buffer (4 and 3 without).
int wide_waves_for(int device, int B, int NX) {
    int cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    const size_t lds_cu = 160 * 1024;
    int per_cu = (int)(lds_cu / wide_step_lds_bytes(NX));
    if (per_cu > 4) per_cu = 4;
    if (per_cu < 1) per_cu = 1;
    if (const char* e = getenv("MPCQP_MHE_WAVES_PER_CU")) per_cu = atoi(e) > 0 ? atoi(e) : per_cu;
    const int cap = cus * per_cu;
    return B < cap ? B : cap;
}

}  // namespace mhe
}  // namespace mpcqp
