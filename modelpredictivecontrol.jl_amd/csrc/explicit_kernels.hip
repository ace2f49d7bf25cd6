// explicit_kernels.hip -- gfx950 kernels of the batched ExplicitMPC (bodies: explicit_bodies.h).  One wavefront per
// workgroup everywhere:
//   k_explicit_factor   one controller per workgroup, once per model: 2 n^2 doubles of LDS (64 KB at n = 64)
//   k_explicit_step     one controller per workgroup, every period: F, M (F - R^y), the step-response table and H~^-1 in LDS
//                       (up to the 160 KB of a CU, like the condensed step kernels: explicit_launch.h, step_lds_doubles)
//   k_explicit_law      persistent grid, 64 rows of the batch's Z~ (or u0) per wavefront and trip: several controllers per
//                       wavefront, 16-byte loads of consecutive addresses
//   k_explicit_law_unit / _pack   element-wise helpers of the law build (superposition on device buffers)
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "explicit_bodies.h"
#include "explicit_launch.h"
#include "mpcqp_devwave.h"

namespace mpcqp {
namespace ex {

extern __shared__ double ex_smem[];

__global__ __launch_bounds__(64) void k_explicit_factor(FactorArgs a) {
    DevWave w{(int)threadIdx.x};
    explicit_factor_body(w, a, (int)blockIdx.x, ex_smem);
}

__global__ __launch_bounds__(64) void k_explicit_step(StepArgs a) {
    DevWave w{(int)threadIdx.x};
    explicit_step_body(w, a, (int)blockIdx.x, ex_smem);
}

__global__ __launch_bounds__(64) void k_explicit_law(LawArgs a) {
    DevWave w{(int)threadIdx.x};
    explicit_law_body(w, a, (int)blockIdx.x);
}

__global__ __launch_bounds__(64) void k_explicit_law_unit(LawBuildArgs a, int nt) {
    const size_t id = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (id < (size_t)a.B * nt) explicit_law_unit_at(a, id / nt, (int)(id % nt));
}

__global__ __launch_bounds__(64) void k_explicit_law_pack(LawBuildArgs a) {
    const size_t R = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (R < (size_t)a.B * a.n) explicit_law_pack_at(a, R);
}

hipError_t launch_explicit_factor(const FactorArgs& a, hipStream_t st) {
    const size_t lds = factor_lds_doubles(a.n) * sizeof(double);
    if (a.B < 1 || a.n < 1 || a.n > EX_NMAX || lds > EX_LDS_MAX) return hipErrorInvalidValue;
    if (hipError_t e = ensure_lds((const void*)k_explicit_factor, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_explicit_factor, dim3(a.B), dim3(WAVE), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_explicit_step(const StepArgs& a, hipStream_t st) {
    const size_t lds = step_lds_doubles(a.d) * sizeof(double);
    if (a.d.B < 1 || a.d.nDU < 1 || a.d.nDU > EX_NMAX || lds > EX_LDS_MAX || !a.Hinv) return hipErrorInvalidValue;
    if (hipError_t e = ensure_lds((const void*)k_explicit_step, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_explicit_step, dim3(a.d.B), dim3(WAVE), lds, st, a);
    return hipGetLastError();
}

hipError_t launch_explicit_law(const LawArgs& a, hipStream_t st) {
    if (a.B < 1 || a.rows < 1 || a.nwaves < 1 || a.kp < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_explicit_law, dim3(a.nwaves), dim3(WAVE), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_explicit_law_unit(const LawBuildArgs& a, hipStream_t st) {
    const int nt = a.nd > 0 ? a.Hp : 1;
    const size_t total = (size_t)a.B * nt;
    hipLaunchKernelGGL(k_explicit_law_unit, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, st, a, nt);
    return hipGetLastError();
}

hipError_t launch_explicit_law_pack(const LawBuildArgs& a, hipStream_t st) {
    const size_t total = (size_t)a.B * a.n;
    hipLaunchKernelGGL(k_explicit_law_pack, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, st, a);
    return hipGetLastError();
}

// The grid of the law kernel: a handful of registers and no LDS, so sixteen wavefronts per CU; what is not resident at once is
// reached by the kernel's loop over groups.  The environment variable MPCQP_EXPLICIT_WAVES (include/mpcqp.h) caps the grid; it
// is read here, that is once per mpcqp_explicit_prepare, and the handle keeps the result.
int explicit_law_waves_for(int device, long groups) {
    int cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    long cap = (long)cus * 16;
    if (const char* e = getenv("MPCQP_EXPLICIT_WAVES")) {
        const long v = atol(e);
        if (v >= 1 && v < cap) cap = v;
    }
    return (int)(groups < cap ? (groups < 1 ? 1 : groups) : cap);
}

}  // namespace ex
}  // namespace mpcqp
