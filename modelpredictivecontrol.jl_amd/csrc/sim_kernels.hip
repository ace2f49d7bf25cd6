// sim_kernels.hip -- gfx950 kernel of the closed-loop simulation's plant (body: sim_bodies.h).  One wavefront per workgroup,
// 64 / G controllers per wavefront (sim_launch.h), 2 KB of LDS for the vectors the lanes of a group hand each other.
#include <hip/hip_runtime.h>

#include "mhe_devwave.h"
#include "mpcqp_devwave.h"
#include "sim_bodies.h"
#include "sim_launch.h"

namespace mpcqp {
namespace sim {

__global__ __launch_bounds__(64) void k_sim_plant(PlantArgs a) {
    __shared__ double sm[PLANT_LDS_DOUBLES];
    DevWave w{(int)threadIdx.x};
    sim_plant_body(w, a, (int)blockIdx.x, sm);
}

hipError_t launch_sim_plant(const PlantArgs& a, hipStream_t st) {
    if (!plant_args_ok(a)) return hipErrorInvalidValue;
    const long waves = plant_waves(a);
    if (waves > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sim_plant, dim3((unsigned)waves), dim3(WAVE), 0, st, a);
    return hipGetLastError();
}

extern __shared__ double sim_smem[];

// (356 VGPRs: one wavefront per SIMD.  A budget of two per SIMD -- amdgpu_waves_per_eu(2) -- spills 101 of them to scratch)
__global__ __launch_bounds__(64) void k_sim_explicit(FusedArgs a) {
    mhe::MheDevWave w{(int)threadIdx.x};
    sim_explicit_body(w, a, (int)blockIdx.x, sim_smem);
}

hipError_t launch_sim_explicit(const FusedArgs& a, hipStream_t st) {
    const PlantArgs& p = a.p;
    const size_t lds = fused_lds_doubles(p, a.ncol) * sizeof(double);
    if (p.B < 1 || p.N < 1 || !fused_dims_ok(p) || p.nym < 1 || lds > 160 * 1024 || !a.law || !a.Khat || !a.Ahat || !a.Bhu ||
        !a.fstatus || !p.A || !p.Bu || !p.C || !p.Chat || !p.x || !p.xhat || !p.lastu0 || !p.ry || !p.i_ym || (p.nd > 0 && !p.d))
        return hipErrorInvalidValue;
    if (hipError_t e = ensure_lds((const void*)k_sim_explicit, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sim_explicit, dim3((unsigned)fused_waves(p)), dim3(WAVE), lds, st, a);
    return hipGetLastError();
}

}  // namespace sim
}  // namespace mpcqp
