// ms_kernels.hip -- gfx950 kernels of the MultipleShooting LinMPC step (ms_bodies.h): one controller per 64-lane
// wavefront, one wavefront per workgroup.  Two placements of the horizon-long data (iterate, Riccati factor, rows):
//   k_ms_step    everything in LDS (small problems: up to MPCQP_MS_LDS_SHARE bytes per wavefront), grid = B;
//   k_ms_step_g  the model and the work matrices of a stage in LDS, the horizon-long data in a per-wavefront scratch in
//                HBM (L2-resident for the stage in flight); persistent grid of `nslots` wavefronts looping over the batch,
//                so the scratch is nslots x big doubles whatever B -- any horizon, eight wavefronts per CU.
#include <map>
#include <mutex>
#include <utility>
#include <hip/hip_runtime.h>

#include "mpcqp_bodies.h"
#include "mpcqp_devwave.h"
#include "ms_bodies.h"
#include "ms_launch.h"

namespace mpcqp {

// (custom linear constraints: the _w kernels, instantiated with the rows; stage-separable N_Hc / L_Hp blocks, MPCQP_FLAG_KEEP_QP
//  and MPCQP_FLAG_WARM_DUAL: the _o kernels (ms_has_options).  A handle without them runs the kernels it ran before.)
#define MPCQP_MS_KERNEL_LDS(name, HAS_W, HAS_OPT)                                                                              \
    __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 8))) void name(Dims d, Model m, StepIO io, MsIO ms) { \
        DevWave w{(int)threadIdx.x};                                                                                           \
        ms_step_body_t<false, HAS_W, HAS_OPT>(w, d, m, io, ms, (int)blockIdx.x, mpcqp_smem, (double*)nullptr);                \
    }
MPCQP_MS_KERNEL_LDS(k_ms_step, false, false)
MPCQP_MS_KERNEL_LDS(k_ms_step_w, true, false)
MPCQP_MS_KERNEL_LDS(k_ms_step_o, false, true)
MPCQP_MS_KERNEL_LDS(k_ms_step_wo, true, true)

#ifndef MPCQP_MS_WAVES
#define MPCQP_MS_WAVES 2
#endif
// controllers are handed out one at a time (ms.next: a counter in HBM, zeroed before the launch): a solve that runs to
// its iteration limit (80 iterations against a mean of 13) then delays its own wavefront, not a fixed share of the
// batch -- with the static assignment b = blockIdx + k gridDim one such controller set the time of the whole launch
// (measured: 131 ms for 2048 C3 controllers of which one is at the limit, 25 ms of work per wavefront otherwise)
// (two wavefronts per SIMD: without the attribute the compiler takes 372 registers and leaves one)
#define MPCQP_MS_KERNEL_HBM(name, HAS_W, HAS_OPT)                                                                                \
    __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(MPCQP_MS_WAVES, 8))) void name(Dims d, Model m, StepIO io, \
                                                                                                   MsIO ms, size_t big) {        \
        DevWave w{(int)threadIdx.x};                                                                                             \
        double* scratch = ms.scratch + (size_t)blockIdx.x * big;                                                                 \
        for (;;) {                                                                                                               \
            int b = 0;                                                                                                           \
            if (threadIdx.x == 0) b = atomicAdd(ms.next, 1);                                                                     \
            b = __builtin_amdgcn_readfirstlane(b);                                                                               \
            if (b >= d.B) break;                                                                                                 \
            ms_step_body_t<true, HAS_W, HAS_OPT>(w, d, m, io, ms, b, mpcqp_smem, scratch);                                      \
            w.sync();                                                                                                            \
        }                                                                                                                        \
    }
MPCQP_MS_KERNEL_HBM(k_ms_step_g, false, false)
MPCQP_MS_KERNEL_HBM(k_ms_step_gw, true, false)
MPCQP_MS_KERNEL_HBM(k_ms_step_go, false, true)
MPCQP_MS_KERNEL_HBM(k_ms_step_gwo, true, true)

// the kernel of a handle: [HBM placement][custom rows][options]
static const void* ms_kernel(bool hbm, bool hw, bool opt) {
    static const void* const k[2][2][2] = {{{(const void*)k_ms_step, (const void*)k_ms_step_o}, {(const void*)k_ms_step_w, (const void*)k_ms_step_wo}},
                                           {{(const void*)k_ms_step_g, (const void*)k_ms_step_go}, {(const void*)k_ms_step_gw, (const void*)k_ms_step_gwo}}};
    return k[hbm][hw][opt];
}

size_t ms_lds_bytes(const Dims& d, const Model& m) { return (size_t)make_ms_carve(d, m).total * sizeof(double); }

// bytes of HBM scratch the step needs (0: everything lives in LDS) and the number of resident wavefronts
size_t ms_scratch_bytes(const Dims& d, const Model& m, int* nslots) {
    const MsCarve c = make_ms_carve(d, m);
    if (c.big_in_lds) { if (nslots) *nslots = 0; return 0; }
    const size_t lds = (size_t)c.small * sizeof(double);
    // resident wavefronts per CU: what the runtime says for this kernel and this much LDS (registers, LDS allocation
    // granularity).  A persistent grid larger than that runs its surplus workgroups as a SECOND round (measured: 2048
    // launched where 1792 fit cost 2x).  The answer depends on (device, LDS bytes) only: asked once, then remembered,
    // so that a step does no runtime queries.
    int dev = 0, cus = 256, per_cu = 0;
    (void)hipGetDevice(&dev);
    const void* kern = ms_kernel(true, d.nw > 0, ms_has_options(d, m));
    {
        static std::mutex mu;
        static std::map<std::pair<std::pair<int, size_t>, const void*>, std::pair<int, int>> seen;
        std::lock_guard<std::mutex> lock(mu);
        auto it = seen.find({{dev, lds}, kern});
        if (it == seen.end()) {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, dev) == hipSuccess) cus = prop.multiProcessorCount;
            if (ensure_lds(kern, lds) != hipSuccess ||
                hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, WAVE, lds) != hipSuccess || per_cu < 1) {
                per_cu = (int)((160 * 1024) / (lds ? lds : 1));
                per_cu = per_cu > 8 ? 8 : per_cu < 1 ? 1 : per_cu;
            }
            it = seen.emplace(std::make_pair(std::make_pair(dev, lds), kern), std::make_pair(cus, per_cu)).first;
        }
        cus = it->second.first; per_cu = it->second.second;
    }
    int n = cus * per_cu;
    if (n > d.B) n = d.B;
    if (nslots) *nslots = n;
    return (size_t)n * c.big * sizeof(double);
}

hipError_t launch_ms_step(const Dims& d, const Model& m, const StepIO& io, const MsIO& ms, hipStream_t st) {
    const MsCarve c = make_ms_carve(d, m);
    const size_t lds = (size_t)c.total * sizeof(double);
    const void* kern = ms_kernel(!c.big_in_lds, d.nw > 0, ms_has_options(d, m));
    hipError_t e = ensure_lds(kern, lds);
    if (e != hipSuccess) return e;
    if (c.big_in_lds) {
        void* args[] = {(void*)&d, (void*)&m, (void*)&io, (void*)&ms};
        e = hipLaunchKernel(kern, dim3(d.B), dim3(WAVE), args, lds, st);
    } else {
        if (!ms.scratch || ms.nslots < 1 || !ms.next) return hipErrorInvalidValue;
        e = hipMemsetAsync(ms.next, 0, sizeof(int), st);
        if (e != hipSuccess) return e;
        size_t big = (size_t)c.big;
        void* args[] = {(void*)&d, (void*)&m, (void*)&io, (void*)&ms, (void*)&big};
        e = hipLaunchKernel(kern, dim3(ms.nslots), dim3(WAVE), args, lds, st);
    }
    if (e != hipSuccess) return e;
    return hipGetLastError();
}

}  // namespace mpcqp
