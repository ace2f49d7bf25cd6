// est_kernels.hip -- gfx950 kernel of the estimator half of initstate! (body: est_init_bodies.h).  One wavefront per workgroup
// and per member, no LDS: the matrix lives in registers, one row per lane.
#include <hip/hip_runtime.h>

#include "est_init_bodies.h"
#include "est_init_launch.h"
#include "mpcqp_devwave.h"

namespace mpcqp {
namespace est {

template <int NX>
__global__ __launch_bounds__(64) void k_est_init(InitArgs a) {
    DevWave w{(int)threadIdx.x};
    est_init_body<NX>(w, a, (int)blockIdx.x);
}

hipError_t launch_est_init(const InitArgs& a, hipStream_t st) {
    if (!init_args_ok(a)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.B), block(WAVE);
    switch (init_columns_for(a.nx)) {
        case 4: hipLaunchKernelGGL(k_est_init<4>, grid, block, 0, st, a); break;
        case 8: hipLaunchKernelGGL(k_est_init<8>, grid, block, 0, st, a); break;
        case 16: hipLaunchKernelGGL(k_est_init<16>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(k_est_init<32>, grid, block, 0, st, a);
    }
    return hipGetLastError();
}

}  // namespace est
}  // namespace mpcqp
