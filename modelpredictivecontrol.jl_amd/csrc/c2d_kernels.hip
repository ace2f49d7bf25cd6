// c2d_kernels.hip -- gfx950 kernel of the discretisation and augmentation of a batch of continuous-time models (body:
// c2d_bodies.h).  One wavefront per workgroup and per member; the dynamic LDS is c2d_lds_bytes(NX) (c2d_launch.h).
#include <hip/hip_runtime.h>

#include "c2d_bodies.h"
#include "c2d_launch.h"
#include "mpcqp_devwave.h"

namespace mpcqp {
namespace c2d {

template <int NX>
__global__ __launch_bounds__(64) void k_c2d(C2dArgs a) {
    DevWave w{(int)threadIdx.x};
    c2d_body<NX>(w, a, (int)blockIdx.x, mpcqp_smem);
}

hipError_t launch_c2d(const C2dArgs& a, hipStream_t st) {
    if (!c2d_args_ok(a)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.B), block(WAVE);
    const int NX = c2d_columns_for(c2d_need(a));
    const size_t lds = c2d_lds_bytes(NX);
    switch (NX) {
        case 4: hipLaunchKernelGGL(k_c2d<4>, grid, block, lds, st, a); break;
        case 8: hipLaunchKernelGGL(k_c2d<8>, grid, block, lds, st, a); break;
        case 16: hipLaunchKernelGGL(k_c2d<16>, grid, block, lds, st, a); break;
        default: hipLaunchKernelGGL(k_c2d<32>, grid, block, lds, st, a);
    }
    return hipGetLastError();
}

}  // namespace c2d
}  // namespace mpcqp
