// im_kernels.hip -- gfx950 kernels of the InternalModel estimator (bodies: im_bodies.h).  One wavefront per workgroup, four
// members per wavefront (one per 16-lane row) or one (im_launch.h: group_lanes), 20 KB of LDS: two N x N matrices per member
// and the vectors the lanes of a member hand each other.
#include <hip/hip_runtime.h>

#include "im_bodies.h"
#include "im_launch.h"
#include "mpcqp_devwave.h"

namespace mpcqp {
namespace im {

__global__ __launch_bounds__(64) void k_im_setup(ImArgs a) {
    __shared__ double sm[IM_LDS_DOUBLES];
    DevWave w{(int)threadIdx.x};
    im_setup_body(w, a, (int)blockIdx.x, sm);
}

__global__ __launch_bounds__(64) void k_im_correct(ImArgs a) {
    __shared__ double sm[IM_LDS_DOUBLES];
    DevWave w{(int)threadIdx.x};
    im_correct_body(w, a, (int)blockIdx.x, sm);
}

__global__ __launch_bounds__(64) void k_im_update(ImArgs a) {
    __shared__ double sm[IM_VEC * WAVE];
    DevWave w{(int)threadIdx.x};
    im_update_body(w, a, (int)blockIdx.x, sm);      // (the update uses the vector slots only)
}

__global__ __launch_bounds__(64) void k_im_init(ImArgs a) {
    __shared__ double sm[IM_LDS_DOUBLES];
    DevWave w{(int)threadIdx.x};
    im_init_body(w, a, (int)blockIdx.x, sm);
}

__global__ __launch_bounds__(256) void k_im_beff(ImArgs a, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) im_beff_body(a, i);
}

hipError_t launch_im(const ImArgs& a, int kind, hipStream_t st) {
    if (!args_ok(a, kind)) return hipErrorInvalidValue;
    const long nw = waves(a);
    if (nw > 0x7fffffffL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nw), block(WAVE);
    switch (kind) {
        case IM_SETUP: hipLaunchKernelGGL(k_im_setup, grid, block, 0, st, a); break;
        case IM_CORRECT: hipLaunchKernelGGL(k_im_correct, grid, block, 0, st, a); break;
        case IM_UPDATE: hipLaunchKernelGGL(k_im_update, grid, block, 0, st, a); break;
        case IM_INIT: hipLaunchKernelGGL(k_im_init, grid, block, 0, st, a); break;
        case IM_BEFF: {
            const size_t n = (size_t)a.B * a.Hp * a.ny;
            if ((n + 255) / 256 > 0x7fffffffUL) return hipErrorInvalidValue;
            hipLaunchKernelGGL(k_im_beff, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, n);
            break;
        }
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace im
}  // namespace mpcqp
