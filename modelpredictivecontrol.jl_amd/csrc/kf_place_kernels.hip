// kf_place_kernels.hip -- gfx950 kernel of the pole placement of the Luenberger observer (body: kf_place_bodies.h).  One
// wavefront per workgroup and per member; the dynamic LDS is place_carve() of the shape (kf_place_launch.h).
#include <hip/hip_runtime.h>

#include "kf_place_bodies.h"
#include "kf_place_launch.h"
#include "mpcqp_devwave.h"

namespace mpcqp {
namespace kf {

template <int NX>
__global__ __launch_bounds__(64) void k_kf_place(PlaceArgs a) {
    DevWave w{(int)threadIdx.x};
    kf_place_body<NX>(w, a, (int)blockIdx.x, mpcqp_smem);
}

hipError_t launch_kf_place(const PlaceArgs& a, hipStream_t st) {
    if (!place_args_ok(a)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.B), block(WAVE);
    const size_t lds = place_lds_bytes(a);
    switch (place_columns_for(a.nx > a.nym ? a.nx : a.nym)) {
        case 4: hipLaunchKernelGGL(k_kf_place<4>, grid, block, lds, st, a); break;
        case 8: hipLaunchKernelGGL(k_kf_place<8>, grid, block, lds, st, a); break;
        case 16: hipLaunchKernelGGL(k_kf_place<16>, grid, block, lds, st, a); break;
        default: hipLaunchKernelGGL(k_kf_place<32>, grid, block, lds, st, a);
    }
    return hipGetLastError();
}

}  // namespace kf
}  // namespace mpcqp
