// kf_dare_lds_kernels.hip -- gfx950 kernels of the steady-state Riccati solve of the SteadyKalmanFilter for
// 32 < max(nx̂, nym) <= 64 (body: kf_dare_lds_bodies.h): k_kf_dare_lds<N, T>, N = 48, 64 the padded order, T = 1, 2, 4 the
// wavefronts of the workgroup that holds one estimator.  Persistent grid, one workgroup per CU (the four operand buffers
// take 140.5 KB of the CU's 160 KB at N = 64, 82.9 KB at N = 48), grid-stride loop over the batch.
#include <hip/hip_runtime.h>

#include "kf_dare_lds_bodies.h"
#include "kf_dare_lds_launch.h"
#include "mpcqp_devwave.h"

namespace mpcqp {
namespace kf {

// the wave of these kernels: a lane index within the wavefront and the workgroup barrier
struct DareLdsWave {
    int lane;
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

// (registers: two accumulator sets -- the running product and the operand kept out of LDS -- of 16 / T tiles of four
// doubles each at N = 64: 256 VGPRs at T = 1, 64 at T = 4; one wavefront per SIMD either way, as the LDS decides.  With
// the addresses of the unrolled tile loops T = 1 at N = 64 spills (lib/isa_resources.txt): it is the yardstick of the
// team-size tests, not the product form, which has no spill)
template <int N, int T>
__global__ __launch_bounds__(WAVE * T) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_kf_dare_lds(DareArgs a) {
    DareLdsWave w{(int)threadIdx.x & (WAVE - 1)};
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    kf_dare_lds_body<DareLdsWave, N, T>(w, a, (int)blockIdx.x, wv, mpcqp_smem);
}

template <int N, int T>
static hipError_t launch_nt(const DareArgs& a, hipStream_t st) {
    const size_t lds = dare_lds_doubles(N, T) * sizeof(double);
    if (hipError_t e = ensure_lds((const void*)k_kf_dare_lds<N, T>, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL((k_kf_dare_lds<N, T>), dim3(a.nwaves), dim3(WAVE * T), lds, st, a);
    return hipGetLastError();
}
template <int N>
static hipError_t launch_n(const DareArgs& a, int team, hipStream_t st) {
    return team == 1 ? launch_nt<N, 1>(a, st) : team == 2 ? launch_nt<N, 2>(a, st) : launch_nt<N, 4>(a, st);
}

hipError_t launch_kf_dare_lds(const DareArgs& a, int team, hipStream_t st) {
    if (!kf_dare_lds_args_ok(a, team)) return hipErrorInvalidValue;
    return a.NX == 48 ? launch_n<48>(a, team, st) : launch_n<64>(a, team, st);
}

int kf_dare_lds_team_for(int wanted) { return wanted == 1 || wanted == 2 || wanted == 4 ? wanted : DARE_LDS_TEAM; }

// the grid: one workgroup per CU is what the LDS admits at either order (two of N = 48 would need 165.8 KB)
int kf_dare_lds_waves_for(int device, int B, int N) {
    (void)N;
    int cus = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    return B < cus ? B : cus;
}

}  // namespace kf
}  // namespace mpcqp
