// kf_dare_lds_launch.h -- host-side launch entry points of the steady-state Riccati solve of the SteadyKalmanFilter for
// 32 < max(nx̂, nym) <= 64 (kf_dare_lds_kernels.hip; body: kf_dare_lds_bodies.h): operands in LDS, one estimator per
// workgroup of `team` wavefronts.  WEAK declarations, as in kf_dare_launch.h: a library linked without the launcher
// (tests/emu/libmpcqp_emu_est.so; libmpcqp_emu_est_lds.so has the one of tests/emu/emu_kf_dare_lds.cpp) still links, and
// mpcqp_kf_set_steady keeps answering MPCQP_ERR_UNSUPPORTED beyond 32 (kf_dare_lds_available()).  The arguments, the
// constants and the statuses are those of kf_dare_launch.h; DareArgs::NX carries the padded order N, DareArgs::nwaves the
// WORKGROUPS of the persistent grid, and DareArgs::path is not written (the host zeroes it: there is no second pass).
#pragma once
#include "kf_dare_launch.h"

namespace mpcqp {
namespace kf {

constexpr int DARE_LDS_NMAX = 64;          // largest padded order
constexpr int DARE_LDS_TEAM = 4;           // wavefronts per estimator of the product form (1, 2: test hooks)
// padded order of max(nx̂, nym): a multiple of the 16 x 16 output tile of v_mfma_f64_16x16x4
inline int kf_dare_lds_order_for(int nmax) { return nmax <= 48 ? 48 : 64; }
// Leading dimension of an N x N operand in LDS.  N + 2: the first operand of a tile product is read as [i = lane & 15][k =
// lane >> 4], i.e. at 2 i + k (mod 32) in units of the 8-byte bank pair -- 32 different ones for the 32 lanes of a
// half-wave (N = 64; N = 48: 18 i + k, the same).  The second operand, [k][j = lane & 15], sits at j + 2 k: the two k of a
// half-wave overlap in 14 banks (two cycles instead of one); its transposed form is read like the first operand.
constexpr int dare_lds_ld(int N) { return N + 2; }
// LDS of one workgroup in doubles: four N x LD operands, the pivot row / column of the inverse (two of each: a step writes
// the next step's while its own are read), the N reciprocal pivots, three reduction slots per lane
constexpr size_t dare_lds_doubles(int N, int team) { return (size_t)4 * N * dare_lds_ld(N) + 5 * N + 3 * 64 * team; }

inline bool kf_dare_lds_args_ok(const DareArgs& a, int team) {
    return kf_dare_args_ok(a) && (a.NX == 48 || a.NX == 64) && (team == 1 || team == 2 || team == 4);
}

__attribute__((weak)) hipError_t launch_kf_dare_lds(const DareArgs& a, int team, hipStream_t st);
__attribute__((weak)) int kf_dare_lds_waves_for(int device, int B, int N);     // workgroups of the persistent grid
// the team this launcher runs when `wanted` is asked for (0 or anything it has not compiled: its default -- DARE_LDS_TEAM
// on the device, 1 on the CPU emulator, which has one emulated wavefront)
__attribute__((weak)) int kf_dare_lds_team_for(int wanted);
inline bool kf_dare_lds_available() { return launch_kf_dare_lds && kf_dare_lds_waves_for && kf_dare_lds_team_for; }

}  // namespace kf
}  // namespace mpcqp
