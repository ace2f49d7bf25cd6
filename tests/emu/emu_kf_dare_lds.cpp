// TEST INFRASTRUCTURE ONLY: the LDS-resident steady-state Riccati solve (csrc/kf_dare_lds_bodies.h, 32 < max(nx̂, nym) <= 64)
// on the CPU.  Defines the launchers that csrc/kf_dare_lds_launch.h declares weak over ONE emulated wavefront per workgroup
// (T = 1: the fibers of emu_rowwave.h are the 64 lanes, their barrier is the workgroup barrier), with the "LDS" as a host
// buffer and the plain-loop side of the tile product.  Whatever team is asked for, T = 1 runs (kf_dare_lds_team_for), so
// mpcqp_kf_lanes_per_estimator answers 64 here.  The workgroups run one after the other.  Linked only into
// libmpcqp_emu_est_lds.so (tests/emu/dare_lds.mk); libmpcqp_emu_est.so has no such launcher and keeps refusing beyond 32.
#include "emu_rowwave.h"
#include "kf_dare_lds_bodies.h"
#include "kf_dare_lds_launch.h"

namespace mpcqp {
namespace kf {

template <int N>
static void run_order(const DareArgs& a) {
    using W = mhe::EmuRow16;              // (lane and sync() are all the body uses of it)
    mhe::run_row_waves<W>(a.nwaves, dare_lds_doubles(N, 1), [&](W& w, int wg, double* lds) { kf_dare_lds_body<W, N, 1>(w, a, wg, 0, lds); });
}

hipError_t launch_kf_dare_lds(const DareArgs& a, int team, hipStream_t) {
    if (!kf_dare_lds_args_ok(a, team) || team != 1) return hipErrorInvalidValue;
    if (a.NX == 48) run_order<48>(a);
    else run_order<64>(a);
    return hipSuccess;
}
int kf_dare_lds_team_for(int) { return 1; }
// as on the device: a workgroup per estimator up to the number of CUs (256 where there is no device to ask)
int kf_dare_lds_waves_for(int, int B, int) { return B < 256 ? B : 256; }

}  // namespace kf
}  // namespace mpcqp
