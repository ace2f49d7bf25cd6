// TEST INFRASTRUCTURE ONLY: the steady-state Riccati solve of the SteadyKalmanFilter (csrc/kf_dare_bodies.h) on the CPU.
// Defines the launchers that csrc/kf_dare_launch.h declares weak, over the waves of emu_rowwave.h, like emu_kf_cov.cpp: four
// estimators per wavefront on 16-lane rows (max(nx̂, nym) <= 16) or one on the 64 lanes with the staged products (plain-loop
// side of Ops::mm_staged).  The doubling loop ends on a wave-wide vote: lanes that leave it at different iterations abort in
// the wave's divergence check.  Linked only into libmpcqp_emu_est.so (tests/emu/Makefile); the stock emulator library has
// no such launcher and answers MPCQP_ERR_UNSUPPORTED to mpcqp_kf_set_steady.
#include "emu_rowwave.h"
#include "kf_dare_bodies.h"
#include "kf_dare_launch.h"

namespace mpcqp {
namespace kf {

hipError_t launch_kf_dare(const DareArgs& a, hipStream_t) {
    if (!kf_dare_args_ok(a)) return hipErrorInvalidValue;
    return mhe::dispatch_nx<mhe::NX_NARROW | mhe::NX_WIDE>(a.NX, [&]<int NX>(mhe::Cols<NX>) {
        using W = mhe::EmuRowWaveFor<NX>;
        mhe::run_row_waves<W>(a.nwaves, 0, [&](W& w, int wv, double*) { kf_dare_body<W, NX>(w, a, wv); });
    });
}
// the grid of the covariance recursion (emu_kf_cov.cpp), as on the device
int kf_dare_waves_for(int device, int B, int NX) { return kf_cov_waves_for(device, B, NX); }

}  // namespace kf
}  // namespace mpcqp
