// TEST INFRASTRUCTURE ONLY: the covariance / gain recursion of the time-varying KalmanFilter (csrc/kf_cov_bodies.h) on the
// CPU.  Defines the launchers that csrc/kf_cov_launch.h declares weak, over the waves of emu_rowwave.h: four estimators per
// wavefront on 16-lane rows (max(nx̂, nym) <= 16) or one on the 64 lanes with the staged products (plain-loop side of
// Ops::mm_staged).  Linked only into libmpcqp_emu_est.so (tests/emu/Makefile); the stock emulator library has no such
// launcher and answers MPCQP_ERR_UNSUPPORTED to mpcqp_kf_set_covariances.
#include "emu_rowwave.h"
#include "kf_cov_bodies.h"
#include "kf_cov_launch.h"

namespace mpcqp {
namespace kf {

hipError_t launch_kf_cov(const CovArgs& a, int mode, hipStream_t) {
    if (!kf_cov_args_ok(a)) return hipErrorInvalidValue;
    return mhe::dispatch_nx<mhe::NX_NARROW | mhe::NX_WIDE>(a.NX, [&]<int NX>(mhe::Cols<NX>) {
        using W = mhe::EmuRowWaveFor<NX>;
        mhe::run_row_waves<W>(a.nwaves, 0, [&](W& w, int wv, double*) { kf_cov_body<W, NX>(w, a, mode, wv); });
    });
}
// two "persistent" wavefronts: the grid-stride loop is exercised
int kf_cov_waves_for(int, int B, int NX) {
    const int groups = NX > mhe::RL ? B : (B + mhe::GPW - 1) / mhe::GPW;
    return groups < 2 ? groups : 2;
}

}  // namespace kf
}  // namespace mpcqp
