// TEST INFRASTRUCTURE ONLY: the second pass of the steady-state Riccati solve (csrc/kf_dare_bodies.h: its square-root form
// for a semidefinite Q̂) on the CPU.  Defines the launcher that csrc/kf_dare_launch.h declares weak, over the waves of
// emu_rowwave.h, like emu_kf_dare.cpp: the same wavefronts (a.nwaves comes from kf_dare_waves_for of that file), four
// estimators per wavefront on 16-lane rows or one on the 64 lanes with the staged products.  Both of its votes -- "does this
// wavefront hold a candidate" and the loop exit -- are wave-wide: lanes that disagree abort in the wave's divergence check.
// Linked only into libmpcqp_emu_est_psd.so (tests/emu/psd.mk); libmpcqp_emu_est.so has no such launcher and keeps the
// result of the first pass.
#include "emu_rowwave.h"
#include "kf_dare_launch.h"
#include "kf_dare_psd_bodies.h"

namespace mpcqp {
namespace kf {

hipError_t launch_kf_dare_psd(const DareArgs& a, hipStream_t) {
    if (!kf_dare_args_ok(a) || !a.path) return hipErrorInvalidValue;
    return mhe::dispatch_nx<mhe::NX_NARROW | mhe::NX_WIDE>(a.NX, [&]<int NX>(mhe::Cols<NX>) {
        using W = mhe::EmuRowWaveFor<NX>;
        mhe::run_row_waves<W>(a.nwaves, 0, [&](W& w, int wv, double*) { kf_dare_psd_body<W, NX>(w, a, wv); });
    });
}

}  // namespace kf
}  // namespace mpcqp
