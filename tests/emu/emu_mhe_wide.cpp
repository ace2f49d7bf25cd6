// TEST INFRASTRUCTURE ONLY: the wide MovingHorizonEstimator kernels (16 < max(nx̂, nym) <= 32, one estimator per wavefront)
// on the CPU.  Defines the launchers that csrc/mhe_wide_launch.h declares weak, over the 64-lane wave of emu_rowwave.h: the
// bodies of csrc/mhe_bodies.h with GL = 64, GPW = 1 and the staged products (Ops::mm_staged, plain-loop side).  Linked only
// into libmpcqp_emu_est.so (tests/emu/Makefile); the stock emulator library has no wide launchers and refuses such handles.
#include "emu_rowwave.h"
#include "mhe_wide_launch.h"

namespace mpcqp {
namespace mhe {

hipError_t launch_wide_setup(const Dims& d, const Raw& in, double* cst, hipStream_t) {
    return dispatch_nx<NX_WIDE>(d.NX, [&]<int NX>(Cols<NX>) {
        run_row_waves<EmuWide>(d.nwaves, 0, [&](EmuWide& w, int wv, double*) { setup_body<EmuWide, NX>(w, d, in, cst, wv); });
    });
}
hipError_t launch_wide_cov(const Dims& d, const Args& a, int mode, const double* P0, double* Pout, hipStream_t) {
    return dispatch_nx<NX_WIDE>(d.NX, [&]<int NX>(Cols<NX>) {
        run_row_waves<EmuWide>(d.nwaves, 0, [&](EmuWide& w, int wv, double*) { cov_body<EmuWide, NX>(w, d, a, mode, P0, Pout, wv); });
    });
}
hipError_t launch_wide_step(const Dims& d, const Args& a, hipStream_t) {
    return dispatch_nx<NX_WIDE>(d.NX, [&]<int NX>(Cols<NX>) {
        run_row_waves<EmuWide>(d.nwaves, step_lds_doubles(d.NX), [&](EmuWide& w, int wv, double* sm) { step_body<EmuWide, NX, 15u>(w, d, a, wv, sm); });
    });
}
int wide_waves_for(int, int B, int) { return B < 2 ? B : 2; }      // two "persistent" wavefronts: the grid-stride loop is exercised

}  // namespace mhe
}  // namespace mpcqp
