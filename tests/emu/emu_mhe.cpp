// TEST INFRASTRUCTURE ONLY: the 16-lane MovingHorizonEstimator kernels (csrc/mhe_bodies.h, entry points of
// csrc/mhe_launch.h) and the small-problem LinMPC step (csrc/mpcqp_small_bodies.h) on the CPU, over the 16-lane wave and the
// runner of emu_rowwave.h.  Part of both emulator libraries (tests/emu/Makefile).
#include <cstdlib>

#include "emu_rowwave.h"
#include "mhe_launch.h"
#include "mpcqp_launch.h"
#include "mpcqp_small_bodies.h"

namespace mpcqp {
namespace mhe {

using W16 = EmuRow16;

hipError_t launch_setup(const Dims& d, const Raw& in, double* cst, hipStream_t) {
    return dispatch_nx<NX_NARROW>(d.NX, [&]<int NX>(Cols<NX>) {
        run_row_waves<W16>(d.nwaves, 0, [&](W16& w, int wv, double*) { setup_body<W16, NX>(w, d, in, cst, wv); });
    });
}
hipError_t launch_cov(const Dims& d, const Args& a, int mode, const double* P0, double* Pout, hipStream_t) {
    return dispatch_nx<NX_NARROW>(d.NX, [&]<int NX>(Cols<NX>) {
        run_row_waves<W16>(d.nwaves, 0, [&](W16& w, int wv, double*) { cov_body<W16, NX>(w, d, a, mode, P0, Pout, wv); });
    });
}
hipError_t launch_step(const Dims& d, const Args& a, hipStream_t) {
    return dispatch_nx<NX_NARROW>(d.NX, [&]<int NX>(Cols<NX>) {
        run_row_waves<W16>(d.nwaves, step_lds_doubles(d.NX), [&](W16& w, int wv, double* sm) { step_body<W16, NX, 15u>(w, d, a, wv, sm); });
    });
}
}  // namespace mhe

// the small-problem step kernel (csrc/mpcqp_small_bodies.h) has the same wave interface: KYS row slots per lane in the
// variant with dense rows (0: none), POL: with the active-set polish
template <int KYS, bool POL = false>
static hipError_t run_small(const Dims& d, const Model& m, const StepIO& io) {
    using namespace mhe;
    const int grid = (d.B + SMALL_GPW - 1) / SMALL_GPW, NXv = 4 * ((d.nZ + 3) / 4);
    return dispatch_nx<NX_NARROW>(NXv, [&]<int NX>(Cols<NX>) {
        run_row_waves<W16>(grid, small_lds_doubles(d, KYS != 0), [&](W16& w, int wv, double* sm) { step_small_body<W16, NX, KYS, POL>(w, d, m, io, wv, sm); });
    });
}
hipError_t launch_step_small(const Dims& d, const Model& m, const StepIO& io, hipStream_t) {
    if (small_has_y(d)) {
        switch (small_row_slots(d)) {
            case 2: return run_small<2>(d, m, io);
            case 3: return run_small<3>(d, m, io);
            default: return run_small<4>(d, m, io);
        }
    }
    // the product runs the variant with the active-set polish on grids beyond one wavefront per SIMD; here: unless
    // MPCQP_EMU_SMALL_POLISH=0 (the tests run both)
    const char* e = getenv("MPCQP_EMU_SMALL_POLISH");
    return e && e[0] == '0' ? run_small<0>(d, m, io) : run_small<0, true>(d, m, io);
}

namespace mhe {

int waves_for(int, int B, int) {
    const int groups = (B + GPW - 1) / GPW;
    return groups < 2 ? groups : 2;       // two "persistent" wavefronts: the grid-stride loop is exercised
}

}  // namespace mhe
}  // namespace mpcqp
