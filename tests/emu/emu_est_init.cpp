// TEST INFRASTRUCTURE ONLY: the estimator half of initstate! (csrc/est_init_bodies.h) on the CPU, over the 64-lane wave of
// emu_wave.h.  Defines the launcher that csrc/est_init_launch.h declares weak.  Linked only into libmpcqp_emu_mheloop.so
// (tests/emu/mheloop.mk); the other emulator libraries have no such launcher and answer MPCQP_ERR_UNSUPPORTED to
// mpcqp_est_initstate.
#include "emu_wave.h"
#include "est_init_bodies.h"
#include "est_init_launch.h"

namespace mpcqp {
namespace est {

template <int NX>
static void run(const InitArgs& a) {
    run_waves(a.B, 0, [&](EmuWave& w, int b, double*) { est_init_body<NX>(w, a, b); });
}

hipError_t launch_est_init(const InitArgs& a, hipStream_t) {
    if (!init_args_ok(a)) return hipErrorInvalidValue;
    switch (init_columns_for(a.nx)) {
        case 4: run<4>(a); break;
        case 8: run<8>(a); break;
        case 16: run<16>(a); break;
        default: run<32>(a);
    }
    return hipSuccess;
}

}  // namespace est
}  // namespace mpcqp
