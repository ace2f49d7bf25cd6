// TEST INFRASTRUCTURE ONLY: the discretisation and augmentation of continuous-time models (csrc/c2d_bodies.h) on the CPU,
// over the 64-lane wave of emu_wave.h.  Defines the launcher that csrc/c2d_launch.h declares weak.  Linked only into
// libmpcqp_emu_c2d.so (tests/emu/c2d.mk); the other emulator libraries have no such launcher and answer
// MPCQP_ERR_UNSUPPORTED to mpcqp_c2d and mpcqp_set_model_continuous.
#include "emu_wave.h"
#include "c2d_bodies.h"
#include "c2d_launch.h"

namespace mpcqp {
namespace c2d {

template <int NX>
static void run(const C2dArgs& a) {
    run_waves(a.B, c2d_lds_bytes(NX) / sizeof(double), [&](EmuWave& w, int b, double* sm) { c2d_body<NX>(w, a, b, sm); });
}

hipError_t launch_c2d(const C2dArgs& a, hipStream_t) {
    if (!c2d_args_ok(a)) return hipErrorInvalidValue;
    switch (c2d_columns_for(c2d_need(a))) {
        case 4: run<4>(a); break;
        case 8: run<8>(a); break;
        case 16: run<16>(a); break;
        default: run<32>(a);
    }
    return hipSuccess;
}

}  // namespace c2d
}  // namespace mpcqp
