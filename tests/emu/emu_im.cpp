// TEST INFRASTRUCTURE ONLY: the InternalModel estimator (csrc/im_bodies.h) on the CPU, over the 64-lane wave of emu_wave.h
// (the bodies use `lane` and `sync` only).  Defines the launcher that csrc/im_launch.h declares weak.  Linked only into
// libmpcqp_emu_im.so (tests/emu/im.mk); the other emulator libraries have no such launcher and answer
// MPCQP_ERR_UNSUPPORTED to mpcqp_im_set.
#include "emu_wave.h"
#include "im_bodies.h"
#include "im_launch.h"

namespace mpcqp {
namespace im {

hipError_t launch_im(const ImArgs& a, int kind, hipStream_t) {
    if (!args_ok(a, kind)) return hipErrorInvalidValue;
    const int nw = (int)waves(a);
    switch (kind) {
        case IM_SETUP: run_waves(nw, IM_LDS_DOUBLES, [&](EmuWave& w, int wv, double* sm) { im_setup_body(w, a, wv, sm); }); break;
        case IM_CORRECT: run_waves(nw, IM_LDS_DOUBLES, [&](EmuWave& w, int wv, double* sm) { im_correct_body(w, a, wv, sm); }); break;
        case IM_UPDATE: run_waves(nw, IM_VEC * WAVE, [&](EmuWave& w, int wv, double* sm) { im_update_body(w, a, wv, sm); }); break;
        case IM_INIT: run_waves(nw, IM_LDS_DOUBLES, [&](EmuWave& w, int wv, double* sm) { im_init_body(w, a, wv, sm); }); break;
        case IM_BEFF:
            for (size_t i = 0; i < (size_t)a.B * a.Hp * a.ny; ++i) im_beff_body(a, i);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipSuccess;
}

}  // namespace im
}  // namespace mpcqp
