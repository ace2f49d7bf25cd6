// TEST INFRASTRUCTURE ONLY: the pole placement of the Luenberger observer (csrc/kf_place_bodies.h) on the CPU, over the
// 64-lane wave of emu_wave.h.  Defines the launcher that csrc/kf_place_launch.h declares weak.  Linked only into
// libmpcqp_emu_kf_place.so (tests/emu/kf_place.mk); the other emulator libraries have no such launcher and answer
// MPCQP_ERR_UNSUPPORTED to mpcqp_kf_set_poles.
#include "emu_wave.h"
#include "kf_place_bodies.h"
#include "kf_place_launch.h"

namespace mpcqp {
namespace kf {

template <int NX>
static void run(const PlaceArgs& a) {
    run_waves(a.B, place_lds_bytes(a) / sizeof(double), [&](EmuWave& w, int b, double* sm) { kf_place_body<NX>(w, a, b, sm); });
}

hipError_t launch_kf_place(const PlaceArgs& a, hipStream_t) {
    if (!place_args_ok(a)) return hipErrorInvalidValue;
    switch (place_columns_for(a.nx > a.nym ? a.nx : a.nym)) {
        case 4: run<4>(a); break;
        case 8: run<8>(a); break;
        case 16: run<16>(a); break;
        default: run<32>(a);
    }
    return hipSuccess;
}

}  // namespace kf
}  // namespace mpcqp
