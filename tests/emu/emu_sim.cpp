// TEST INFRASTRUCTURE ONLY: the plant of the closed-loop simulation and the fused loop of an explicit-law handle
// (csrc/sim_bodies.h) on the CPU.  Defines the launchers that csrc/sim_launch.h declares weak: the plant over the 64-lane wave
// of emu_wave.h, the fused loop over the 16-lane rows of emu_rowwave.h.  Linked only into libmpcqp_emu_sim.so
// (tests/emu/sim.mk); the other emulator libraries have no such launcher and answer MPCQP_ERR_UNSUPPORTED to
// mpcqp_sim_set_plant.
#include "emu_rowwave.h"
#include "emu_wave.h"
#include "sim_bodies.h"
#include "sim_launch.h"

namespace mpcqp {
namespace sim {

hipError_t launch_sim_plant(const PlantArgs& a, hipStream_t) {
    if (!plant_args_ok(a)) return hipErrorInvalidValue;
    run_waves((int)plant_waves(a), PLANT_LDS_DOUBLES, [&](EmuWave& w, int wv, double* sm) { sim_plant_body(w, a, wv, sm); });
    return hipSuccess;
}

hipError_t launch_sim_explicit(const FusedArgs& a, hipStream_t) {
    if (a.p.B < 1 || a.p.N < 1 || !fused_dims_ok(a.p) || fused_lds_doubles(a.p, a.ncol) * sizeof(double) > 160 * 1024) return hipErrorInvalidValue;
    using W = mhe::EmuRow16;
    mhe::run_row_waves<W>((int)fused_waves(a.p), fused_lds_doubles(a.p, a.ncol), [&](W& w, int wv, double* sm) { sim_explicit_body(w, a, wv, sm); });
    return hipSuccess;
}

}  // namespace sim
}  // namespace mpcqp
