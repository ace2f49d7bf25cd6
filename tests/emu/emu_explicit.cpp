// TEST INFRASTRUCTURE ONLY: the ExplicitMPC bodies (csrc/explicit_bodies.h) on the CPU.  Defines the launchers that
// csrc/explicit_launch.h declares weak, over the 64-lane wave of emu_wave.h: one controller per wavefront for the factorisation
// and the step, two "persistent" wavefronts for the law kernel (its loop over groups of 64 rows is exercised).  Linked only
// into libmpcqp_emu_explicit.so (tests/emu/explicit.mk); the stock emulator libraries have no such launcher and answer
// MPCQP_ERR_UNSUPPORTED to mpcqp_explicit_prepare.
#include "emu_wave.h"
#include "explicit_bodies.h"
#include "explicit_launch.h"

namespace mpcqp {
namespace ex {

hipError_t launch_explicit_factor(const FactorArgs& a, hipStream_t) {
    if (a.B < 1 || a.n < 1 || a.n > EX_NMAX || factor_lds_doubles(a.n) * sizeof(double) > EX_LDS_MAX) return hipErrorInvalidValue;
    run_waves(a.B, factor_lds_doubles(a.n), [&](EmuWave& w, int b, double* sm) { explicit_factor_body(w, a, b, sm); });
    return hipSuccess;
}
hipError_t launch_explicit_step(const StepArgs& a, hipStream_t) {
    if (a.d.B < 1 || a.d.nDU < 1 || a.d.nDU > EX_NMAX || step_lds_doubles(a.d) * sizeof(double) > EX_LDS_MAX || !a.Hinv)
        return hipErrorInvalidValue;
    run_waves(a.d.B, step_lds_doubles(a.d), [&](EmuWave& w, int b, double* sm) { explicit_step_body(w, a, b, sm); });
    return hipSuccess;
}
hipError_t launch_explicit_law(const LawArgs& a, hipStream_t) {
    if (a.B < 1 || a.rows < 1 || a.nwaves < 1 || a.kp < 1) return hipErrorInvalidValue;
    run_waves(a.nwaves, 0, [&](EmuWave& w, int wv, double*) { explicit_law_body(w, a, wv); });
    return hipSuccess;
}
hipError_t launch_explicit_law_unit(const LawBuildArgs& a, hipStream_t) {
    const int nt = a.nd > 0 ? a.Hp : 1;
    for (size_t b = 0; b < (size_t)a.B; ++b)
        for (int t = 0; t < nt; ++t) explicit_law_unit_at(a, b, t);
    return hipSuccess;
}
hipError_t launch_explicit_law_pack(const LawBuildArgs& a, hipStream_t) {
    for (size_t R = 0; R < (size_t)a.B * a.n; ++R) explicit_law_pack_at(a, R);
    return hipSuccess;
}
int explicit_law_waves_for(int, long groups) { return groups < 2 ? 1 : 2; }

}  // namespace ex
}  // namespace mpcqp
