// kf_cov_launch.h -- arguments and host-side launch entry points of the covariance / gain recursion of the time-varying
// KalmanFilter of the LinMPC loop (kf_kernels.hip; bodies: kf_cov_bodies.h).  WEAK declarations, as in mhe_wide_launch.h:
// a library linked without that unit (the stock CPU emulator tests/emu/libmpcqp_emu.so; libmpcqp_emu_est.so has the launchers
// of tests/emu/emu_kf_cov.cpp) still links, and mpcqp_kf_set_covariances answers MPCQP_ERR_UNSUPPORTED (kf_cov_available()).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mhe_types.h"

namespace mpcqp {
namespace kf {

// mode bits of one launch (3: both, P̂(k|k) stays in registers).  COV_NO_YM (without COV_CORRECT): the period has no
// measurement at all (ym = nothing) -- every estimator's correction is missed, its status becomes COV_MISSED
enum { COV_CORRECT = 1, COV_PREDICT = 2, COV_NO_YM = 4 };
// per-estimator status: what became of the last correction attempt.  COV_MISSED: skipped for a missing measurement (a NaN
// in the estimator's y0m row); P̂ and K̂ keep their bits and, unlike COV_DROPPED, the prediction of that period runs
enum { COV_OK = 0, COV_MISSED = 1, COV_DROPPED = 2 };

// Everything in ABI layout (column-major inside an estimator), read where mpcqp_set_model / mpcqp_kf_set_covariances
// left it: the launch sees the model that is resident at that moment.
struct CovArgs {
    const double *Ahat, *C;      // [B][nx*nx], [B][ny*nx]: Model::Ahat, Model::C
    const int* i_ym;             // [nym] measured rows of Ĉ
    const double *Q, *R;         // [B][nx*nx], [B][nym*nym]
    double* P;                   // [B][nx*nx]  P̂, in and out
    double* K;                   // [B][nym][nx] K̂ (KfParams::Khat / StepIO::kf_K), out of a correction
    int32_t* status;             // [B] COV_OK / COV_MISSED / COV_DROPPED
    int B, nx, ny, nym;
    int NX;                      // register columns: mhe::register_columns_for(max(nx, nym))
    int nwaves;                  // wavefronts launched (each loops over groups of GPW estimators)
    const double* y0m;           // [B][nym] measurements of a COV_CORRECT launch (any(isnan) of a row: that estimator's
                                 // correction is missed), or null: every correction runs
};
// what every launcher (kf_kernels.hip, tests/emu/emu_kf_cov.cpp) checks before it picks a kernel for a.NX
inline bool kf_cov_args_ok(const CovArgs& a) { return a.B >= 1 && a.nwaves >= 1 && a.nx >= 1 && a.nym >= 1 && a.nx <= a.NX && a.nym <= a.NX; }

__attribute__((weak)) hipError_t launch_kf_cov(const CovArgs& a, int mode, hipStream_t st);
__attribute__((weak)) int kf_cov_waves_for(int device, int B, int NX);      // size of the persistent grid
inline bool kf_cov_available() { return launch_kf_cov && kf_cov_waves_for; }
// register columns: a multiple of four up to 16 (one DPP row per estimator), of eight above (24, 32: one wavefront each)
inline int kf_cov_columns_for(int nmax) { return nmax <= mhe::RL ? 4 * ((nmax + 3) / 4) : 8 * ((nmax + 7) / 8); }
inline int kf_cov_lanes_for(int NX) { return NX <= mhe::RL ? mhe::RL : mhe::WIDE_RL; }

}  // namespace kf
}  // namespace mpcqp
