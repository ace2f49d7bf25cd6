// kf_dare_launch.h -- arguments and host-side launch entry points of the steady-state Riccati solve of the
// SteadyKalmanFilter (kf_kernels.hip; body: kf_dare_bodies.h).  WEAK declarations, as in kf_cov_launch.h: a library linked
// without the launcher (the stock CPU emulator tests/emu/libmpcqp_emu.so; libmpcqp_emu_est.so has the one of
// tests/emu/emu_kf_dare.cpp) still links, and mpcqp_kf_set_steady answers MPCQP_ERR_UNSUPPORTED (kf_dare_available()).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kf_cov_launch.h"

namespace mpcqp {
namespace kf {

// The doubling iteration stops when max|H(k+1) - H(k)| <= DARE_TOL max(1, max|H(k+1)|), or after DARE_MAX_ITER iterations.
// (Measured: 6 - 11 iterations on the shapes of the tests, 18 for Q̂ = 1e-8 I; every iteration squares the closed-loop
// transition matrix, so 40 of them cover a spectral radius of 1 - 1e-11.)  Constants, not options.
constexpr int DARE_MAX_ITER = 40;
constexpr double DARE_TOL = 1e-13;

// per-estimator status of the last solve.  DARE_NOT_CONVERGED: the cap was reached (the reference's "Cannot compute the
// optimal Kalman gain", kalman.jl:211-221: an undetectable pair).  DARE_BROKE_DOWN: a pivot of R̂, H(k) or H(k)⁻¹ + G(k)
// was outside (0, inf), or a value was not finite.  K̂ and P̂ of an estimator are written with DARE_OK only.
enum { DARE_OK = 0, DARE_NOT_CONVERGED = 1, DARE_BROKE_DOWN = 2 };

// Everything in ABI layout (column-major inside an estimator), read where mpcqp_set_model / mpcqp_kf_set_steady left it:
// the launch sees the model that is resident at that moment.
struct DareArgs {
    const double *Ahat, *C;      // [B][nx*nx], [B][ny*nx]: Model::Ahat, Model::C
    const int* i_ym;             // [nym] measured rows of Ĉ
    const double *Q, *R;         // [B][nx*nx], [B][nym*nym]
    double* K;                   // [B][nym][nx] K̂ (filter form: P̂ Ĉm' (Ĉm P̂ Ĉm' + R̂)⁻¹), out
    double* P;                   // [B][nx*nx]  P̂∞ (of the predictor DARE), out
    int32_t* status;             // [B] DARE_OK / DARE_NOT_CONVERGED / DARE_BROKE_DOWN
    int32_t* iters;              // [B] doubling iterations run
    int B, nx, ny, nym;
    int NX;                      // register columns: kf_cov_columns_for(max(nx, nym))
    int nwaves;                  // wavefronts launched (each loops over groups of GPW estimators)
};
// what every launcher (kf_kernels.hip, tests/emu/emu_kf_dare.cpp) checks before it picks a kernel for a.NX
inline bool kf_dare_args_ok(const DareArgs& a) { return a.B >= 1 && a.nwaves >= 1 && a.nx >= 1 && a.nym >= 1 && a.nx <= a.NX && a.nym <= a.NX; }

__attribute__((weak)) hipError_t launch_kf_dare(const DareArgs& a, hipStream_t st);
__attribute__((weak)) int kf_dare_waves_for(int device, int B, int NX);     // size of the persistent grid
inline bool kf_dare_available() { return launch_kf_dare && kf_dare_waves_for; }

}  // namespace kf
}  // namespace mpcqp
