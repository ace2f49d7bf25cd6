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
// The square-root form of the body (kf_dare_bodies.h, PSD = true) factors H(k) = L L' without pivoting and drops the columns of pivots <= 0.  A
// pivot below -DARE_PSD_NEG max(1, max diag H(k)) is not rounding: H(k) is indefinite and the estimator breaks down.
// (Measured: rounding pivots down to -5.6e-14 on the shapes of the tests; the indefinite member of the tests has -1e-3.)
constexpr double DARE_PSD_NEG = 1e-8;
// A Q̂ whose smallest pivot is at or below DARE_PSD_SING max diag Q̂ is numerically singular (relative to Q̂'s own size: a
// small definite Q̂ such as 1e-11 I stays with the definite body).  The definite body may
// still get through it -- a pivot that is zero in exact arithmetic comes out of the rounding with either sign, and a
// positive one passes its test, H(0)⁻¹ then has entries of 1e16 and the result is wrong with status 0 (measured: 17 % off in
// P̂∞ for a rank-one Q̂ block) -- so the second pass takes such an estimator whatever the first one said about it.
constexpr double DARE_PSD_SING = 1e-10;
// The square-root body takes H for converged only once max|A(k+1)| <= DARE_PSD_STAB as well: the closed-loop transition
// matrix over 2^(k+1) periods is dying out (it squares with every iteration, so any bound below 1 tells a stable mode from
// one on the unit circle; see kf_dare_bodies.h).
constexpr double DARE_PSD_STAB = 0.5;

// per-estimator status of the last solve.  DARE_NOT_CONVERGED: the cap was reached (the reference's "Cannot compute the
// optimal Kalman gain", kalman.jl:211-221: an undetectable pair).  DARE_BROKE_DOWN: a pivot of R̂, H(k) or H(k)⁻¹ + G(k)
// was outside (0, inf) (square-root body: a pivot of I + L'GL, or one of H(k) below -DARE_PSD_NEG), or a value was not
// finite.  K̂ and P̂ of an estimator are written with DARE_OK only (and zeroed by the second pass where it refuses an
// estimator the first pass had served).
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
    int32_t* path;               // [B] 1: the square-root body ran for this estimator (second pass); 0: the definite body's result stands
};
// what every launcher (kf_kernels.hip, tests/emu/emu_kf_dare.cpp) checks before it picks a kernel for a.NX
inline bool kf_dare_args_ok(const DareArgs& a) { return a.B >= 1 && a.nwaves >= 1 && a.nx >= 1 && a.nym >= 1 && a.nx <= a.NX && a.nym <= a.NX; }

__attribute__((weak)) hipError_t launch_kf_dare(const DareArgs& a, hipStream_t st);
__attribute__((weak)) int kf_dare_waves_for(int device, int B, int NX);     // size of the persistent grid
inline bool kf_dare_available() { return launch_kf_dare && kf_dare_waves_for; }

// Second pass over the batch, on the same stream right after launch_kf_dare and with the same arguments: the estimators
// that the definite body left with DARE_BROKE_DOWN (a semidefinite Q̂: H(0)⁻¹ does not exist) or whose Q̂ is numerically
// singular (DARE_PSD_SING) are solved again by the square-root body; every other estimator's K̂, P̂∞, status, iters and path
// are not touched.  Such an estimator that the square-root body refuses after the definite body had written a result gets
// zeros in K̂ and P̂∞.  A library without this launcher
// (the stock emulator, tests/emu/libmpcqp_emu_est.so) keeps the result of the first pass.
__attribute__((weak)) hipError_t launch_kf_dare_psd(const DareArgs& a, hipStream_t st);
inline bool kf_dare_psd_available() { return kf_dare_available() && launch_kf_dare_psd; }

}  // namespace kf
}  // namespace mpcqp
