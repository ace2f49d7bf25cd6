// est_init_launch.h -- arguments and host-side launch entry point of the estimator half of initstate! (est_kernels.hip; body:
// est_init_bodies.h).  WEAK declaration, as in sim_launch.h: a library linked without that unit (the stock CPU emulator
// libraries; libmpcqp_emu_mheloop.so has the launcher of tests/emu/emu_est_init.cpp) still links, and mpcqp_est_initstate
// answers MPCQP_ERR_UNSUPPORTED (est_init_available()).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpcqp_types.h"

namespace mpcqp {
namespace est {

enum { EST_INIT_NMAX = 32 };    // max(nx̂, nym): the estimators' own limit, so nx̂ + nym <= 64 rows = one wavefront

// One launch of k_est_init<NX>: init_estimate! (src/estimator/execute.jl:246-259) of every member,
//   [I - Â; Ĉm] x̂0 = [B̂u u0 + B̂d d0 + (f̂op - x̂op); y0m - D̂dm d0]
// in the least-squares sense by Householder QR without pivoting.  One member per wavefront; lane r owns row r of the
// (nx̂ + nym) x nx̂ matrix and of the right-hand side, the row's NX column entries in registers.
struct InitArgs {
    const double *Ahat, *Bu, *C, *Bd, *Dd, *fx;      // the controller handle's model (ABI layout, column-major per member); fx = f̂op - x̂op or null
    const int* i_ym;                                 // [nym] rows of Ĉ / D̂d that are measured
    int B, nx, nu, ny, nd, nym;
    const double *u0, *y0m, *d0;                     // [B][nu], [B][nym], [B][nd] (null iff nd = 0)
    double* xhat0;                                   // [B][nx]  written for the members that solved (status 0), untouched otherwise
    int32_t* status;                                 // [B]      0 solved, 1 no full column rank
};

inline int init_columns_for(int nx) { return nx <= 4 ? 4 : nx <= 8 ? 8 : nx <= 16 ? 16 : 32; }
inline bool init_args_ok(const InitArgs& a) {
    return a.B >= 1 && a.nx >= 1 && a.nx <= EST_INIT_NMAX && a.nym >= 1 && a.nym <= EST_INIT_NMAX && a.nym <= a.ny && a.nu >= 0 &&
           a.nd >= 0 && a.nx + a.nym <= WAVE && a.Ahat && a.C && a.i_ym && a.y0m && a.xhat0 && a.status && (a.nu == 0 || (a.Bu && a.u0)) &&
           (a.nd == 0 || (a.Bd && a.Dd && a.d0));
}

__attribute__((weak)) hipError_t launch_est_init(const InitArgs& a, hipStream_t st);
inline bool est_init_available() { return launch_est_init != nullptr; }

}  // namespace est
}  // namespace mpcqp
