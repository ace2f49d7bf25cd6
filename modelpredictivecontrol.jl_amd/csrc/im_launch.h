// im_launch.h -- arguments and host-side launch entry points of the InternalModel estimator (im_kernels.hip; bodies:
// im_bodies.h; src/estimator/internal_model.jl).  WEAK declarations, as in est_init_launch.h: a library linked without that
// unit (the stock CPU emulator libraries; libmpcqp_emu_im.so has the launchers of tests/emu/emu_im.cpp) still links, and
// mpcqp_im_set answers MPCQP_ERR_UNSUPPORTED (im_available()).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpcqp_types.h"

namespace mpcqp {
namespace im {

enum { IM_NMAX = 32 };          // max(nx, ny, nxs): the estimators' own limit

// One member owns a group of G consecutive lanes: a 16-lane row when max(nx, nu, ny, nd, nxs) <= 16 (four members per
// wavefront), the whole wavefront otherwise.  Lane r of a group owns row r of every matrix and entry r of every vector;
// vectors travel between the lanes of a group through LDS (IM_VEC slots of WAVE doubles), and two N x N matrices per group
// (N = 16 or 32, column-major with leading dimension N: the lanes of a group hit N different banks) hold what a kernel
// reads more than once: As and Cs of the recurrence, or the matrix and right-hand sides of an elimination.
//
// The stochastic model is the one on the MEASURED outputs: As (nxs,nxs), Bs (nxs,nym), Cs (nym,nxs), Ds (nym,nym), all
// column-major per member like the controller's model; the expansion to ny outputs (stoch_ym2y) only adds zero rows and
// columns, which no kernel stores.
struct ImArgs {
    const double *Ahat, *Bu, *C, *Bd, *Dd, *dop;     // the controller handle's model; dop = f̂op - x̂op or null
    const double* Bvec;                              // [B][nY] the model's B of the prediction (k_predmat)
    const int* i_ym;                                 // [nym]
    int B, nx, nu, ny, nd, nym, nxs, Hp, G;
    const double *As, *Bs, *Cs, *Ds;                 // [B][nxs*nxs], [B][nxs*nym], [B][nym*nxs], [B][nym*nym]
    double *Ahs, *Bhs;                               // Âs = As - B̂s Cs, B̂s = Bs Ds⁻¹ (written by the set-up)
    double *xs, *ys, *Yhs, *Beff, *z;                // x̂s [B][nxs], ŷs [B][ny], Ŷs [B][nY], B + Ŷs [B][nY], Âs x̂s + B̂s ŷs [B][nxs]
    int32_t* status;                                 // [B] 0, or 2: Ds singular, the stochastic part of the member is off
    const double *y0m, *d0, *u0;                     // per call: [B][nym], [B][nd] (null iff nd = 0), [B][nu]
    double* xhat0;                                   // [B][nx] x̂d = x̂0
    int32_t* init_status;                            // [B] initstate: 0 solved, 1 a singular system (nothing written)
};

enum { IM_SETUP = 0, IM_CORRECT, IM_UPDATE, IM_INIT, IM_BEFF };

inline int group_lanes(int nx, int nu, int ny, int nd, int nxs) {
    int n = nx;
    for (int v : {nu, ny, nd, nxs}) n = v > n ? v : n;
    return n <= 16 ? 16 : WAVE;
}
MPCQP_HD constexpr int mat_dim(int G) { return G == 16 ? 16 : IM_NMAX; }
enum { IM_VEC = 8, IM_MAT_DOUBLES = 2 * IM_NMAX * IM_NMAX, IM_LDS_DOUBLES = IM_MAT_DOUBLES + IM_VEC * WAVE };
static_assert(4 * 2 * 16 * 16 == IM_MAT_DOUBLES, "four 16-lane groups or one 64-lane group: the same matrix area");

inline bool dims_ok(int nx, int nu, int ny, int nd, int nym, int nxs) {
    return nx >= 1 && nu >= 1 && ny >= 1 && nd >= 0 && nym >= 1 && nym <= ny && nxs >= 1 && nx <= IM_NMAX && nu <= IM_NMAX &&
           ny <= IM_NMAX && nd <= IM_NMAX && nxs <= IM_NMAX;
}
inline bool args_ok(const ImArgs& a, int kind) {
    if (a.B < 1 || a.Hp < 1 || !dims_ok(a.nx, a.nu, a.ny, a.nd, a.nym, a.nxs) || a.G != group_lanes(a.nx, a.nu, a.ny, a.nd, a.nxs)) return false;
    if (!a.Bvec || !a.i_ym || !a.As || !a.Bs || !a.Cs || !a.Ds || !a.Ahs || !a.Bhs || !a.xs || !a.ys || !a.Yhs || !a.Beff || !a.z || !a.status)
        return false;
    if (kind == IM_SETUP || kind == IM_BEFF) return true;
    if (!a.Ahat || !a.Bu || !a.C || !a.xhat0 || (a.nd > 0 && (!a.Bd || !a.Dd || !a.d0))) return false;
    if (kind == IM_CORRECT) return a.y0m != nullptr;
    if (kind == IM_UPDATE) return a.u0 != nullptr;
    return a.y0m && a.u0 && a.init_status;
}
inline long waves(const ImArgs& a) { return ((long)a.B + (WAVE / a.G) - 1) / (WAVE / a.G); }

__attribute__((weak)) hipError_t launch_im(const ImArgs& a, int kind, hipStream_t st);
inline bool im_available() { return launch_im != nullptr; }

}  // namespace im
}  // namespace mpcqp
