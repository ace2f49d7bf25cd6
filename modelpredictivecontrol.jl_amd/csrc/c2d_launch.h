// c2d_launch.h -- arguments and host-side launch entry point of the discretisation of a batch of continuous-time models
// (c2d_kernels.hip; body: c2d_bodies.h).  WEAK declaration, as in est_init_launch.h / kf_place_launch.h: a library linked
// without the launcher (the stock CPU emulator libraries; libmpcqp_emu_c2d.so has the one of tests/emu/emu_c2d.cpp) still
// links, and mpcqp_c2d / mpcqp_set_model_continuous answer MPCQP_ERR_UNSUPPORTED (c2d_available()).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpcqp_types.h"

namespace mpcqp {
namespace c2d {

enum { C2D_NMAX = 32 };                     // block order nx + nu (+ nd under ZOH), and nx, ny, nd of the Tustin block
enum { C2D_NXH_MAX = 64 };                  // nx̂ = nx_dis + Σnint_u + Σnint_ym: one row of the augmented model per lane
enum { C2D_OK = 0, C2D_REFUSED = 2 };       // per-member status
enum { C2D_TUSTIN = 0, C2D_ZOH = 1 };       // d_method (MPCQP_C2D_TUSTIN / MPCQP_C2D_ZOH of include/mpcqp.h)
constexpr int C2D_SQ_MAX = 64;              // most squarings: a member whose scaled norm needs more is refused
constexpr double C2D_THETA13 = 5.371920351148152;      // Higham (2005): the [13/13] Padé approximant is accurate to the unit
                                                       // roundoff of doubles up to this norm

// Inputs in the layouts of mpcqp_set_model (column-major inside a member), continuous time.  Outputs: the discrete,
// augmented model; written for a member with C2D_OK only.
struct C2dArgs {
    const double *A, *Bu, *C, *Bd, *Dd;     // [B][nx*nx], [B][nx*nu], [B][ny*nx], [B][nx*nd], [B][ny*nd] (Bd, Dd: nd > 0)
    const double* Ts;                       // [B]
    const double* dop;                      // [B][nxd] f̂op - x̂op of the plant states, may be null
    double *Ahat, *Bhu, *Chat, *Bhd, *Dhd;  // [B][nxh*nxh], [B][nxh*nu], [B][ny*nxh], [B][nxh*nd], [B][ny*nd]
    double* dophat;                         // [B][nxh] dop padded with zeros (null iff dop is null)
    int32_t* status;                        // [B]
    int B, nx, nu, ny, nd, method;
    int nsu, nsy;                           // Σnint_u, Σnint_ym
    int nxd, nxh;                           // order of the discrete plant (nx, or 2 nx with the Tustin block) and of the augmented model
    // the stochastic states s = 0 .. nsu + nsy - 1 (init_estimstoch): s_in[s] the input i with Cs_u(i, s) = 1, s_out[s] the
    // output row i with Cs_y(i, s) = 1 (-1: none), s_prev[s] = 1 iff As(s, s-1) = 1 (s-1 is in the same chain of integrators)
    signed char s_in[C2D_NXH_MAX], s_out[C2D_NXH_MAX], s_prev[C2D_NXH_MAX];
};

MPCQP_HD inline bool c2d_tustin(const C2dArgs& a) { return a.nd > 0 && a.method == C2D_TUSTIN; }
MPCQP_HD inline int c2d_order(const C2dArgs& a) { return a.nx + a.nu + (a.nd > 0 && a.method == C2D_ZOH ? a.nd : 0); }

// Register columns NX of the member's rows: the block order, and with the Tustin block ny and nd too (C and Bd are operands
// of its products) rounded up to 4, 8, 16 or 32
inline int c2d_columns_for(int n) { return n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : 32; }
inline int c2d_need(const C2dArgs& a) {
    int n = c2d_order(a);
    if (c2d_tustin(a)) n = n > a.ny ? n : a.ny, n = n > a.nd ? n : a.nd;
    return n;
}

// LDS of one member: seven NX x NX matrices, column-major with leading dimension NX, zero beyond the live part.
//   the exponential:  M0 = M Ts / 2^s   M1, M2, M3 = its 2nd, 4th, 6th power   M4 = right operand of the Padé products, then
//                     the pivot row of the solve   M5 = exp(M Ts): [Φ Γu (Γd); 0 I]   (M6 unused)
//   the Tustin block: M0 = A, then C, then Dt   M1 = W = (I - aA)^-1   M2 = I + aA, then Bd Ts, then Bd   M3 = At   M4 = the
//                     pivot row, then Bt   M6 = Ct
enum { C2D_NBUF = 7 };
inline size_t c2d_lds_bytes(int NX) { return (size_t)C2D_NBUF * NX * NX * sizeof(double); }

inline bool c2d_dims_ok(const C2dArgs& a) {
    return a.B >= 1 && a.nx >= 1 && a.nu >= 1 && a.ny >= 1 && a.nd >= 0 && (a.method == C2D_TUSTIN || a.method == C2D_ZOH) &&
           a.nsu >= 0 && a.nsy >= 0 && a.nxd == (c2d_tustin(a) ? 2 * a.nx : a.nx) && a.nxh == a.nxd + a.nsu + a.nsy;
}
inline bool c2d_supported(const C2dArgs& a) { return c2d_need(a) <= C2D_NMAX && a.nxh <= C2D_NXH_MAX; }
inline bool c2d_args_ok(const C2dArgs& a) {
    return c2d_dims_ok(a) && c2d_supported(a) && a.A && a.Bu && a.C && a.Ts && (a.nd == 0 || (a.Bd && a.Dd)) && a.Ahat && a.Bhu &&
           a.Chat && (a.nd == 0 || (a.Bhd && a.Dhd)) && (!a.dop == !a.dophat) && a.status;
}

__attribute__((weak)) hipError_t launch_c2d(const C2dArgs& a, hipStream_t st);
inline bool c2d_available() { return launch_c2d != nullptr; }

}  // namespace c2d
}  // namespace mpcqp
