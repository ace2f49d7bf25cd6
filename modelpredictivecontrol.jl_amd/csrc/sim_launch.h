// sim_launch.h -- arguments and host-side launch entry point of the plant kernel of the closed-loop simulation (sim_kernels.hip;
// body: sim_bodies.h).  WEAK declaration, as in explicit_launch.h: a library linked without that unit (the stock CPU emulator
// libraries; libmpcqp_emu_sim.so has the launcher of tests/emu/emu_sim.cpp) still links, and mpcqp_sim_set_plant answers
// MPCQP_ERR_UNSUPPORTED (sim_available()).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpcqp_types.h"

namespace mpcqp {
namespace sim {

enum { SIM_NMAX = WAVE };       // plant states, inputs, outputs, disturbances: at most one lane each inside a group

// One launch of k_sim_plant.  A controller owns a group of G consecutive lanes, G the power of two >= max(nxp, nu, ny, nd, nym),
// so a wavefront serves 64 / G controllers; lane r of a group owns row r of every vector.  Which parts of sim_closedloop!
// (src/plot_sim.jl:291-311) the launch runs is told by three period indices, -1 = not in this launch:
//   i_est   X̂ and Ŷ = Ĉ x̂0 + D̂d d0 of that period, after the correction (alone in its launch)
//   i_tail  ud0 = u0 + u_step + σu∘w_u, records U and Ud, lastu0 <- u0, status, x0 <- A x0 + Bu ud0 + Bd d0 + fx + σx∘w_x
//   i_head  d0 = d + d_step + σd∘w_d, y0 = C x0 + Dd d0 + y_step + σy∘w_y, y0m = y0[i_ym], records D, X, Y; the set point of the
//           period into ry_cur when ry comes per period, repeat(d0, Hp) into Dhat0 when the controller reads a horizon
// Records are [B][N][n], draws [B][N][n] (ABI (n,N,B)); every record pointer may be null.
struct PlantArgs {
    const double *A, *Bu, *C, *Bd, *Dd, *fx;         // the plant: [B][nxp][nxp], [B][nu][nxp], [B][nxp][ny], [B][nd][nxp], [B][nd][ny], [B][nxp]
    const double *Chat, *Dhd;                        // the estimator's Ĉ [B][nxh][ny], D̂d [B][nd][ny] (i_est)
    const int* i_ym;                                 // [nym]
    int B, nxp, nu, ny, nd, nym, nxh, Hp, N, G;
    int i_est, i_tail, i_head;
    const double *ry, *d;                            // [B][ny] or [B][N][ny] (ry_per_period), [B][nd]
    int ry_per_period;
    const double *u_step, *y_step, *d_step;          // [B][n] or null
    const double *su, *sy, *sd, *sx;                 // σ, [B][n] or null
    const double *wu, *wy, *wd, *wx;                 // standard-normal draws, [B][N][n]; read only with their σ
    double* x;                                       // [B][nxp] in/out
    const double* xhat;                              // [B][nxh]
    double* lastu0;                                  // [B][nu]
    const double* u0;                                // [B][nu] what the controller left
    const int32_t* st;                               // [B] its status
    double *d0, *y0m, *ry_cur, *Dhat0;               // per-period buffers: [B][nd], [B][nym], [B][ny] or null, [B][Hp][nd] or null
    double *Y, *X, *D, *Xhat, *Yhat, *U, *Ud;
    int32_t* status;                                 // [B][N] or null
    const double* yhs;                               // [B][ny] or null: added to Ŷ (i_est), the ŷs of an InternalModel
};

inline int group_lanes(int nxp, int nu, int ny, int nd, int nym) {
    int n = nxp;
    for (int v : {nu, ny, nd, nym}) n = v > n ? v : n;
    int G = 1;
    while (G < n) G *= 2;
    return G;
}
inline bool plant_args_ok(const PlantArgs& a) {
    const int G = a.G;
    return a.B >= 1 && a.N >= 1 && G >= 1 && G <= WAVE && (G & (G - 1)) == 0 && a.nxp >= 1 && a.nxp <= G && a.nu >= 1 && a.nu <= G &&
           a.ny >= 1 && a.ny <= G && a.nd >= 0 && a.nd <= G && a.nym >= 1 && a.nym <= a.ny && a.nxh >= 1 && a.Hp >= 1 &&
           a.i_est < a.N && a.i_tail < a.N && a.i_head < a.N && (a.i_est < 0 || (a.i_tail < 0 && a.i_head < 0)) &&
           a.A && a.Bu && a.C && a.x && a.y0m && a.i_ym && (a.nd == 0 || (a.d && a.d0)) &&
           (a.i_tail < 0 || (a.u0 && a.lastu0)) && (a.i_est < 0 || (a.xhat && a.Chat)) && (!a.ry_per_period || !a.ry_cur || a.ry) &&
           (!a.su || a.wu) && (!a.sy || a.wy) && (!a.sd || a.wd) && (!a.sx || a.wx);
}
inline long plant_waves(const PlantArgs& a) { return ((long)a.B + (WAVE / a.G) - 1) / (WAVE / a.G); }
enum { PLANT_LDS_DOUBLES = 4 * WAVE };             // x, ud / ŷ, d, y of every group

__attribute__((weak)) hipError_t launch_sim_plant(const PlantArgs& a, hipStream_t st);
inline bool sim_available() { return launch_sim_plant != nullptr; }

// The whole N-period loop of an explicit-law handle with a steady gain in ONE launch (k_sim_explicit).  One controller per
// 16-lane row, four per wavefront; lane r owns row r of every table and of every vector.  The tables -- Ĉm, D̂dm, K̂, Ĉ, D̂d, Â,
// B̂u, B̂d, the plant's A, Bu, Bd, C, Dd and the nu rows of the u0 law -- are loaded ONCE into the lane's own LDS block (row-major,
// compact in the handle's dimensions; a lane reads only what it wrote, so no barrier orders it); vectors travel by
// row_newbcast.  The loop reads the draws and writes the records that were asked for; x0, x̂0 and lastu0 go back at the end.
// Registers were not kept for the tables: at C3 dimensions they are 141 doubles per lane padded to the unrolled widths,
// 282 VGPRs, below two wavefronts per SIMD; in LDS they are 864 doubles (6.9 KB) per controller, 27 KB per wavefront: five wavefronts per CU.
enum { FUSED_RL = 16 };
struct FusedArgs {
    PlantArgs p;                                     // plant, dimensions, inputs, draws, state, records (i_*, u0, st, d0, y0m, ry_cur, Dhat0 unused)
    const double *Ahat, *Bhu, *Bhd, *dop;            // the estimator's model; Chat, Dhd in p
    const double* Khat;                              // [B][nym][nxh]
    const double* law;                               // the u0 table of explicit_launch.h (law_index), kp column pairs
    const int32_t* fstatus;                          // [B] status of the factorisation
    int kp, ncol, direct;
};
// doubles of one controller's tables: rows x columns (padded to a multiple of four) of each, in the order the body lays them out
inline int fused_ctrl_doubles(const PlantArgs& p, int) {
    auto c = [](int n) { return (n + 3) & ~3; };
    return p.nym * (c(p.nxh) + c(p.nd)) + p.nxh * c(p.nym) + p.ny * (c(p.nxh) + c(p.nd)) + p.nxh * (c(p.nxh) + c(p.nu) + c(p.nd)) +
           p.nxp * (c(p.nxp) + c(p.nu) + c(p.nd)) + p.ny * (c(p.nxp) + c(p.nd)) + p.nu * (4 + c(p.nxh) + c(p.nu) + c(p.ny) + c(p.nd));
}
inline size_t fused_lds_doubles(const PlantArgs& p, int ncol) { return (size_t)4 * fused_ctrl_doubles(p, ncol); }
inline bool fused_dims_ok(const PlantArgs& p) {
    for (int v : {p.nxh, p.nxp, p.nu, p.ny, p.nd, p.nym})
        if (v > FUSED_RL) return false;
    return true;
}
inline long fused_waves(const PlantArgs& p) { return ((long)p.B + 3) / 4; }
__attribute__((weak)) hipError_t launch_sim_explicit(const FusedArgs& a, hipStream_t st);
inline bool sim_fused_available() { return launch_sim_explicit != nullptr; }

}  // namespace sim
}  // namespace mpcqp
