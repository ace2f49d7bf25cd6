// explicit_launch.h -- arguments and host-side launch entry points of the ExplicitMPC kernels (explicit_kernels.hip; bodies:
// explicit_bodies.h).  WEAK declarations, as in kf_cov_launch.h: a library linked without that unit (the stock CPU emulator
// tests/emu/libmpcqp_emu.so; libmpcqp_emu_explicit.so has the launchers of tests/emu/emu_explicit.cpp) still links, and
// mpcqp_explicit_prepare answers MPCQP_ERR_UNSUPPORTED (explicit_available()).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpcqp_types.h"

namespace mpcqp {
namespace ex {

enum { EX_OK = 0, EX_FAILED = 2 };         // per-controller status of the factorisation (MPCQP_STATUS_OPTIMAL / _ERROR)
enum { EX_NMAX = WAVE };                   // nZ~ = nDU <= 64: one row of H~ per lane
enum { EX_LDS_MAX = 160 * 1024 };          // the LDS of a CU: the bound of the condensed step kernels (mpcqp_host.hip: condensed_fits)

// What k_explicit_factor leaves per controller:
//   Hinv  H~^-1 = L^-T L^-1, its lower triangle packed row-major, entry (i, j <= i) at tri(i) + j: half the bytes of the square,
//         which is what the step pays for every period (zeros for a controller whose factorisation failed)
//   Lsum  [n] per (move j, channel c): sum of the diagonal L weights over the steps t >= j_j -- with R^u = 0 (the default
//         R^u = Uop) the input-weight term of q~ is 2 Lsum lastu0[c] and the horizon of L is not read per period
MPCQP_HD constexpr int tri(int i) { return i * (i + 1) / 2; }
struct FactorArgs {
    const double* Hpk;       // [B][npk]  Model::Hpk
    const double* Ldiag;     // [B][Hp][nu] Model::Ldiag
    const int* jl;           // Model::jl
    double* Hinv;            // [B][tri(n)]
    double* Lsum;            // [B][n]
    int32_t* status;         // [B] EX_OK / EX_FAILED
    int B, n, npk, nu, Hp;
};
// dense H~, then L^-1: 2 n^2 doubles
inline size_t factor_lds_doubles(int n) { return (size_t)2 * n * n; }

// One explicit period (k_explicit_step).  Pointers and layouts of mpcqp_step_device; Z is output only.
struct StepArgs {
    Dims d;                  // d.flags: MPCQP_FLAG_RY_CONSTANT is read (bit 0)
    Model m;
    const double *xhat0, *lastu0, *Ry, *Ru, *d0, *Dhat0;
    double *Z, *u0, *Yhat0;  // Yhat0 may be null
    int32_t* status;
    double *q_keep, *F_keep; // optional (MPCQP_FLAG_KEEP_QP)
    const double* Hinv;      // FactorArgs::Hinv
    const double* Lsum;      // FactorArgs::Lsum
    const int32_t* fstatus;  // FactorArgs::status
};
// LDS of one period, in doubles: F [nY], T [max(nY, 64)] = M (F - R^y) and, once q~ has it, the 64-word exchange buffer of the
// dense-L_Hp sum and of Y^0, the step-response table [Hp][ny][nu] and the packed H~^-1.  This is below the carve-up of the
// condensed step kernel (mpcqp_bodies.h: make_carve holds the table, the packed H~, 2 nY and 7 nZ~ words) for every nY >= 64,
// and under 51 KB for nY < 64, nZ~ <= 64: every handle with a condensed Hessian (mpcqp_host.hip: condensed_fits, 160 KB) and
// nZ~ <= 64 fits, whatever Hp.
inline size_t step_lds_doubles(const Dims& d) {
    return (size_t)d.nY + (size_t)(d.nY > WAVE ? d.nY : WAVE) + (size_t)d.Hp * d.ny * d.nu + (size_t)tri(d.nDU);
}

// The law tables.  A table has `rows` rows per controller (nZ~ for all of Z~, nu for u0 alone) and ncol = 1 + nx + nu + ny + nd
// columns [g0 Gx Gu Gr Gd].  The rows of the whole batch are numbered R = b * rows + i and one lane of k_explicit_law owns one
// of them; columns come in pairs.  Entry (R, k) lives at
//     ((R / 64) * kp + k / 2) * 128 + (R % 64) * 2 + (k & 1),        kp = (ncol + 1) / 2
// so that the 64 lanes of a wavefront read 64 consecutive 16-byte pairs (1 KB) per load, whatever `rows` is.
inline int law_ncol(const Dims& d) { return 1 + d.nxh + d.nu + d.ny + d.nd; }
inline int law_kp(const Dims& d) { return (law_ncol(d) + 1) / 2; }
MPCQP_HD inline size_t law_index(size_t R, int k, int kp) { return ((R / WAVE) * kp + (size_t)(k >> 1)) * (2 * WAVE) + (R % WAVE) * 2 + (size_t)(k & 1); }
inline size_t law_doubles(const Dims& d, int rows) { return (((size_t)d.B * rows + WAVE - 1) / WAVE) * law_kp(d) * 2 * WAVE; }

struct LawArgs {
    const double* table;     // see above
    const double *xhat0, *lastu0, *ry, *d0;     // [B][nx], [B][nu], [B][ny], [B][nd]
    double* Z;               // [B][rows] or null (rows == nu: u0 alone)
    double* u0;              // [B][nu]
    int32_t* status;         // [B]
    const int32_t* fstatus;  // [B]
    int B, rows, nx, nu, ny, nd, kp;
    int nwaves;              // wavefronts launched (each loops over groups of 64 rows)
};

// Building the tables by superposition (once per model): `unit` writes the inputs of column k of the law into the zeroed
// input buffers of a step, `pack` stores Z(k) - Z(0) (k = 0: Z(0)) as column k of both tables.
struct LawBuildArgs {
    double *xhat0, *lastu0, *ry, *d0, *Dhat0;   // unit inputs (zeroed by the host)
    const double *Zk, *Z0;                      // [B][n]
    double *table_z, *table_u;
    int B, n, nx, nu, ny, nd, Hp, kp, k;
};

__attribute__((weak)) hipError_t launch_explicit_factor(const FactorArgs& a, hipStream_t st);
__attribute__((weak)) hipError_t launch_explicit_step(const StepArgs& a, hipStream_t st);
__attribute__((weak)) hipError_t launch_explicit_law(const LawArgs& a, hipStream_t st);
__attribute__((weak)) hipError_t launch_explicit_law_unit(const LawBuildArgs& a, hipStream_t st);
__attribute__((weak)) hipError_t launch_explicit_law_pack(const LawBuildArgs& a, hipStream_t st);
__attribute__((weak)) int explicit_law_waves_for(int device, long groups);      // size of the persistent grid
inline bool explicit_available() {
    return launch_explicit_factor && launch_explicit_step && launch_explicit_law && launch_explicit_law_unit &&
           launch_explicit_law_pack && explicit_law_waves_for;
}

}  // namespace ex
}  // namespace mpcqp
