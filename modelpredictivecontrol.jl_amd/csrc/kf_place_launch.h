// kf_place_launch.h -- arguments and host-side launch entry point of the pole placement of the Luenberger observer
// (kf_place_kernels.hip; body: kf_place_bodies.h).  WEAK declaration, as in est_init_launch.h: a library linked without the
// launcher (the stock CPU emulator libraries; libmpcqp_emu_kf_place.so has the one of tests/emu/emu_kf_place.cpp) still
// links, and mpcqp_kf_set_poles answers MPCQP_ERR_UNSUPPORTED (kf_place_available()).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpcqp_types.h"

namespace mpcqp {
namespace kf {

enum { PLACE_NMAX = 32 };                   // max(nx̂, nym): the estimators' own limit
enum { PLACE_OK = 0, PLACE_BROKE_DOWN = 2 };   // per-member status (2: the value the steady Riccati solve uses for a breakdown)
constexpr int PLACE_CAP_DEFAULT = 30, PLACE_CAP_MAX = 100;
constexpr double PLACE_DET_RTOL = 1e-3;     // the sweeps stop when |det X| moved by no more than this fraction of its value
constexpr double PLACE_VEC_TOL = 1e-8;      // a projection shorter than this is no direction
constexpr int PLACE_LDS_STORED_MAX = 8192;  // doubles (64 KB): up to here the reflectors of every T_j stay in LDS

// Everything in ABI layout (column-major inside a member), read where mpcqp_set_model / mpcqp_kf_set_poles left it: the
// launch sees the model that is resident at that moment.
struct PlaceArgs {
    const double *Ahat, *C;      // [B][nx*nx], [B][ny*nx]: Model::Ahat, Model::C
    const int* i_ym;             // [nym] measured rows of Ĉ
    const double* poles;         // [B][nx]
    double* K;                   // [B][nym][nx] K̂ (filter form), written with PLACE_OK only
    int32_t* status;             // [B] PLACE_OK / PLACE_BROKE_DOWN
    int32_t* sweeps;             // [B] sweeps run
    int B, nx, ny, nym;
    int cap;                     // most sweeps, 0 .. PLACE_CAP_MAX
    int stored;                  // 1: the reflectors of all nx admissible subspaces are kept in LDS; 0: recomputed at each visit
};

// LDS carve-up of one member, in doubles (n = nx, mm = min(nx, nym), q = n - mm the dimension of range(G)'s complement):
//   A  n*n   Â                          Q  n*n   [U0 U1] of G = [U0 U1][Z; 0]        AU n*q   Â U1
//   Z  mm*mm the triangle of G          XR n*n   reflectors of the QR of X           R  n*n   its triangle, then S'
//   WT n*q per kept subspace: the reflectors of T_j = (Â - λ_j I) U1
struct PlaceCarve {
    int A, Q, AU, Z, XR, R, WT, total;
};
MPCQP_HD inline PlaceCarve place_carve(int n, int nym, bool stored) {
    const int mm = nym < n ? nym : n, q = n - mm;
    PlaceCarve c;
    c.A = 0;
    c.Q = c.A + n * n;
    c.AU = c.Q + n * n;
    c.Z = c.AU + n * q;
    c.XR = c.Z + mm * mm;
    c.R = c.XR + n * n;
    c.WT = c.R + n * n;
    c.total = c.WT + n * q * (stored ? n : 1);
    return c;
}
inline bool place_stored_for(int nx, int nym) { return place_carve(nx, nym, true).total <= PLACE_LDS_STORED_MAX; }
inline size_t place_lds_bytes(const PlaceArgs& a) { return (size_t)place_carve(a.nx, a.nym, a.stored != 0).total * sizeof(double); }

inline int place_columns_for(int n) { return n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : 32; }
inline bool place_args_ok(const PlaceArgs& a) {
    return a.B >= 1 && a.nx >= 1 && a.nx <= PLACE_NMAX && a.nym >= 1 && a.nym <= PLACE_NMAX && a.nym <= a.ny && a.cap >= 0 &&
           a.cap <= PLACE_CAP_MAX && a.Ahat && a.C && a.i_ym && a.poles && a.K && a.status && a.sweeps &&
           (a.stored == 0 || (a.stored == 1 && place_stored_for(a.nx, a.nym))) && place_lds_bytes(a) <= 64 * 1024;
}

__attribute__((weak)) hipError_t launch_kf_place(const PlaceArgs& a, hipStream_t st);
inline bool kf_place_available() { return launch_kf_place != nullptr; }

}  // namespace kf
}  // namespace mpcqp
