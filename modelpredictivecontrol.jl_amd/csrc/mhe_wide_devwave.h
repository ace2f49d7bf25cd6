// mhe_wide_devwave.h -- gfx950 wave interface of the WIDE MovingHorizonEstimator kernels (16 < max(nx̂, nym) <= 32): one
// estimator per wavefront, lane r < NX owns row r.  The bodies (mhe_bodies.h) are the ones of the 16-lane-row kernels;
// what changes is how a lane reaches another lane's value:
//   * a row-lane broadcast is a wave-uniform one -- v_readlane_b32 of the two halves into a scalar pair, which the
//     v_fma_f64 takes as an operand (DevWave::lane_value).  No DPP, so none of its wait states and no inline assembly:
//     the compiler schedules the scalar reads and covers their hazards itself;
//   * the reductions are DevWave's full-wave ones (DPP inside the rows, row_bcast across them);
//   * the NX x NX x NX products go through LDS to the matrix cores (Ops::mm_staged in mhe_bodies.h) when the interface
//     carries a staging buffer (MheWideMfmaWave); MheWideDevWave keeps them on the broadcasts.
#pragma once
#include "mhe_devwave.h"
#include "mhe_types.h"

namespace mpcqp {
namespace mhe {

struct MheWideDevWave : MheDevWave {
    static constexpr int GL = WIDE_RL, GPW = WIDE_GPW;      // lanes per estimator, estimators per wavefront (WaveGeom)
    template <int C>
    __device__ __forceinline__ double rowbc(double v) const { return lane_value(v, C); }
    template <int L0, int L1, int L2, int L3>
    __device__ __forceinline__ void fmabc4(double& acc, double x0, double x1, double x2, double x3, double y0, double y1,
                                           double y2, double y3) const {
        acc = fma(lane_value(x0, L0), y0, acc); acc = fma(lane_value(x1, L1), y1, acc);
        acc = fma(lane_value(x2, L2), y2, acc); acc = fma(lane_value(x3, L3), y3, acc);
    }
    template <int L0, int L1, int L2, int L3>
    __device__ __forceinline__ void rank1bc4(double& a0, double& a1, double& a2, double& a3, double x, double y0, double y1,
                                             double y2, double y3) const {
        a0 = fma(lane_value(x, L0), y0, a0); a1 = fma(lane_value(x, L1), y1, a1);
        a2 = fma(lane_value(x, L2), y2, a2); a3 = fma(lane_value(x, L3), y3, a3);
    }
    template <int L0, int L1, int L2, int L3>
    __device__ __forceinline__ void fmsbc4(double& acc, double x0, double x1, double x2, double x3, double y0, double y1,
                                           double y2, double y3) const {
        acc = fma(-lane_value(x0, L0), y0, acc); acc = fma(-lane_value(x1, L1), y1, acc);
        acc = fma(-lane_value(x2, L2), y2, acc); acc = fma(-lane_value(x3, L3), y3, acc);
    }
    // a_i <- a_i + g (a_i of lane K): the pivot row is read before any of the four is written
    template <int K>
    __device__ __forceinline__ void gjacc4(double& a0, double& a1, double& a2, double& a3, double g) const {
        const double p0 = lane_value(a0, K), p1 = lane_value(a1, K), p2 = lane_value(a2, K), p3 = lane_value(a3, K);
        a0 = fma(p0, g, a0); a1 = fma(p1, g, a1); a2 = fma(p2, g, a2); a3 = fma(p3, g, a3);
    }
    __device__ __forceinline__ double rsum(double v) { return sum(v); }
    __device__ __forceinline__ double rmin(double v) { return minv(v); }
    __device__ __forceinline__ double rmax(double v) { return maxv(v); }
};

// the same with the staging buffer of the matrix-core products (LDS, stage_doubles() of mhe_bodies.h, behind the step's own)
struct MheWideMfmaWave : MheWideDevWave {
    double* stage;
};

}  // namespace mhe
}  // namespace mpcqp
