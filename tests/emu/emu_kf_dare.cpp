// TEST INFRASTRUCTURE ONLY: the steady-state Riccati solve of the SteadyKalmanFilter (csrc/kf_dare_bodies.h) on the CPU.
// Defines the launchers that csrc/kf_dare_launch.h declares weak, over the emulated wavefront of emu_fiber.h, like
// emu_kf_cov.cpp: four estimators per wavefront on 16-lane rows (max(nx̂, nym) <= 16) or one on the 64 lanes with the staged
// products (plain-loop side of Ops::mm_staged).  The wave below is emu_kf_cov.cpp's plus what the doubling loop needs: the
// maximum over an estimator's lanes and the wave-wide vote that ends the loop.  Linked only into libmpcqp_emu_kf_dare.so
// (tests/kf_dare_util.py); the other emulator libraries have no such launcher and answer MPCQP_ERR_UNSUPPORTED to
// mpcqp_kf_set_steady.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "emu_fiber.h"
#include "kf_dare_bodies.h"
#include "kf_dare_launch.h"

namespace mpcqp {
namespace kf {

namespace {

struct Shared {
    LaneFibers& bar = lane_fibers();
    double xd[2][WAVE];
    unsigned cn[2][WAVE];                // index of the cross-lane operation every lane is in
};

// GLV lanes per estimator: a broadcast reads lane C of this lane's group, a reduction runs over the group, a vote over the
// wavefront.  Every cross-lane operation writes buffer (n % 2) of its n-th call, waits once, reads; lanes that disagree on
// the sequence of operations (a loop exit that is not wave-uniform) abort.
template <int GLV>
struct EmuDareWave {
    static constexpr int GL = GLV, GPW = WAVE / GLV;
    int lane;
    Shared* sh;
    unsigned n = 0;
    void sync() { sh->bar.arrive_and_wait(); }
    double* xchg(double v) {
        sh->cn[n & 1][lane] = n;
        double* buf = sh->xd[n++ & 1];
        buf[lane] = v;
        sh->bar.arrive_and_wait();
        for (int i = 0; i < WAVE; ++i)
            if (sh->cn[(n - 1) & 1][i] != n - 1) {
                fprintf(stderr, "[emu kf dare] lanes disagree on the sequence of cross-lane operations: lane %d in operation %u, lane %d in %u\n",
                        lane, n - 1, i, sh->cn[(n - 1) & 1][i]);
                fflush(stderr);
                abort();
            }
        return buf;
    }
    template <int C>
    double rowbc(double v) { return xchg(v)[(lane & ~(GLV - 1)) + C]; }
    template <int L0, int L1, int L2, int L3>
    void fmabc4(double& acc, double x0, double x1, double x2, double x3, double y0, double y1, double y2, double y3) {
        acc = fma(rowbc<L0>(x0), y0, acc); acc = fma(rowbc<L1>(x1), y1, acc);
        acc = fma(rowbc<L2>(x2), y2, acc); acc = fma(rowbc<L3>(x3), y3, acc);
    }
    template <int L0, int L1, int L2, int L3>
    void fmsbc4(double& acc, double x0, double x1, double x2, double x3, double y0, double y1, double y2, double y3) {
        acc = fma(rowbc<L0>(x0), -y0, acc); acc = fma(rowbc<L1>(x1), -y1, acc);
        acc = fma(rowbc<L2>(x2), -y2, acc); acc = fma(rowbc<L3>(x3), -y3, acc);
    }
    template <int K>
    void gjacc4(double& a0, double& a1, double& a2, double& a3, double g) {
        const double b0 = rowbc<K>(a0), b1 = rowbc<K>(a1), b2 = rowbc<K>(a2), b3 = rowbc<K>(a3);
        a0 = fma(b0, g, a0); a1 = fma(b1, g, a1); a2 = fma(b2, g, a2); a3 = fma(b3, g, a3);
    }
    double rmin(double v) {
        const double* buf = xchg(v);
        const int r0 = lane & ~(GLV - 1);
        double s = buf[r0];
        for (int i = 1; i < GLV; ++i) s = fmin(s, buf[r0 + i]);
        return s;
    }
    double rmax(double v) {
        const double* buf = xchg(v);
        const int r0 = lane & ~(GLV - 1);
        double s = buf[r0];
        for (int i = 1; i < GLV; ++i) s = fmax(s, buf[r0 + i]);
        return s;
    }
    bool any(bool p) {                   // over the whole wavefront (DevWave::any)
        const double* buf = xchg(p ? 1.0 : 0.0);
        bool s = false;
        for (int i = 0; i < WAVE; ++i) s = s || buf[i] != 0.0;
        return s;
    }
};

struct EmuDareRowWave : EmuDareWave<mhe::RL> {};
struct EmuDareWideWave : EmuDareWave<mhe::WIDE_RL> {
    double* stage = nullptr;
};

template <class W, int NX>
void run_dare(const DareArgs& a) {
    std::vector<double> smem(mhe::stage_doubles() + 16, 0.0);
    Shared sh;
    int perm[64];
    emu_lane_order(perm);
    sh.bar.run([&](int fiber) {
        W w{};
        w.lane = perm[fiber]; w.sh = &sh;
        if constexpr (mhe::WaveStaged<W>::value) w.stage = smem.data();
        for (int wv = 0; wv < a.nwaves; ++wv) {
            kf_dare_body<W, NX>(w, a, wv);
            w.sync();
        }
    });
}

}  // namespace

hipError_t launch_kf_dare(const DareArgs& a, hipStream_t) {
    if (a.B < 1 || a.nwaves < 1 || a.nx < 1 || a.nym < 1 || a.nx > a.NX || a.nym > a.NX) return hipErrorInvalidValue;
    switch (a.NX) {
        case 4: run_dare<EmuDareRowWave, 4>(a); break;
        case 8: run_dare<EmuDareRowWave, 8>(a); break;
        case 12: run_dare<EmuDareRowWave, 12>(a); break;
        case 16: run_dare<EmuDareRowWave, 16>(a); break;
        case 24: run_dare<EmuDareWideWave, 24>(a); break;
        case 32: run_dare<EmuDareWideWave, 32>(a); break;
        default: return hipErrorInvalidValue;
    }
    return hipSuccess;
}
// two "persistent" wavefronts: the grid-stride loop is exercised
int kf_dare_waves_for(int, int B, int NX) {
    const int groups = NX > mhe::RL ? B : (B + mhe::GPW - 1) / mhe::GPW;
    return groups < 2 ? groups : 2;
}

}  // namespace kf
}  // namespace mpcqp
