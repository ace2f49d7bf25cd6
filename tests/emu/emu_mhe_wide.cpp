// TEST INFRASTRUCTURE ONLY: the wide MovingHorizonEstimator kernels (16 < max(nx̂, nym) <= 32, one estimator per wavefront)
// on the CPU.  Defines the launchers that csrc/mhe_wide_launch.h declares weak, over an emulated 64-lane group: the bodies
// of csrc/mhe_bodies.h with GL = 64, GPW = 1 and the staged products (Ops::mm_staged, plain-loop side).  Linked only into
// libmpcqp_emu_wide.so (tests/test_mhe_wide.py); the stock emulator library has no wide launchers and refuses such handles.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "emu_fiber.h"
#include "mhe_bodies.h"
#include "mhe_wide_launch.h"

namespace mpcqp {
namespace mhe {

namespace {

struct WideShared {
    LaneFibers& bar = lane_fibers();
    double xd[2][WAVE];
    unsigned cn[2][WAVE];                // index of the cross-lane operation every lane is in
};

// one estimator on the 64 lanes: a broadcast reads lane C of the wavefront, a reduction runs over all lanes.  Every
// cross-lane operation writes buffer (n % 2) of its n-th call, waits once, reads (see EmuWave of emu_mhe.cpp).
struct EmuWideWave {
    static constexpr int GL = WIDE_RL, GPW = WIDE_GPW;
    int lane;
    WideShared* sh;
    double* stage;                       // "LDS" of the staged products
    unsigned n = 0;
    void sync() { sh->bar.arrive_and_wait(); }
    double* xchg(double v) {
        sh->cn[n & 1][lane] = n;
        double* buf = sh->xd[n++ & 1];
        buf[lane] = v;
        sh->bar.arrive_and_wait();
        for (int i = 0; i < WAVE; ++i)
            if (sh->cn[(n - 1) & 1][i] != n - 1) {
                fprintf(stderr, "[emu wide] lanes disagree on the sequence of cross-lane operations: lane %d in operation %u, lane %d in %u\n",
                        lane, n - 1, i, sh->cn[(n - 1) & 1][i]);
                fflush(stderr);
                abort();
            }
        return buf;
    }
    template <int C>
    double rowbc(double v) { return xchg(v)[C]; }
    template <class T>
    T* uniform(T* p) const { return p; }
    struct Buf { double* p; size_t bytes; };
    static constexpr unsigned BUF_OOB = 0xFFFFFFF0u;
    Buf make_buf(double* base, size_t bytes) const { return Buf{base, bytes}; }
    double bload(Buf b, unsigned voff, int soff) const {
        const size_t o = (size_t)voff + (size_t)soff;
        return (voff == BUF_OOB || o + 8 > b.bytes) ? 0.0 : *(const double*)((const char*)b.p + o);
    }
    void bstore(Buf b, unsigned voff, int soff, double v) const {
        const size_t o = (size_t)voff + (size_t)soff;
        if (voff != BUF_OOB && o + 8 <= b.bytes) *(double*)((char*)b.p + o) = v;
    }
    template <int L0, int L1, int L2, int L3>
    void fmabc4(double& acc, double x0, double x1, double x2, double x3, double y0, double y1, double y2, double y3) {
        acc = fma(rowbc<L0>(x0), y0, acc); acc = fma(rowbc<L1>(x1), y1, acc);
        acc = fma(rowbc<L2>(x2), y2, acc); acc = fma(rowbc<L3>(x3), y3, acc);
    }
    template <int L0, int L1, int L2, int L3>
    void rank1bc4(double& a0, double& a1, double& a2, double& a3, double x, double y0, double y1, double y2, double y3) {
        const double b0 = rowbc<L0>(x), b1 = rowbc<L1>(x), b2 = rowbc<L2>(x), b3 = rowbc<L3>(x);
        a0 = fma(b0, y0, a0); a1 = fma(b1, y1, a1); a2 = fma(b2, y2, a2); a3 = fma(b3, y3, a3);
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
    template <class Op>
    double red(double v, Op op) {
        const double* buf = xchg(v);
        double s = buf[0];
        for (int i = 1; i < WAVE; ++i) s = op(s, buf[i]);
        return s;
    }
    double rsum(double v) { return red(v, [](double x, double y) { return x + y; }); }
    double rmin(double v) { return red(v, [](double x, double y) { return fmin(x, y); }); }
    double rmax(double v) { return red(v, [](double x, double y) { return fmax(x, y); }); }
    bool any(bool p) {
        const double* buf = xchg(p ? 1.0 : 0.0);
        for (int i = 0; i < WAVE; ++i) if (buf[i] != 0.0) return true;
        return false;
    }
};

template <class F>
void run_wide(int nwaves, size_t lds_doubles, F body) {
    std::vector<double> smem(lds_doubles + stage_doubles() + 16, 0.0);
    WideShared sh;
    int perm[64];
    emu_lane_order(perm);
    sh.bar.run([&](int fiber) {
        EmuWideWave w{perm[fiber], &sh, smem.data() + lds_doubles};
        for (int wv = 0; wv < nwaves; ++wv) {
            body(w, wv, smem.data());
            w.sync();
        }
    });
}

}  // namespace

#define MHE_WIDE_DISPATCH(NXV, CALL)                     \
    switch (NXV) {                                       \
        case 24: { constexpr int NX = 24; CALL; } break; \
        case 32: { constexpr int NX = 32; CALL; } break; \
        default: return hipErrorInvalidValue;            \
    }

hipError_t launch_wide_setup(const Dims& d, const Raw& in, double* cst, hipStream_t) {
    MHE_WIDE_DISPATCH(d.NX, run_wide(d.nwaves, 0, [&](EmuWideWave& w, int wv, double*) { setup_body<EmuWideWave, NX>(w, d, in, cst, wv); }));
    return hipSuccess;
}
hipError_t launch_wide_cov(const Dims& d, const Args& a, int mode, const double* P0, double* Pout, hipStream_t) {
    MHE_WIDE_DISPATCH(d.NX, run_wide(d.nwaves, 0, [&](EmuWideWave& w, int wv, double*) { cov_body<EmuWideWave, NX>(w, d, a, mode, P0, Pout, wv); }));
    return hipSuccess;
}
hipError_t launch_wide_step(const Dims& d, const Args& a, hipStream_t) {
    MHE_WIDE_DISPATCH(d.NX, run_wide(d.nwaves, step_lds_doubles(d.NX), [&](EmuWideWave& w, int wv, double* sm) { step_body<EmuWideWave, NX, 15u>(w, d, a, wv, sm); }));
    return hipSuccess;
}
int wide_waves_for(int, int B, int) { return B < 2 ? B : 2; }      // two "persistent" wavefronts: the grid-stride loop is exercised

}  // namespace mhe
}  // namespace mpcqp
