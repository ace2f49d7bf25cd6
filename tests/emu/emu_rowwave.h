// TEST INFRASTRUCTURE ONLY: the emulated row-lane wavefront of the estimator kernels (csrc/mhe_bodies.h, kf_cov_bodies.h,
// kf_dare_bodies.h, mpcqp_small_bodies.h) and its runner: one cooperative fiber per lane of a 64-wide "wavefront"
// (emu_fiber.h), wavefronts one after the other.  GL lanes per estimator: 16 (four estimators per wavefront, the interface of
// csrc/mhe_devwave.h) or 64 (one estimator, csrc/mhe_wide_devwave.h, with the "LDS" of the staged products).  The QP step's
// wave (emu_wave.h) has another interface and is not this one.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <type_traits>
#include <vector>

#include "emu_fiber.h"
#include "mhe_bodies.h"
#include "mhe_dispatch.h"

namespace mpcqp {
namespace mhe {

struct EmuRowShared {
    LaneFibers& bar = lane_fibers();
    double xd[2][WAVE];
    unsigned cn[2][WAVE];                // index of the cross-lane operation every lane is in
    unsigned long calls[WAVE] = {};      // cross-lane operations of every lane (MPCQP_EMU_WATCHDOG)
};

// `stage` exists in the staged wave only: WaveStaged (mhe_bodies.h) detects the member, and a wave that merely carried a
// null pointer would move every NX x NX x NX product onto Ops::mm_staged, which the 16-lane GPU kernels do not run
template <bool STAGED>
struct EmuRowStage {};
template <>
struct EmuRowStage<true> {
    double* stage = nullptr;             // "LDS" of the staged products (plain-loop side of Ops::mm_staged)
};

// A broadcast reads lane C of this lane's group, a reduction runs over the group, a vote over the wavefront.  Every
// cross-lane operation writes buffer (n % 2) of its n-th call, waits once, reads: a lane can only reach call n + 2 (same
// buffer) after all lanes passed the barrier of call n + 1, i.e. after all of them finished reading call n
template <int GLV, bool STAGED>
struct EmuRowWave : EmuRowStage<STAGED> {
    static constexpr int GL = GLV, GPW = WAVE / GLV;      // lanes per estimator, estimators per wavefront (WaveGeom)
    int lane = 0;
    EmuRowShared* sh = nullptr;
    unsigned n = 0;
    void sync() { sh->bar.arrive_and_wait(); }
    double* xchg(double v) {
        sh->cn[n & 1][lane] = n;
        double* buf = sh->xd[n++ & 1];
        buf[lane] = v;
        ++sh->calls[lane];
        sh->bar.arrive_and_wait();
        // every lane must be in the SAME cross-lane operation (a product under a per-estimator condition once was not:
        // mhe_bodies.h write_outputs; a loop exit that is not wave-uniform): a divergent call site aborts here
        // with a message instead of corrupting a fiber stack somewhere later
        for (int i = 0; i < WAVE; ++i)
            if (sh->cn[(n - 1) & 1][i] != n - 1) {
                fprintf(stderr, "[emu] lanes disagree on the sequence of cross-lane operations: lane %d in operation %u, lane %d in %u\n",
                        lane, n - 1, i, sh->cn[(n - 1) & 1][i]);
                fflush(stderr);
                abort();
            }
        return buf;
    }
    template <int C>
    double rowbc(double v) { return xchg(v)[(lane & ~(GL - 1)) + C]; }
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
    double rowred(double v, Op op) {     // over the group, from its first lane upward
        const double* buf = xchg(v);
        const int r0 = lane & ~(GL - 1);
        double s = buf[r0];
        for (int i = 1; i < GL; ++i) s = op(s, buf[r0 + i]);
        return s;
    }
    double rsum(double v) { return rowred(v, [](double x, double y) { return x + y; }); }
    double rmin(double v) { return rowred(v, [](double x, double y) { return fmin(x, y); }); }
    double rmax(double v) { return rowred(v, [](double x, double y) { return fmax(x, y); }); }
    bool any(bool p) {                   // over the whole wavefront (DevWave::any)
        const double* buf = xchg(p ? 1.0 : 0.0);
        for (int i = 0; i < WAVE; ++i) if (buf[i] != 0.0) return true;
        return false;
    }
};

using EmuRow16 = EmuRowWave<RL, false>;
using EmuWide = EmuRowWave<WIDE_RL, true>;
template <int NX>
using EmuRowWaveFor = std::conditional_t<(NX > RL), EmuWide, EmuRow16>;      // the family that serves NX register columns
static_assert(!WaveStaged<EmuRow16>::value && WaveStaged<EmuWide>::value, "only the 64-lane wave runs the staged products");
static_assert(WaveGeom<EmuRow16>::GL == 16 && WaveGeom<EmuRow16>::GPW == 4 && WaveGeom<EmuWide>::GL == 64 && WaveGeom<EmuWide>::GPW == 1);

// body(w, wavefront index, "LDS" of lds_doubles doubles) on nwaves wavefronts, one after the other; a staged wave gets
// stage_doubles() more behind the step's own
template <class W, class F>
void run_row_waves(int nwaves, size_t lds_doubles, F body) {
    constexpr bool staged = WaveStaged<W>::value;
    std::vector<double> smem(lds_doubles + (staged ? stage_doubles() : 0) + 16, 0.0);
    EmuRowShared sh;
    std::atomic<bool> stop{false};
    std::thread dog;
    if (getenv("MPCQP_EMU_WATCHDOG"))      // lanes that stopped agreeing on the number of cross-lane operations
        dog = std::thread([&] {
            unsigned long last = 0;
            while (!stop) {
                std::this_thread::sleep_for(std::chrono::seconds(3));
                unsigned long mn = ~0ul, mx = 0;
                for (int i = 0; i < WAVE; ++i) { mn = std::min(mn, sh.calls[i]); mx = std::max(mx, sh.calls[i]); }
                if (mx == last && mx != mn) {
                    fprintf(stderr, "[emu watchdog] lanes disagree:");
                    for (int i = 0; i < WAVE; ++i) fprintf(stderr, " %lu", sh.calls[i]);
                    fprintf(stderr, "\n");
                }
                if (getenv("MPCQP_EMU_WATCHDOG")[0] == '2') fprintf(stderr, "[emu watchdog] %lu..%lu cross-lane ops\n", mn, mx);
                last = mx;
            }
        });
    int perm[64];
    emu_lane_order(perm);
    sh.bar.run([&](int fiber) {
        W w;
        w.lane = perm[fiber]; w.sh = &sh;
        if constexpr (staged) w.stage = smem.data() + lds_doubles;
        for (int wv = 0; wv < nwaves; ++wv) {
            body(w, wv, smem.data());
            w.sync();
        }
    });
    stop = true;
    if (dog.joinable()) dog.join();
}

// (the launchers pick NX with dispatch_nx of csrc/mhe_dispatch.h, like the device units)

}  // namespace mhe
}  // namespace mpcqp
