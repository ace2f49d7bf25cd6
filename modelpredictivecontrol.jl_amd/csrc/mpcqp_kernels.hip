// mpcqp_kernels.hip -- gfx950 kernels of the batched LinMPC step: one QP per 64-lane wavefront,
// one wavefront per workgroup, the condensed problem (step-response table, packed normal-equation
// tile, residual/row state) staged in LDS.  Bodies: mpcqp_bodies.h.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <string>

#include "mpcqp_bodies.h"
#include "mpcqp_devwave.h"
#include "mpcqp_dispatch.h"
#include "mpcqp_launch.h"

namespace mpcqp {

#ifndef MPCQP_K1_MFMA_MIN_NX
#define MPCQP_K1_MFMA_MIN_NX 10   // below, the 16-wide tiles are mostly padding and the LDS loops are faster (C2, nx̂ = 6: 0.55 vs 0.66 ms)
#endif
bool predmat_on_mfma(const Dims& d) {
    static const int min_nx = [] {          // (MPCQP_K1_MFMA_MIN_NX=1 in the environment: every eligible shape, for the tests)
        const char* e = getenv("MPCQP_K1_MFMA_MIN_NX");
        return e && atoi(e) > 0 ? atoi(e) : MPCQP_K1_MFMA_MIN_NX;
    }();
    return predmat_mfma_ok(d) && d.nxh >= min_nx;
}
__global__ __launch_bounds__(64) void k_predmat(Dims d, Model m, int terminal) {
    DevWave w{(int)threadIdx.x};
    predmat_body(w, d, m, (int)blockIdx.x, mpcqp_smem, terminal != 0);
}
// the same tables from chains of v_mfma_f64_16x16x4 (predmat_mfma: no LDS, the state stays in the accumulators)
__global__ __launch_bounds__(64) void k_predmat_mfma(Dims d, Model m, int terminal) {
    predmat_mfma((int)threadIdx.x, d, m, (int)blockIdx.x, terminal != 0);
}

__global__ __launch_bounds__(64) void k_hessian(Dims d, Model m) {
    DevWave w{(int)threadIdx.x};
    hessian_body(w, d, m, (int)blockIdx.x, mpcqp_smem);
}

__global__ __launch_bounds__(64) void k_step(Dims d, Model m, StepIO io) {
    DevWave w{(int)threadIdx.x};
    step_body(w, d, m, io, (int)blockIdx.x, mpcqp_smem);
}

// per-handle step constants (Model::stepc): one thread per (controller, block, channel); runs once per change of the
// bounds / weights, so the strided reads along the horizon do not matter
__global__ __launch_bounds__(256) void k_step_consts(Dims d, Model m, double* out) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < (long long)d.B * d.nDU) step_consts_entry(d, m, (int)(g / d.nDU), (int)(g % d.nDU), out);
}

// SteadyKalmanFilter steps: npad = next power of two >= nx̂ lanes per problem, 256-thread blocks
__global__ __launch_bounds__(256) void k_kf_correct(Dims d, Model m, KfParams kf, double* xhat0,
                                                    const double* y0m, const double* d0, int npad) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    kf_correct_lane(d, m, kf, g / npad, g % npad, xhat0, xhat0, y0m, d0);
}

__global__ __launch_bounds__(256) void k_kf_predict(Dims d, Model m, double* xhat0, const double* u0,
                                                    const double* d0, int npad) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    kf_predict_lane(d, m, g / npad, g % npad, xhat0, xhat0, u0, d0);
}

// ---- launchers (host) ------------------------------------------------------------------------
hipError_t launch_predmat(const Dims& d, const Model& m, bool terminal, hipStream_t st) {
    if (predmat_on_mfma(d)) {
        hipLaunchKernelGGL(k_predmat_mfma, dim3(d.B), dim3(WAVE), 0, st, d, m, terminal ? 1 : 0);
        return hipGetLastError();
    }
    size_t lds = (size_t)predmat_lds_doubles(d) * sizeof(double);
    hipError_t e = ensure_lds((const void*)k_predmat, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_predmat, dim3(d.B), dim3(WAVE), lds, st, d, m, terminal ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_step_consts(const Dims& d, const Model& m, double* out, hipStream_t st) {
    const long long total = (long long)d.B * d.nDU;
    hipLaunchKernelGGL(k_step_consts, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d, m, out);
    return hipGetLastError();
}

// ---- which kernel runs a step -----------------------------------------------------------------
template <class F> static bool first_aot(F&& f) {      // (this library's one visit of the ahead-of-time list: mpcqp_dispatch.h)
    MPCQP_SPECIALIZATIONS(MPCQP_AOT_TRY)
    return false;
}
static bool aot_matches(const Dims& d) { return first_aot([&](auto e) { return decltype(e)::type::matches(d); }); }

// The kernel of a step: 0 the runtime-dimension kernel, 1 an ahead-of-time specialisation, 2 an on-demand one (`spec`: its
// entry points; loaded from the cache, csrc/spec_cache.cpp), 3 the small-problem kernel.  What step_kernel_kind() reports and
// what launch_step() launches both come from choose_step().
struct StepChoice { int kind; SpecEntry spec; };

// The one-QP-per-wavefront kernels: they run the steps the small-problem kernel does not take (Ŷ requested, fused Kalman
// steps).  `verified` = false (mpcqp_prepare): an on-demand object counts as soon as it is loaded, before its comparison.
static StepChoice choose_step_other(const Dims& d, bool verified = true) {
    if (force_generic()) return {0, {}};
    if (!d.dense_w && aot_matches(d)) return {1, {}};     // (the kernels compiled into the library have no dense-weight products)
    const SpecEntry e = verified ? spec_find_verified(d) : spec_find(d);
    return {e.step ? 2 : 0, e};
}

// The small-problem kernel takes the step -- unless it is its dense-row variant on a grid of the latency regime (at most one
// controller per SIMD as one-per-wavefront grid: B <= 1024) and the handle's own specialisation is there: measured on C2
// dimensions with a soft ymax (40 dense rows; scripts/small_vs_wave.py 4,2,2,20,5), one controller per wavefront with the
// matrix-core assembly and the polish is 1.5 times faster at B <= 1024 (0.25 against 0.38 ms), the two tie from 4096 on.
// MPCQP_SMALL_Y=1 keeps the dense-row variant whatever the batch (tests of that kernel).
static StepChoice choose_step(const Dims& d, const Model& m, const StepIO& io) {
    if (force_generic() || !small_eligible(d, m, io)) return choose_step_other(d);
    const char* e = getenv("MPCQP_SMALL_Y");           // (read at every call: tests switch it inside one process)
    const bool keep_y = e && e[0] == '1';
    if (small_has_y(d) && !keep_y && d.B <= 1024) {
        const StepChoice other = choose_step_other(d);
        if (other.kind != 0) return other;
    }
    return {3, {}};
}

int step_kernel_kind(const Dims& d, const Model& m) { return choose_step(d, m, StepIO{}).kind; }
int step_kernel_kind_other(const Dims& d) { return choose_step_other(d).kind; }

// Make the specialised kernel of `d` available (compile if needed, load).  Returns the kernel kind
// as step_kernel_kind_other(); `err` receives the reason when an eligible specialisation could not be built.
static int prepare_step_other(const Dims& d, std::string* err) {
    spec_forget_miss(d);                                 // a remembered miss is looked up again by a prepare
    const int kind = choose_step_other(d, false).kind;
    if (kind != 0 || force_generic() || !spec_enabled(d)) return kind;
    if (spec_build(d, nullptr, err) != 0) return 0;
    spec_forget_miss(d);                                 // forget a remembered failure of an earlier load
    if (spec_find(d).step) return 2;
    if (err) *err = "the specialisation was built but could not be loaded";
    return 0;
}

int prepare_step(const Dims& d, const Model& m, std::string* err) {
    // (the kernel behind the small one is prepared as well: steps that ask for Ŷ or fuse the Kalman steps run on it)
    const int other = prepare_step_other(d, err);
    return choose_step(d, m, StepIO{}).kind == 3 ? 3 : other;
}

// compile only (no device, no load -- so not choose_step_other(), which loads): for build pipelines
int prebuild_step(const Dims& d, std::string* err) {
    if (aot_matches(d)) return 1;
    if (!spec_enabled(d)) return 0;
    return spec_build(d, nullptr, err) == 0 ? 2 : -1;
}

// the runtime-dimension kernel
hipError_t launch_step_generic(const Dims& d, const Model& m, const StepIO& io, hipStream_t st) {
    size_t lds = (size_t)make_carve(d).total * sizeof(double);
    hipError_t e = ensure_lds((const void*)k_step, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_step, dim3(d.B), dim3(WAVE), lds, st, d, m, io);
    return hipGetLastError();
}

hipError_t launch_hessian(const Dims& d, const Model& m, hipStream_t st) {
    // (a block-diagonal M_Hp takes the scalar contraction of the runtime-dims kernel: set-up path)
    hipError_t err = hipSuccess;
    if (!force_generic() && !m.Mblk && !m.Mfull && !m.Ndense && !m.Ldense && first_aot([&](auto e) {
            using SD = typename decltype(e)::type;
            return SD::matches_dims(d) && ((err = launch_hessian_static<SD>(d, m, st)), true);
        }))
        return err;
    // (the Hessian of other dimensions stays on the generic kernel: it runs once per set_model)
    size_t lds = (size_t)make_carve(d).total * sizeof(double);
    hipError_t e = ensure_lds((const void*)k_hessian, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_hessian, dim3(d.B), dim3(WAVE), lds, st, d, m);
    return hipGetLastError();
}

static hipError_t launch_chosen(const StepChoice& c, const Dims& d, const Model& m, const StepIO& io, hipStream_t st) {
    if (c.kind == 3) return launch_step_small(d, m, io, st);
    if (c.kind == 2) return (hipError_t)c.spec.step(&d, &m, &io, (void*)st);
    hipError_t err = hipSuccess;
    if (c.kind == 1 && first_aot([&](auto e) {
            using SD = typename decltype(e)::type;
            return SD::matches(d) && ((err = launch_step_static<SD>(d, m, io, st)), true);
        }))
        return err;
    return launch_step_generic(d, m, io, st);
}

hipError_t launch_step(const Dims& d, const Model& m, const StepIO& io, hipStream_t st) { return launch_chosen(choose_step(d, m, io), d, m, io, st); }
// the one-QP-per-wavefront kernels: ahead-of-time specialisation, on-demand specialisation, runtime dimensions
hipError_t launch_step_spec_or_aot(const Dims& d, const Model& m, const StepIO& io, hipStream_t st) { return launch_chosen(choose_step_other(d), d, m, io, st); }

// the on-demand specialisation itself, verified or not: only mpcqp_prepare's comparison calls this
hipError_t launch_step_unverified_spec(const Dims& d, const Model& m, const StepIO& io, hipStream_t st) {
    const SpecEntry e = spec_find(d);
    return e.step ? (hipError_t)e.step(&d, &m, &io, (void*)st) : launch_step_spec_or_aot(d, m, io, st);
}

static int kf_npad(const Dims& d) {
    int n = 1;
    while (n < d.nxh) n <<= 1;
    return n;
}

hipError_t launch_kf_correct(const Dims& d, const Model& m, const KfParams& kf, double* xhat0,
                             const double* y0m, const double* d0, hipStream_t st) {
    const int npad = kf_npad(d);
    const long long total = (long long)d.B * npad;
    hipLaunchKernelGGL(k_kf_correct, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d, m, kf,
                       xhat0, y0m, d0, npad);
    return hipGetLastError();
}

hipError_t launch_kf_predict(const Dims& d, const Model& m, double* xhat0, const double* u0,
                             const double* d0, hipStream_t st) {
    const int npad = kf_npad(d);
    const long long total = (long long)d.B * npad;
    hipLaunchKernelGGL(k_kf_predict, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d, m,
                       xhat0, u0, d0, npad);
    return hipGetLastError();
}

size_t step_lds_bytes(const Dims& d) { return (size_t)make_carve(d).total * sizeof(double); }

}  // namespace mpcqp
