// mpcqp_host.hip -- C-ABI of include/mpcqp.h: handle, device residency, launches.
// There is deliberately NO CPU fallback in this library: every compute entry point needs a HIP
// device and fails with MPCQP_ERR_DEVICE otherwise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mpcqp_mhe.h"
#include "c2d_launch.h"
#include "est_init_launch.h"
#include "explicit_launch.h"
#include "im_launch.h"
#include "kf_cov_launch.h"
#include "kf_dare_launch.h"
#include "kf_dare_lds_launch.h"
#include "kf_place_launch.h"
#include "mpcqp_hostutil.h"
#include "mpcqp_launch.h"
#include "ms_bodies.h"
#include "ms_launch.h"
#include "sim_launch.h"

using namespace mpcqp;

thread_local std::string g_hip_err;

struct DBuf {                      // owned device array of doubles (or ints)
    void* p = nullptr;
    size_t bytes = 0;
};

// Which estimator sits behind a handle: exactly one of these at a time (mpcqp_handle_s::est; the setters switch with
// adopt_estimator).  The four Kalman kinds are contiguous: est_is_kf.
enum {
    EST_NONE = 0,
    EST_KF_GAIN,        // mpcqp_kf_set: a gain of the caller's
    EST_KF_TV,          // mpcqp_kf_set_covariances: the covariance kernel writes K̂(k) ahead of every estimator step
    EST_KF_STEADY,      // mpcqp_kf_set_steady: the gain the Riccati kernel solved for
    EST_KF_PLACE,       // mpcqp_kf_set_poles: the gain the placement kernel found
    EST_MHE,            // mpcqp_mhe_attach: a MovingHorizonEstimator handle (mpcqp_handle_s::mhe)
    EST_IM              // mpcqp_im_set: the InternalModel
};

struct mpcqp_handle_s {
    Dims d{};
    Model m{};
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_s0 = nullptr, ev_s1 = nullptr, ev_c0 = nullptr, ev_c1 = nullptr, ev_cm = nullptr;
    bool step_timed = false, cond_timed = false;
    bool have_model = false, have_weights = false, terminal_built = false;
    // Model::Hpk holds K2's result for the CURRENT tables and weights.  Cleared whenever an input of K2 changes or its
    // launch is skipped (the problem did not fit the LDS at that moment: condensed_fits depends on the row groups, which
    // set_bounds / set_custom_bounds may shrink later); ensure_hessian() launches K2 lazily wherever H~ is about to be read.
    bool hessian_valid = false;
    // Model::stepc holds the step constants of the CURRENT bounds and weights (k_step_consts).  Every setter that writes one of
    // their inputs drops the block (invalidate_stepc); ensure_stepc() builds it lazily on the stream of the next step.
    bool stepc_valid = false;
    DBuf stepc;
    int stepc_builds = 0;      // launches of k_step_consts so far (mpcqp_step_consts_builds)
    std::vector<int> nb, jl, blk;
    std::vector<void*> owned;
    // model / weights / bounds storage
    DBuf Ahat, Bu, C, Bd, Dd, dop, Mdiag, Ndiag, Ldiag, Cwt, Mblk, Mfull, Ndense, Ldense;
    DBuf Wy, Wu, Wd, Wr, w_op, Wmin, Wmax, C_wmin, C_wmax, ry_now;
    DBuf bnd[16];
    // staging for the host-pointer step
    DBuf s_x, s_lu, s_ry, s_ru, s_d0, s_dh, s_Z, s_u0, s_st, s_it, s_yh;
    DBuf keep_q, keep_F, prof, lam, audit;
    bool lam_valid = false;     // lam holds the multipliers of the previous step (MPCQP_FLAG_WARM_DUAL)
    bool lam_stage = false;     // ... in the row order of the stage-structured kernel (else of the condensed kernels)
    int lam_rows = 0;           // ... that many per controller
    // mpcqp_set_dense_weights: the matrix is stage-separable, every entry outside its diagonal blocks (M_Hp: ny x ny per
    // step, N_Hc: nu x nu per free move, L_Hp: nu x nu per step) is exactly 0.0 in every member.  The stage-structured kernel
    // takes such weights (ms_bodies.h); the condensed kernels go on reading Mfull / Ndense / Ldense.
    bool sepM = false, sepN = false, sepL = false;
    DBuf ms_Mblk;               // [B][Hp][ny][ny] the blocks of a stage-separable Mfull, for the stage kernel (Model::Mblk there)
    // the estimator behind the handle (EST_*); kf.i_ym / kf.nym hold the measured rows of every kind, kf.Khat the gain of
    // the Kalman kinds
    int est = EST_NONE;
    // SteadyKalmanFilter
    DBuf kf_K, kf_iym, kf_x, kf_y, kf_u, kf_d;
    KfParams kf{};
    // time-varying KalmanFilter (EST_KF_TV): kf_K then holds K̂(k), written by the covariance kernel
    // (kf_kernels.hip) ahead of every estimator step that reads it
    DBuf kf_Q, kf_R, kf_P, kf_st;
    int kf_NX = 0, kf_waves = 0;   // register columns and persistent grid of the covariance kernel
    // SteadyKalmanFilter from Q̂ and R̂ (EST_KF_STEADY): kf_K holds the gain the Riccati kernel (kf_dare_bodies.h) solved
    // for, kf_P its P̂∞, kf_st / kf_it the status and iteration count of the last solve
    DBuf kf_it;
    DBuf kf_path;     // which body produced each estimator's result (kf_dare_launch.h: DareArgs::path)
    int kf_dare_waves = 0;
    // 32 < max(nx̂, nym) <= 64: the solve runs on the LDS-resident kernels (kf_dare_lds_bodies.h), kf_NX is their padded
    // order, kf_dare_waves their workgroups, kf_dare_team the wavefronts per estimator of the last solve
    bool kf_dare_lds = false;
    int kf_dare_team = 0;
    // Luenberger observer from its poles (EST_KF_PLACE): kf_K holds the gain the placement kernel (kf_place_bodies.h)
    // found, kf_st / kf_it its status and sweep count
    DBuf kf_poles;
    int kf_place_cap = kf::PLACE_CAP_DEFAULT;
    // mpcqp_kf_set_direct: 1 filter form (mpcqp_loop_device: correction, step, prediction), 0 predictor form (step, correction,
    // prediction).  A property of the handle: the setters of the gain and of the covariances leave it alone
    int kf_direct = 1;
    // MultipleShooting transcription (mpcqp_set_transcription): the stage-structured kernel of ms_bodies.h
    int transcription = MPCQP_SINGLE_SHOOTING;
    bool stage_only = false;         // nZ~ > 256: only the stage-structured kernel can take this handle (nothing is condensed)
    bool stage_rows = false;         // C_umin / C_umax vary inside a move-blocking interval: the U rows cannot be merged, the
                                     // stage-structured kernel (one U row per step) takes the handle
    bool dual_reg_given = false;     // mpcqp_dims.dual_reg > 0 (else each kernel's own default)
    DBuf ms_X, ms_defect, ms_scratch, ms_next;
    // ExplicitMPC (mpcqp_explicit_prepare): ex_Hinv / ex_st are what k_explicit_factor left for the CURRENT H~ -- every
    // setter that changes H~ runs explicit_refresh on a prepared handle -- and ex_law_z / ex_law_u the law tables (ex_law).
    // ex_stale: H~ changed while the handle had finite rows (the explicit calls answer MPCQP_ERR_ORDER then, the setters do
    // not factor); the first explicit call after the rows are gone factors again (explicit_current)
    bool ex_prepared = false, ex_law = false, ex_stale = false;
    DBuf ex_Hinv, ex_Lsum, ex_st, ex_law_z, ex_law_u;
    DBuf ex_bx, ex_blu, ex_bry, ex_bd0, ex_bdh, ex_bZ0, ex_bZk, ex_bu0, ex_bst;     // device buffers of the law build
    int ex_waves_z = 0, ex_waves_u = 0;
    // the plant of the closed-loop simulation (mpcqp_sim_set_plant) and the per-period buffers of mpcqp_sim_device: what the
    // controller leaves (u0, status, iterations) and what k_sim_plant hands the estimator and the controller (d0, y0m, the set
    // point of the period, repeat(d0, Hp)); sim_s: staging of the host-pointer call, in the order of mpcqp_sim_io
    bool have_plant = false;
    int sim_nxp = 0;
    DBuf sp_A, sp_Bu, sp_C, sp_Bd, sp_Dd, sp_fx;
    bool sp_has_Bd = false, sp_has_Dd = false, sp_has_fx = false;
    DBuf sim_u0, sim_st, sim_it, sim_d0, sim_y0m, sim_ry, sim_dh;
    DBuf sim_s[26];
    // LinMPC(MovingHorizonEstimator): the estimator behind this controller (mpcqp_mhe_attach; borrowed), NULL unless est is
    // EST_MHE.  sim_est: its status array after every period of the last mpcqp_sim[_device], [N][B]; ei_*: staging of the
    // host-pointer mpcqp_est_initstate
    mpcqp_mhe mhe = nullptr;
    DBuf sim_est;
    int sim_est_N = 0;
    DBuf ei_x, ei_u, ei_y, ei_d, ei_st;
    // InternalModel (mpcqp_im_set): the stochastic model as given (im_As .. im_Ds), Âs and B̂s of the set-up, x̂s, ŷs, Ŷs, the
    // B + Ŷs every step of the handle reads in place of Model::Bvec, z = Âs x̂s + B̂s ŷs of the last correction (next period's
    // x̂s) and the set-up's status (EST_IM).
    bool in_multi = false;      // a shard of mpcqp_multi_create
    int im_nxs = 0;
    DBuf im_As, im_Bs, im_Cs, im_Ds, im_Ahs, im_Bhs, im_xs, im_ys, im_Yhs, im_Beff, im_z, im_st;
    // mpcqp_set_model_continuous: staging of the host-pointer call (A, Bu, C, Bd, Dd, Ts, dop) and the status of the kernel
    DBuf c2d_s[7], c2d_st;
};

static int dev_alloc(mpcqp_handle h, DBuf& b, size_t bytes) {
    if (b.p && b.bytes >= bytes) return MPCQP_OK;
    void* p = nullptr;
    if (bytes == 0) bytes = 8;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {
        g_hip_err = std::string("hipMalloc: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? MPCQP_ERR_NOMEM : MPCQP_ERR_DEVICE;
    }
    h->owned.push_back(p);
    b.p = p;
    b.bytes = bytes;
    return MPCQP_OK;
}

// give a scratch array back before the handle goes (temporaries of mpcqp_prepare's self-test)
static void dev_release(mpcqp_handle h, DBuf& b) {
    if (!b.p) return;
    for (size_t i = 0; i < h->owned.size(); ++i)
        if (h->owned[i] == b.p) { h->owned.erase(h->owned.begin() + (long)i); break; }
    (void)hipFree(b.p);
    b = DBuf{};
}

// A step enqueued on a caller's stream (mpcqp_step_device) may still read the handle's device
// arrays: every upload into them is ordered behind the end of that step (event ev_s1).
static int upload(mpcqp_handle h, DBuf& b, const void* src, size_t bytes) {
    int rc = dev_alloc(h, b, bytes);
    if (rc) return rc;
    if (h->step_timed) HIPCHK(hipStreamWaitEvent(h->stream, h->ev_s1, 0));
    HIPCHK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, h->stream));
    return MPCQP_OK;
}

static bool est_is_kf(mpcqp_handle h) { return h->est >= EST_KF_GAIN && h->est <= EST_KF_PLACE; }     // a gain in kf.Khat
static bool est_has_cov(mpcqp_handle h) { return h->est == EST_KF_TV || h->est == EST_KF_STEADY; }     // a P̂ in kf_P
static bool est_any(mpcqp_handle h) { return h->est != EST_NONE; }

// The one place where a handle changes its estimator: the measured rows are those just uploaded into kf_iym, `Khat` the
// gain of a Kalman kind (NULL otherwise), and whatever was there before -- an attachment included -- is gone.
static void adopt_estimator(mpcqp_handle h, int kind, const double* Khat, int32_t nym) {
    h->kf.Khat = Khat;
    h->kf.i_ym = (const int*)h->kf_iym.p;
    h->kf.nym = nym;
    h->est = kind;
    h->mhe = nullptr;
}

// validate_ym, construct.jl:190-196: every measured row inside 0 .. ny-1 and named once (the bounds of nym are the caller's)
static int check_iym(const Dims& d, const int32_t* i_ym, int32_t nym) {
    for (int i = 0; i < nym; ++i) {
        if (i_ym[i] < 0 || i_ym[i] >= d.ny) return MPCQP_ERR_ARG;
        for (int j = 0; j < i; ++j)
            if (i_ym[j] == i_ym[i]) return MPCQP_ERR_ARG;
    }
    return MPCQP_OK;
}

// `count` int32 of a status-like array for the host, after everything that may still write it: the handle's stream, and
// the device, because the producer may have been enqueued on a stream of the caller's
static int read_back_i32(mpcqp_handle h, const DBuf& b, size_t count, int32_t* out) {
    ON_DEVICE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, b.p, count * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MPCQP_OK;
}

// The host-pointer twin of a _device entry point: inputs go up into staging buffers of the handle, outputs are allocated
// there, the device entry runs on the handle's stream, the results come down, finish() waits.  The first error sticks:
// every later member does nothing, so a twin looks at `rc` once after its uploads and once at its end.
struct Staging {
    mpcqp_handle h;
    int rc = MPCQP_OK;
    template <class T>
    T* in(DBuf& b, const T* host, size_t count) {           // the device copy of `host`; NULL stays NULL
        if (!host || rc) return nullptr;
        rc = upload(h, b, host, count * sizeof(T));
        return (T*)b.p;
    }
    template <class T>
    T* out(DBuf& b, size_t count) {
        if (rc) return nullptr;
        rc = dev_alloc(h, b, count * sizeof(T));
        return (T*)b.p;
    }
    void down(void* host, const DBuf& b, size_t bytes) {    // (an output the caller did not ask for: nothing)
        if (!host || rc) return;
        const hipError_t e = hipMemcpyAsync(host, b.p, bytes, hipMemcpyDeviceToHost, h->stream);
        if (e != hipSuccess) {
            g_hip_err = std::string("hipMemcpyAsync to the host: ") + hipGetErrorString(e);
            rc = MPCQP_ERR_DEVICE;
        }
    }
    int finish() {
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));
        return MPCQP_OK;
    }
};

// slice of a problem-major array with `per` values per problem (NULL stays NULL)
template <class T>
static T* shard_of(T* a, int off, size_t per) { return a ? a + (size_t)off * per : nullptr; }

struct mpcqp_multi_s {
    std::vector<mpcqp_handle> h;
    std::vector<int> off, cnt;
    Dims d{};                       // whole-batch dimensions (B = total)
};

extern "C" {

#ifndef HIP_VERSION_MAJOR      // (the CPU wave emulator's stand-in runtime, tests/emu/fakehip)
#define HIP_VERSION_MAJOR 0
#define HIP_VERSION_MINOR 0
#endif
#define MPCQP_STR2(x) #x
#define MPCQP_STR(x) MPCQP_STR2(x)
// (the HIP version of the BUILD: the loader of api.py compares it with the runtime the process ends up with)
const char* mpcqp_version(void) { return "mpcqp 0.1.0 (gfx950, HIP " MPCQP_STR(HIP_VERSION_MAJOR) "." MPCQP_STR(HIP_VERSION_MINOR) ")"; }

const char* mpcqp_strerror(int code) {
    switch (code) {
        case MPCQP_OK: return "ok";
        case MPCQP_ERR_NULL: return "required pointer is NULL";
        case MPCQP_ERR_DIMS: return "dimension mismatch";
        case MPCQP_ERR_ARG: return "illegal argument value";
        case MPCQP_ERR_UNSUPPORTED: return "configuration not supported by this build";
        case MPCQP_ERR_ORDER: return "model, weights must be set before step";
        case MPCQP_ERR_DEVICE: return "HIP runtime error (see mpcqp_last_hip_error)";
        case MPCQP_ERR_NOMEM: return "out of device memory";
        default: return "unknown error code";
    }
}

const char* mpcqp_last_hip_error(void) { return g_hip_err.c_str(); }

static void layout_rows(mpcqp_handle h) {
    Dims& d = h->d;
    d.cnt_[P_BOX] = d.nZ; d.cnt_[P_U] = d.nDU; d.cnt_[P_DU] = d.nDU; d.cnt_[P_X] = d.nxh;
    d.cnt_[P_Y] = d.nY + (d.eps_host() >= 0 ? 1 : 0);         // + the row -eps <= 0 when a Ŷ group hosts it (mpcqp_types.h)
    d.cnt_[P_W] = d.nW;
    int o = 0;
    for (int g = 0; g < NGROUP; ++g) {
        d.rowoff_[g] = o;
        if ((d.gmask >> g) & 1u) o += d.cnt_[g >> 1];
    }
    d.rowoff_[NGROUP] = o;
    h->lam_valid = false;       // the row layout changed: stored multipliers no longer line up
}

int mpcqp_create(const mpcqp_dims* in, mpcqp_handle* out) {
    if (!in || !out) return MPCQP_ERR_NULL;
    *out = nullptr;
    if (in->batch < 1 || in->nxhat < 1 || in->nu < 1 || in->ny < 1 || in->nd < 0) return MPCQP_ERR_ARG;
    // validate_weights, src/controller/construct.jl:99-103
    if (in->Hp < 1 || in->Hc < 1 || in->Hc > in->Hp) return MPCQP_ERR_ARG;
    if (in->neps != 0 && in->neps != 1) return MPCQP_ERR_ARG;
    std::vector<int> nb(in->Hc, 1);
    if (in->nb) {
        int sum = 0;
        for (int i = 0; i < in->Hc; ++i) {
            if (in->nb[i] < 1) return MPCQP_ERR_ARG;   // move_blocking, construct.jl:632
            nb[i] = in->nb[i];
            sum += nb[i];
        }
        if (sum != in->Hp) return MPCQP_ERR_DIMS;
    } else {
        nb[in->Hc - 1] = in->Hp - in->Hc + 1;          // construct.jl:653-660
    }
    const int nZ = in->nu * in->Hc + in->neps;
    // nZ~ <= 64: one Cholesky row per lane (specialised kernels); above that the runtime-dims kernel
    // gives every lane several rows, as long as the problem fits the 160 KB of LDS (checked in layout_rows)
    // Beyond nZ~ = 256 (the reference has no size limit: transcription.jl:2-4) there is no condensed kernel -- the Newton
    // matrix alone would not fit the LDS.  Such handles run the SAME QP on the stage-structured kernel of ms_bodies.h
    // (cost linear in the horizon, no nZ~ limit), whatever their transcription: `stage_only`.  Nothing is condensed for
    // them (no K1 / K2 tables, no packed H~).
    const bool stage_only = nZ > 4 * WAVE;
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (in->device < 0 || in->device >= ndev) return MPCQP_ERR_ARG;
    DeviceGuard guard_(in->device);
    if (!guard_.ok) { g_hip_err = "hipSetDevice failed"; return MPCQP_ERR_DEVICE; }
    mpcqp_handle h = new (std::nothrow) mpcqp_handle_s();
    if (!h) return MPCQP_ERR_NOMEM;
    Dims& d = h->d;
    d.B = in->batch; d.nxh = in->nxhat; d.nu = in->nu; d.ny = in->ny; d.nd = in->nd;
    d.Hp = in->Hp; d.Hc = in->Hc; d.neps = in->neps;
    d.nZ = nZ; d.nDU = in->nu * in->Hc; d.nU = in->nu * in->Hp; d.nY = in->ny * in->Hp;
    d.nD = in->nd * in->Hp;
    d.nw = 0; d.nW = 0;
    d.npk = pk_size(nZ);
    d.flags = in->flags;
    d.max_iter = in->max_iter > 0 ? in->max_iter : 80;
    d.gap_tol = in->gap_tol > 0 ? in->gap_tol : 1e-12;
    d.res_tol = in->res_tol > 0 ? in->res_tol : 1e-11;
    d.dual_reg = in->dual_reg > 0 ? in->dual_reg : 1e-12;
    h->dual_reg_given = in->dual_reg > 0;
    h->stage_only = stage_only;
    d.gmask = d.neps ? 1u : 0u;                        // ϵ >= 0 is always there
    layout_rows(h);
    h->device = in->device;
    h->nb = nb;
    d.default_nb = 1;
    for (int i = 0; i < d.Hc; ++i)
        if (nb[i] != (i == d.Hc - 1 ? d.Hp - d.Hc + 1 : 1)) d.default_nb = 0;
    h->jl.assign(d.Hc + 1, 0);
    for (int i = 0; i < d.Hc; ++i) h->jl[i + 1] = h->jl[i] + nb[i];
    h->blk.assign(d.Hp, 0);
    for (int i = 0; i < d.Hc; ++i)
        for (int t = h->jl[i]; t < h->jl[i + 1]; ++t) h->blk[t] = i;
    int rc = MPCQP_OK;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&h->ev_s0);
    if (e == hipSuccess) e = hipEventCreate(&h->ev_s1);
    if (e == hipSuccess) e = hipEventCreate(&h->ev_c0);
    if (e == hipSuccess) e = hipEventCreate(&h->ev_c1);
    if (e == hipSuccess) e = hipEventCreate(&h->ev_cm);
    if (e != hipSuccess) {
        g_hip_err = std::string("stream/event create: ") + hipGetErrorString(e);
        rc = MPCQP_ERR_DEVICE;
    }
    auto mk = [&](size_t n) -> double* {
        if (rc) return nullptr;
        DBuf b;
        rc = dev_alloc(h, b, n * sizeof(double));
        return (double*)b.p;
    };
    const size_t B = d.B;
    if (!stage_only) {
        h->m.Stab = mk(B * d.Hp * d.ny * d.nu);
        h->m.Ktab = mk(B * d.nxh * d.nY);
        h->m.Bvec = mk(B * d.nY);
        h->m.Hpk = mk(B * d.npk);
        if (d.nd > 0) h->m.Gdtab = mk(B * d.Hp * d.ny * d.nd);
    }
    if (!rc) {
        DBuf bj, bb;
        rc = dev_alloc(h, bj, (d.Hc + 1) * sizeof(int));
        if (!rc) rc = dev_alloc(h, bb, d.Hp * sizeof(int));
        if (!rc) {
            hipError_t e1 = hipMemcpy(bj.p, h->jl.data(), (d.Hc + 1) * sizeof(int), hipMemcpyHostToDevice);
            hipError_t e2 = hipMemcpy(bb.p, h->blk.data(), d.Hp * sizeof(int), hipMemcpyHostToDevice);
            if (e1 != hipSuccess || e2 != hipSuccess) { g_hip_err = "hipMemcpy(jl/blk)"; rc = MPCQP_ERR_DEVICE; }
            h->m.jl = (const int*)bj.p;
            h->m.blk = (const int*)bb.p;
        }
    }
    if (rc) { mpcqp_destroy(h); return rc; }
    *out = h;
    return MPCQP_OK;
}

int mpcqp_destroy(mpcqp_handle h) {
    if (!h) return MPCQP_ERR_NULL;
    DeviceGuard guard_(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void* p : h->owned) (void)hipFree(p);
    if (h->ev_s0) (void)hipEventDestroy(h->ev_s0);
    if (h->ev_s1) (void)hipEventDestroy(h->ev_s1);
    if (h->ev_c0) (void)hipEventDestroy(h->ev_c0);
    if (h->ev_c1) (void)hipEventDestroy(h->ev_c1);
    if (h->ev_cm) (void)hipEventDestroy(h->ev_cm);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return MPCQP_OK;
}

int mpcqp_get_sizes(mpcqp_handle h, mpcqp_sizes* out) {
    if (!h || !out) return MPCQP_ERR_NULL;
    out->nZ = h->d.nZ; out->nDU = h->d.nDU; out->nU = h->d.nU; out->nY = h->d.nY; out->nD = h->d.nD;
    return MPCQP_OK;
}

static bool terminal_on(const Dims& d) { return (d.gmask >> (2 * P_X)) & 3u; }

// the condensed kernels keep one problem's tables in the LDS of a CU: a handle whose problem does not fit (nZ~ beyond ~165 at
// C3-like shapes; the fit test is the carve-up of the runtime-dimension kernel, which mpcqp_prepare's comparison needs) has no condensed Hessian and no condensed step -- MPCQP_ERR_UNSUPPORTED from the step / mpcqp_get, the
// MultipleShooting transcription is the way to run it
static bool aot_or_generic_other(const Dims& d) { return step_kernel_kind_other(d) == MPCQP_KERNEL_AOT; }
static bool condensed_fits(const Dims& d) { return step_lds_bytes(d) <= 160 * 1024; }

// K2 for the handle's current tables and weights, or -- when it cannot run now -- the note that Hpk is stale
static int refresh_hessian(mpcqp_handle h, hipStream_t st) {
    h->hessian_valid = false;
    if (h->have_model && h->have_weights && !h->stage_only && condensed_fits(h->d)) {
        HIPCHK(launch_hessian(h->d, h->m, st));
        h->hessian_valid = true;
    }
    return MPCQP_OK;
}
static int ensure_hessian(mpcqp_handle h, hipStream_t st) { return h->hessian_valid ? MPCQP_OK : refresh_hessian(h, st); }

// the step constants: dropped by the setters, built where a step is about to be launched.  Without the launcher (a library
// linked without the kernel) or with a dense L_Hp the handle carries no block and the step forms the values itself.
static void invalidate_stepc(mpcqp_handle h) { h->stepc_valid = false; h->m.stepc = nullptr; }
static int ensure_stepc(mpcqp_handle h, hipStream_t st) {
    if (h->stepc_valid) return MPCQP_OK;
    h->m.stepc = nullptr;
    if (!step_consts_available() || !h->have_weights || h->stage_only || h->m.Ldense) return MPCQP_OK;
    const Dims& d = h->d;
    int rc = dev_alloc(h, h->stepc, (size_t)d.B * SC_N * d.nDU * sizeof(double));
    if (rc) return rc;
    if (h->step_timed) HIPCHK(hipStreamWaitEvent(st, h->ev_s1, 0));     // (an earlier step, on whatever stream, may still read the block)
    HIPCHK(launch_step_consts(d, h->m, (double*)h->stepc.p, st));
    h->m.stepc = (const double*)h->stepc.p;
    h->stepc_valid = true;
    ++h->stepc_builds;
    return MPCQP_OK;
}

static int condense(mpcqp_handle h, hipStream_t st, bool timed) {
    const Dims& d = h->d;
    if (!h->have_model || h->stage_only) return MPCQP_OK;
    const bool term = terminal_on(d);
    if (term && !h->m.exT) {
        DBuf a, b, c, x;
        int rc = dev_alloc(h, a, (size_t)d.B * d.Hc * d.nxh * d.nu * sizeof(double));
        if (!rc) rc = dev_alloc(h, b, (size_t)d.B * d.nxh * d.nxh * sizeof(double));
        if (!rc) rc = dev_alloc(h, c, (size_t)d.B * d.nxh * sizeof(double));
        if (!rc && d.nd > 0) rc = dev_alloc(h, x, (size_t)d.B * d.Hp * d.nxh * d.nd * sizeof(double));
        if (rc) return rc;
        h->m.exT = (double*)a.p; h->m.kxT = (double*)b.p; h->m.bxv = (double*)c.p;
        h->m.Xdtab = d.nd > 0 ? (double*)x.p : nullptr;
    }
    if (h->step_timed && st == h->stream) HIPCHK(hipStreamWaitEvent(st, h->ev_s1, 0));
    if (timed) HIPCHK(hipEventRecord(h->ev_c0, st));
    HIPCHK(launch_predmat(d, h->m, term, st));
    h->terminal_built = term;
    if (timed) HIPCHK(hipEventRecord(h->ev_cm, st));       // between K1 (prediction tables) and K2 (Hessian)
    { int rc = refresh_hessian(h, st); if (rc) return rc; }
    if (timed) { HIPCHK(hipEventRecord(h->ev_c1, st)); h->cond_timed = true; }
    return MPCQP_OK;
}

// ---- ExplicitMPC (src/controller/explicitmpc.jl): H~ factored once per model, a solve or a gain per period ----------------

// what mpcqp_explicit_prepare refuses with MPCQP_ERR_ARG, and what turns a prepared handle away from the explicit calls later
static bool explicit_constrained(mpcqp_handle h) {
    return h->d.neps != 0 || h->d.gmask != 0 || h->transcription != MPCQP_SINGLE_SHOOTING;
}

static void explicit_step_args(mpcqp_handle h, ex::StepArgs& a, uint32_t flags) {
    a.d = h->d;
    a.d.flags = flags;
    a.m = h->m;
    a.Hinv = (const double*)h->ex_Hinv.p;
    a.Lsum = (const double*)h->ex_Lsum.p;
    a.fstatus = (const int32_t*)h->ex_st.p;
}

// Factor (and law) of a prepared handle for the H~ that is resident now, enqueued on `st` behind K2.  Nothing on the host.
// A handle that has become constrained since (its explicit calls answer MPCQP_ERR_ORDER, and with the row groups its problem
// may have outgrown the condensed kernels) is only marked: the setter that called goes on serving the other kernels.
static int explicit_refresh(mpcqp_handle h, hipStream_t st) {
    if (!h->ex_prepared) return MPCQP_OK;
    if (!h->have_model || !h->have_weights) return MPCQP_OK;
    if (explicit_constrained(h)) { h->ex_stale = true; return MPCQP_OK; }
    const Dims& d = h->d;
    const size_t B = d.B, sz = sizeof(double);
    { int rc = ensure_hessian(h, st); if (rc) return rc; }
    if (!h->hessian_valid) return MPCQP_ERR_UNSUPPORTED;
    h->ex_stale = false;
    if (h->step_timed) HIPCHK(hipStreamWaitEvent(st, h->ev_s1, 0));     // (an explicit call on another stream may still read the tables)
    ex::FactorArgs f{};
    f.Hpk = h->m.Hpk; f.Ldiag = h->m.Ldiag; f.jl = h->m.jl;
    f.Hinv = (double*)h->ex_Hinv.p; f.Lsum = (double*)h->ex_Lsum.p;
    f.status = (int32_t*)h->ex_st.p; f.B = d.B; f.n = d.nZ; f.npk = d.npk; f.nu = d.nu; f.Hp = d.Hp;
    HIPCHK(ex::launch_explicit_factor(f, st));
    if (!h->ex_law) return MPCQP_OK;
    // the law by superposition: the explicit step itself on the 1 + nx + nu + ny + nd unit inputs, held over the horizon
    ex::LawBuildArgs lb{};
    lb.xhat0 = (double*)h->ex_bx.p; lb.lastu0 = (double*)h->ex_blu.p; lb.ry = (double*)h->ex_bry.p;
    lb.d0 = d.nd > 0 ? (double*)h->ex_bd0.p : nullptr; lb.Dhat0 = d.nd > 0 ? (double*)h->ex_bdh.p : nullptr;
    lb.Z0 = (const double*)h->ex_bZ0.p; lb.Zk = (const double*)h->ex_bZk.p;
    lb.table_z = (double*)h->ex_law_z.p; lb.table_u = (double*)h->ex_law_u.p;
    lb.B = d.B; lb.n = d.nZ; lb.nx = d.nxh; lb.nu = d.nu; lb.ny = d.ny; lb.nd = d.nd; lb.Hp = d.Hp; lb.kp = ex::law_kp(d);
    ex::StepArgs a{};
    explicit_step_args(h, a, MPCQP_FLAG_RY_CONSTANT);
    a.xhat0 = lb.xhat0; a.lastu0 = lb.lastu0; a.Ry = lb.ry; a.Ru = nullptr; a.d0 = lb.d0; a.Dhat0 = lb.Dhat0;
    a.u0 = (double*)h->ex_bu0.p; a.status = (int32_t*)h->ex_bst.p;
    const int ncol = ex::law_ncol(d);
    for (int k = 0; k < ncol; ++k) {
        HIPCHK(hipMemsetAsync(lb.xhat0, 0, B * d.nxh * sz, st));
        HIPCHK(hipMemsetAsync(lb.lastu0, 0, B * d.nu * sz, st));
        HIPCHK(hipMemsetAsync(lb.ry, 0, B * d.ny * sz, st));
        if (d.nd > 0) {
            HIPCHK(hipMemsetAsync(lb.d0, 0, B * d.nd * sz, st));
            HIPCHK(hipMemsetAsync(lb.Dhat0, 0, B * d.nD * sz, st));
        }
        lb.k = k;
        if (k > 0) HIPCHK(ex::launch_explicit_law_unit(lb, st));
        a.Z = k == 0 ? (double*)h->ex_bZ0.p : (double*)h->ex_bZk.p;
        HIPCHK(ex::launch_explicit_step(a, st));
        HIPCHK(ex::launch_explicit_law_pack(lb, st));
    }
    return MPCQP_OK;
}

// what every explicit call does first: the factor of a handle whose H~ changed while it was constrained
static int explicit_current(mpcqp_handle h, hipStream_t st) { return h->ex_stale ? explicit_refresh(h, st) : MPCQP_OK; }

// ---- InternalModel (include/mpcqp.h; kernels: im_bodies.h) -------------------------------------------------------------------

static void im_args(mpcqp_handle h, im::ImArgs& a) {
    const Dims& d = h->d;
    a.Ahat = h->m.Ahat; a.Bu = h->m.Bu; a.C = h->m.C; a.Bd = d.nd > 0 ? h->m.Bd : nullptr; a.Dd = d.nd > 0 ? h->m.Dd : nullptr;
    a.dop = h->m.dop; a.Bvec = h->m.Bvec; a.i_ym = h->kf.i_ym;
    a.B = d.B; a.nx = d.nxh; a.nu = d.nu; a.ny = d.ny; a.nd = d.nd; a.nym = h->kf.nym; a.nxs = h->im_nxs; a.Hp = d.Hp;
    a.G = im::group_lanes(a.nx, a.nu, a.ny, a.nd, a.nxs);
    a.As = (const double*)h->im_As.p; a.Bs = (const double*)h->im_Bs.p; a.Cs = (const double*)h->im_Cs.p; a.Ds = (const double*)h->im_Ds.p;
    a.Ahs = (double*)h->im_Ahs.p; a.Bhs = (double*)h->im_Bhs.p;
    a.xs = (double*)h->im_xs.p; a.ys = (double*)h->im_ys.p; a.Yhs = (double*)h->im_Yhs.p; a.Beff = (double*)h->im_Beff.p;
    a.z = (double*)h->im_z.p; a.status = (int32_t*)h->im_st.p;
}

// B_eff = B + Ŷs after k_predmat wrote a new B (mpcqp_set_model, mpcqp_recondense_device)
static int im_refresh(mpcqp_handle h, hipStream_t st) {
    if (h->est != EST_IM) return MPCQP_OK;
    im::ImArgs a{};
    im_args(h, a);
    HIPCHK(im::launch_im(a, im::IM_BEFF, st));
    return MPCQP_OK;
}

// ---- what the setters share: the tail that brings the handle's derived data up to date ------------------------------------------

// A new model lies in Ahat .. dop: the kernels read it from now on, and everything derived from it is rebuilt on `st` -- the
// prediction tables and H~, B_eff of an InternalModel (the new B + the Ŷs of the last correction), the explicit factor.
static int model_resident(mpcqp_handle h, bool with_dop, hipStream_t st) {
    const Dims& d = h->d;
    h->m.Ahat = (const double*)h->Ahat.p; h->m.Bu = (const double*)h->Bu.p; h->m.C = (const double*)h->C.p;
    h->m.Bd = d.nd > 0 ? (const double*)h->Bd.p : nullptr;
    h->m.Dd = d.nd > 0 ? (const double*)h->Dd.p : nullptr;
    h->m.dop = with_dop ? (const double*)h->dop.p : nullptr;
    h->have_model = true;
    invalidate_stepc(h);
    int rc = condense(h, st, true);
    if (!rc) rc = im_refresh(h, st);
    return rc ? rc : explicit_refresh(h, st);
}

// A weight changed: the step constants go, H~ and the explicit factor follow it, and the setter returns with them complete.
static int weights_changed(mpcqp_handle h) {
    invalidate_stepc(h);
    int rc = refresh_hessian(h, h->stream);
    if (!rc) rc = explicit_refresh(h, h->stream);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

// The row groups changed: the new layout, then H~ again if it had been skipped (the row groups decide whether the problem
// fits the LDS).  `terminal`: mpcqp_set_bounds, the one setter that can add terminal rows -- their tables come first.
static int rows_changed(mpcqp_handle h, bool terminal = false) {
    layout_rows(h);
    if (terminal && terminal_on(h->d) && !h->terminal_built && h->have_model) {
        int rc = condense(h, h->stream, false);
        if (rc) return rc;
    }
    { int rc = ensure_hessian(h, h->stream); if (rc) return rc; }
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

int mpcqp_set_model(mpcqp_handle h, const double* Ahat, const double* Bu, const double* C,
                    const double* Bd, const double* Dd, const double* dop) {
    if (!h || !Ahat || !Bu || !C) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    if (d.nd > 0 && (!Bd || !Dd)) return MPCQP_ERR_NULL;
    ON_DEVICE(h);
    const size_t B = d.B, sz = sizeof(double);
    int rc = upload(h, h->Ahat, Ahat, B * d.nxh * d.nxh * sz);
    if (!rc) rc = upload(h, h->Bu, Bu, B * d.nxh * d.nu * sz);
    if (!rc) rc = upload(h, h->C, C, B * d.ny * d.nxh * sz);
    if (!rc && d.nd > 0) rc = upload(h, h->Bd, Bd, B * d.nxh * d.nd * sz);
    if (!rc && d.nd > 0) rc = upload(h, h->Dd, Dd, B * d.ny * d.nd * sz);
    if (!rc && dop) rc = upload(h, h->dop, dop, B * d.nxh * sz);
    if (rc) return rc;
    rc = model_resident(h, dop != nullptr, h->stream);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

int mpcqp_set_weights(mpcqp_handle h, const double* Mdiag, const double* Ndiag,
                      const double* Ldiag, const double* Cwt) {
    if (!h || !Mdiag || !Ndiag || !Ldiag) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    if (d.neps && !Cwt) return MPCQP_ERR_NULL;
    ON_DEVICE(h);
    const size_t B = d.B, sz = sizeof(double);
    int rc = upload(h, h->Mdiag, Mdiag, B * d.nY * sz);
    if (!rc) rc = upload(h, h->Ndiag, Ndiag, B * d.nDU * sz);
    if (!rc) rc = upload(h, h->Ldiag, Ldiag, B * d.nU * sz);
    if (!rc && d.neps) rc = upload(h, h->Cwt, Cwt, B * sz);
    if (rc) return rc;
    h->m.Mdiag = (const double*)h->Mdiag.p; h->m.Ndiag = (const double*)h->Ndiag.p;
    h->m.Ldiag = (const double*)h->Ldiag.p;
    h->m.Cwt = d.neps ? (const double*)h->Cwt.p : nullptr;
    h->have_weights = true;
    return weights_changed(h);
}

int mpcqp_set_output_weight_blocks(mpcqp_handle h, const double* Mblk) {
    if (!h) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    if (!h->have_weights) return MPCQP_ERR_ORDER;       // N, L, C come from mpcqp_set_weights
    ON_DEVICE(h);
    if (Mblk) {
        int rc = upload(h, h->Mblk, Mblk, (size_t)d.B * d.Hp * d.ny * d.ny * sizeof(double));
        if (rc) return rc;
        h->m.Mblk = (const double*)h->Mblk.p;
    } else {
        h->m.Mblk = nullptr;
    }
    return weights_changed(h);
}

int mpcqp_set_dense_weights(mpcqp_handle h, const double* M_Hp, const double* N_Hc, const double* L_Hp) {
    if (!h) return MPCQP_ERR_NULL;
    Dims& d = h->d;
    if (!h->have_weights) return MPCQP_ERR_ORDER;       // the diagonals and C come from mpcqp_set_weights
    ON_DEVICE(h);
    struct { const double* src; DBuf* buf; const double** dst; size_t n; } w[3] = {
        {M_Hp, &h->Mfull, &h->m.Mfull, (size_t)d.nY}, {N_Hc, &h->Ndense, &h->m.Ndense, (size_t)d.nDU},
        {L_Hp, &h->Ldense, &h->m.Ldense, (size_t)d.nU}};
    for (auto& e : w) {
        if (e.src) {
            int rc = upload(h, *e.buf, e.src, (size_t)d.B * e.n * e.n * sizeof(double));
            if (rc) return rc;
            *e.dst = (const double*)e.buf->p;
        } else {
            *e.dst = nullptr;
        }
    }
    // stage-separable?  (host pointers: looked at here, once.)  The blocks must be symmetric to the last bit: the stage kernel
    // reads N_j / L_t as they are, one triangle here, the other there (ms_bodies.h), which is the same matrix only then.  A
    // matrix with a block that is not keeps reason 1 and the condensed kernels, which take it as they always did.
    auto separable = [&](const double* a, size_t n, int blk) {
        if (!a) return false;
        for (size_t b = 0; b < (size_t)d.B; ++b)
            for (size_t j = 0; j < n; ++j)
                for (size_t i = 0; i < n; ++i) {
                    const double v = a[b * n * n + i + n * j];
                    if (i / blk != j / blk ? v != 0.0 : v != a[b * n * n + j + n * i]) return false;
                }
        return true;
    };
    h->sepM = separable(M_Hp, (size_t)d.nY, d.ny);
    h->sepN = separable(N_Hc, (size_t)d.nDU, d.nu);
    h->sepL = separable(L_Hp, (size_t)d.nU, d.nu);
    if (h->sepM) {      // the stage kernel's block path reads [Hp][ny][ny]
        std::vector<double> blk((size_t)d.B * d.Hp * d.ny * d.ny);
        const size_t n = (size_t)d.nY;
        for (size_t b = 0; b < (size_t)d.B; ++b)
            for (int t = 0; t < d.Hp; ++t)
                for (int a2 = 0; a2 < d.ny; ++a2)
                    for (int a = 0; a < d.ny; ++a)
                        blk[((b * d.Hp + t) * d.ny + a2) * d.ny + a] = M_Hp[b * n * n + (size_t)(t * d.ny + a) + n * (size_t)(t * d.ny + a2)];
        int rc = upload(h, h->ms_Mblk, blk.data(), blk.size() * sizeof(double));
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));        // (blk leaves scope)
    }
    h->lam_valid = false;
    d.dense_w = (h->m.Mfull || h->m.Ldense) ? 1 : 0;     // (a dense N_Hc only changes H̃: any step kernel serves it)
    return weights_changed(h);
}

int mpcqp_set_flags(mpcqp_handle h, uint32_t flags) {
    if (!h) return MPCQP_ERR_NULL;
    const uint32_t known = MPCQP_FLAG_RY_CONSTANT | MPCQP_FLAG_COLD_START | MPCQP_FLAG_KEEP_QP | MPCQP_FLAG_WARM_DUAL | MPCQP_FLAG_NO_POLISH | MPCQP_FLAG_KEEP_ITERATE;
    if (flags & ~known) return MPCQP_ERR_ARG;
    if ((flags ^ h->d.flags) & MPCQP_FLAG_WARM_DUAL) h->lam_valid = false;
    h->d.flags = flags;
    return MPCQP_OK;
}

int mpcqp_set_custom_constraints(mpcqp_handle h, int nw, const double* Wy, const double* Wu,
                                 const double* Wd, const double* Wr, const double* w_op) {
    if (!h) return MPCQP_ERR_NULL;
    Dims& d = h->d;
    if (nw < 0) return MPCQP_ERR_ARG;
    if (nw > 0 && (!Wy || !Wu)) return MPCQP_ERR_NULL;
    if (nw > 0 && h->est == EST_IM) return MPCQP_ERR_UNSUPPORTED;      // (the ŷ(k) term of the custom rows would need ŷs inside the kernel)
    ON_DEVICE(h);
    Model& m = h->m;
    d.nw = nw; d.nW = nw * (d.Hp + 1);
    d.gmask &= ~(3u << (2 * P_W));          // bounds of a previous definition are dropped
    m.Wy = m.Wu = m.Wd = m.Wr = m.w_op = nullptr;
    m.Wmin = m.Wmax = m.C_wmin = m.C_wmax = nullptr;
    if (nw > 0) {
        const size_t B = d.B, sz = sizeof(double);
        int rc = upload(h, h->Wy, Wy, B * nw * d.ny * sz);
        if (!rc) rc = upload(h, h->Wu, Wu, B * nw * d.nu * sz);
        if (!rc && Wd && d.nd > 0) rc = upload(h, h->Wd, Wd, B * nw * d.nd * sz);
        if (!rc && Wr) rc = upload(h, h->Wr, Wr, B * nw * d.ny * sz);
        if (!rc && w_op) rc = upload(h, h->w_op, w_op, B * nw * sz);
        if (rc) return rc;
        m.Wy = (const double*)h->Wy.p; m.Wu = (const double*)h->Wu.p;
        m.Wd = (Wd && d.nd > 0) ? (const double*)h->Wd.p : nullptr;
        m.Wr = Wr ? (const double*)h->Wr.p : nullptr;
        m.w_op = w_op ? (const double*)h->w_op.p : nullptr;
    }
    return rows_changed(h);
}

int mpcqp_set_current_setpoint(mpcqp_handle h, const double* ry_now) {
    if (!h) return MPCQP_ERR_NULL;
    ON_DEVICE(h);
    if (ry_now) {
        int rc = upload(h, h->ry_now, ry_now, (size_t)h->d.B * h->d.ny * sizeof(double));
        if (rc) return rc;
        h->m.ry_now = (const double*)h->ry_now.p;
        HIPCHK(hipStreamSynchronize(h->stream));
    } else {
        h->m.ry_now = nullptr;
    }
    return MPCQP_OK;
}

int mpcqp_set_custom_bounds(mpcqp_handle h, const double* Wmin, const double* Wmax,
                            const double* C_wmin, const double* C_wmax) {
    if (!h) return MPCQP_ERR_NULL;
    Dims& d = h->d;
    if (d.nw < 1) return MPCQP_ERR_ORDER;               // mpcqp_set_custom_constraints first
    if (!d.neps && (C_wmin || C_wmax)) return MPCQP_ERR_ARG;
    ON_DEVICE(h);
    Model& m = h->m;
    const size_t n = (size_t)d.B * d.nW * sizeof(double);
    const double* src[4] = {Wmin, Wmax, C_wmin, C_wmax};
    DBuf* buf[4] = {&h->Wmin, &h->Wmax, &h->C_wmin, &h->C_wmax};
    const double* dev[4];
    for (int i = 0; i < 4; ++i) {
        dev[i] = nullptr;
        if (!src[i]) continue;
        int rc = upload(h, *buf[i], src[i], n);
        if (rc) return rc;
        dev[i] = (const double*)buf[i]->p;
    }
    m.Wmin = dev[0]; m.Wmax = dev[1]; m.C_wmin = dev[2]; m.C_wmax = dev[3];
    d.gmask &= ~(3u << (2 * P_W));
    if (m.Wmin) d.gmask |= 1u << (2 * P_W);
    if (m.Wmax) d.gmask |= 1u << (2 * P_W + 1);
    return rows_changed(h);
}

int mpcqp_set_bounds(mpcqp_handle h, const mpcqp_bounds* bin) {
    if (!h || !bin) return MPCQP_ERR_NULL;
    Dims& d = h->d;
    if (!d.neps && (bin->C_umin || bin->C_umax || bin->C_dumin || bin->C_dumax || bin->C_ymin ||
                    bin->C_ymax || bin->c_x0min || bin->c_x0max))
        return MPCQP_ERR_ARG;   // "Cwt must be finite to set softness parameters", construct.jl:441
    // U rows of one move-blocking interval are merged into their tightest one (mpcqp_bodies.h);
    // exact as long as the softness of those rows is the same -- true for every `c_umin`/`c_umax`
    // keyword of setconstraint! (repeated per channel).  A horizon-long C_umin/C_umax vector
    // (construct.jl:454-463) that varies inside an interval leaves rows u - c_t eps <= Umax_t of different
    // slopes that no single row replaces: such a handle is served by the stage-structured kernel, which
    // keeps one U row per step (ms_bodies.h) -- if that kernel can take it (ms_unsupported at the step).
    bool varies = false;
    for (const double* cu : {bin->C_umin, bin->C_umax}) {
        if (!cu) continue;
        for (size_t b = 0; b < (size_t)d.B && !varies; ++b)
            for (int j = 0; j < d.Hc && !varies; ++j)
                for (int t = h->jl[j] + 1; t < h->jl[j + 1] && !varies; ++t)
                    for (int c = 0; c < d.nu; ++c)
                        if (cu[b * d.nU + t * d.nu + c] != cu[b * d.nU + h->jl[j] * d.nu + c]) { varies = true; break; }
    }
    h->stage_rows = varies;
    invalidate_stepc(h);
    ON_DEVICE(h);
    const double* src[16] = {bin->U0min, bin->U0max, bin->DUmin, bin->DUmax, bin->Y0min, bin->Y0max,
                             bin->x0min, bin->x0max, bin->C_umin, bin->C_umax, bin->C_dumin,
                             bin->C_dumax, bin->C_ymin, bin->C_ymax, bin->c_x0min, bin->c_x0max};
    const int len[16] = {d.nU, d.nU, d.nDU, d.nDU, d.nY, d.nY, d.nxh, d.nxh,
                         d.nU, d.nU, d.nDU, d.nDU, d.nY, d.nY, d.nxh, d.nxh};
    const double* dev[16];
    for (int i = 0; i < 16; ++i) {
        dev[i] = nullptr;
        if (!src[i]) continue;
        int rc = upload(h, h->bnd[i], src[i], (size_t)d.B * len[i] * sizeof(double));
        if (rc) return rc;
        dev[i] = (const double*)h->bnd[i].p;
    }
    Model& m = h->m;
    m.U0min = dev[0]; m.U0max = dev[1]; m.DUmin = dev[2]; m.DUmax = dev[3];
    m.Y0min = dev[4]; m.Y0max = dev[5]; m.x0min = dev[6]; m.x0max = dev[7];
    m.C_umin = dev[8]; m.C_umax = dev[9]; m.C_dumin = dev[10]; m.C_dumax = dev[11];
    m.C_ymin = dev[12]; m.C_ymax = dev[13]; m.c_x0min = dev[14]; m.c_x0max = dev[15];
    uint32_t g = 0;
    // box lower: hard ΔUmin rows, and the row ϵ >= 0 unless a Ŷ group exists (it then rides there: eps_host_group)
    if (m.DUmin || (d.neps && !m.Y0min && !m.Y0max)) g |= 1u << 0;
    if (m.DUmax) g |= 1u << 1;                           // box upper
    if (m.U0min) g |= 1u << (2 * P_U);
    if (m.U0max) g |= 1u << (2 * P_U + 1);
    if (d.neps && m.DUmin && m.C_dumin) g |= 1u << (2 * P_DU);
    if (d.neps && m.DUmax && m.C_dumax) g |= 1u << (2 * P_DU + 1);
    if (m.Y0min) g |= 1u << (2 * P_Y);
    if (m.Y0max) g |= 1u << (2 * P_Y + 1);
    if (m.x0min) g |= 1u << (2 * P_X);
    if (m.x0max) g |= 1u << (2 * P_X + 1);
    g |= d.gmask & (3u << (2 * P_W));                    // custom rows: mpcqp_set_custom_bounds
    d.gmask = g;
    return rows_changed(h, true);
}

// the handle is routed to the stage-structured kernel: asked for (MultipleShooting), or the condensed kernels cannot take it
// (round 5: also a condensed problem of nZ~ <= 256 that does not fit the LDS of a CU -- nZ~ beyond ~165 at C3-like shapes -- whatever
//  its transcription: the SAME QP, solved in stage form)
static bool uses_stage_kernel(mpcqp_handle h) {
    return h->transcription == MPCQP_MULTIPLE_SHOOTING || h->stage_only || h->stage_rows || !condensed_fits(h->d);
}

// 0 when the MultipleShooting kernel takes this handle; else the reason (bit mask): 1 weight matrices that couple different
// stages (a cost that is not block-tridiagonal: no Riccati recursion solves it) or output blocks beyond ny = 256, 4 the
// stage data does not fit the 160 KB of LDS.  (2, custom linear constraints, and 8, MPCQP_FLAG_KEEP_QP / _WARM_DUAL, are no
// longer set: the stage kernel takes them -- ms_bodies.h.  The values stay reserved.)
static int ms_unsupported(mpcqp_handle h) {
    int why = 0;
    if ((h->m.Mfull && !h->sepM) || (h->m.Ndense && !h->sepN) || (h->m.Ldense && !h->sepL)) why |= 1;
    if ((h->m.Mblk || h->m.Mfull) && h->d.ny > 4 * WAVE) why |= 1;   // (the block-weight sweep of ms_bodies.h keeps a column in four registers per lane)
    if (ms_lds_bytes(h->d, h->m) > 160 * 1024) why |= 4;
    return why;
}

int mpcqp_set_transcription(mpcqp_handle h, int32_t transcription) {
    if (!h) return MPCQP_ERR_NULL;
    if (transcription != MPCQP_SINGLE_SHOOTING && transcription != MPCQP_MULTIPLE_SHOOTING) return MPCQP_ERR_ARG;
    h->transcription = transcription;
    h->lam_valid = false;       // (the handle may move between the condensed and the stage kernels: another row order)
    return MPCQP_OK;
}

int mpcqp_transcription_supported(mpcqp_handle h) {
    if (!h) return MPCQP_ERR_NULL;
    return uses_stage_kernel(h) ? ms_unsupported(h) : 0;
}

// One launch of the covariance / gain recursion of a time-varying handle (kf_kernels.hip) on the model that is resident
// now: mode bit 0 the correction (K̂(k), P̂(k|k)), bit 1 the prediction (P̂(k+1|k)), bit 2 a period without measurements.
// y0m (device, [B][nym]) of a correction: the estimators whose row holds a NaN miss it.
static int kf_cov_launch(mpcqp_handle h, int mode, const double* y0m, hipStream_t st) {
    if (!kf::kf_cov_available()) return MPCQP_ERR_UNSUPPORTED;
    ON_DEVICE(h);
    const Dims& d = h->d;
    kf::CovArgs a{};
    a.Ahat = h->m.Ahat; a.C = h->m.C; a.i_ym = h->kf.i_ym;
    a.Q = (const double*)h->kf_Q.p; a.R = (const double*)h->kf_R.p;
    a.P = (double*)h->kf_P.p; a.K = (double*)h->kf_K.p; a.status = (int32_t*)h->kf_st.p;
    a.B = d.B; a.nx = d.nxh; a.ny = d.ny; a.nym = h->kf.nym;
    a.NX = h->kf_NX; a.nwaves = h->kf_waves;
    a.y0m = y0m;
    HIPCHK(kf::launch_kf_cov(a, mode, st));
    return MPCQP_OK;
}

// shared by mpcqp_step_device (kf = false) and mpcqp_loop_device
static int step_device_impl(mpcqp_handle h, const double* xhat0, const double* lastu0, const double* Ry,
                            const double* Ru, const double* d0, const double* Dhat0, double* Ztilde, double* u0,
                            int32_t* status, int32_t* iters, double* Yhat0, void* stream,
                            const double* y0m, double* xhat0_out, int predict) {
    if (!h || !xhat0 || !lastu0 || !Ry || !Ztilde || !u0 || !status) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    if (d.nd > 0 && (!d0 || !Dhat0)) return MPCQP_ERR_NULL;
    if (!h->have_model || !h->have_weights) return MPCQP_ERR_ORDER;
    ON_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    StepIO io{};
    io.xhat0 = xhat0; io.lastu0 = lastu0; io.Ry = Ry; io.Ru = Ru; io.d0 = d0; io.Dhat0 = Dhat0;
    io.Z = Ztilde; io.u0 = u0; io.Yhat0 = Yhat0; io.status = status; io.iters = iters;
    if (y0m) {
        io.kf_K = h->kf.Khat; io.kf_iym = h->kf.i_ym; io.kf_nym = h->kf.nym;
        io.kf_y0m = y0m; io.xhat0_out = xhat0_out; io.kf_predict = predict;
        io.kf_late = h->kf_direct ? 0 : 1;
    }
    {       // what the convergence test of every solve saw last (mpcqp_get MPCQP_GET_AUDIT)
        int rc = dev_alloc(h, h->audit, (size_t)d.B * 4 * sizeof(double));
        if (rc) return rc;
        io.audit = (double*)h->audit.p;
    }
    if (d.flags & MPCQP_FLAG_KEEP_QP) {
        int rc = dev_alloc(h, h->keep_q, (size_t)d.B * d.nZ * sizeof(double));
        if (!rc) rc = dev_alloc(h, h->keep_F, (size_t)d.B * d.nY * sizeof(double));
        if (rc) return rc;
        io.q_keep = (double*)h->keep_q.p;
        io.F_keep = (double*)h->keep_F.p;
    }
    if (d.flags & MPCQP_FLAG_WARM_DUAL) {
        // sized for the kernel that runs: the rows of the condensed kernels or of the stage carve; multipliers stored by the
        // other kind, or for another number of rows, do not line up (a setter moved the handle between the kernels)
        const bool stage = uses_stage_kernel(h);
        const int rows = stage ? make_ms_carve(d, h->m).nrows : d.nrows();
        if (stage != h->lam_stage || rows != h->lam_rows) h->lam_valid = false;
        h->lam_stage = stage; h->lam_rows = rows;
        const size_t nl = (size_t)d.B * (size_t)(rows > 0 ? rows : 1) * sizeof(double);
        if (!h->lam.p || h->lam.bytes < nl) h->lam_valid = false;
        int rc = dev_alloc(h, h->lam, nl);
        if (rc) return rc;
        io.lam_out = (double*)h->lam.p;
        io.lam_prev = h->lam_valid ? (const double*)h->lam.p : nullptr;
        h->lam_valid = true;
    }
#ifdef MPCQP_PROFILE
    {
        int rc = dev_alloc(h, h->prof, (size_t)d.B * 16 * sizeof(double));
        if (rc) return rc;
        io.prof = (double*)h->prof.p;
    }
#endif
    // (refusals first: nothing is recorded on the stream for a step that does not run)
    if (uses_stage_kernel(h) && ms_unsupported(h)) return MPCQP_ERR_UNSUPPORTED;      // (the fused Kalman loop runs on the stage-structured kernel too since round 6)
    if (h->est == EST_IM && (uses_stage_kernel(h) || d.nW > 0)) return MPCQP_ERR_UNSUPPORTED;  // (the stage kernel does not read B; custom rows need ŷs)
    // (the step constants are handle data like H~: built before the step's time starts)
    if (!uses_stage_kernel(h)) { int rc = ensure_stepc(h, st); if (rc) return rc; }
    HIPCHK(hipEventRecord(h->ev_s0, st));
    if (uses_stage_kernel(h)) {
        // the stage-structured kernel: model as equality constraints, Riccati recursion, H~ and E never formed
        MsIO ms{};
        int rc = dev_alloc(h, h->ms_X, (size_t)d.B * d.nxh * d.Hp * sizeof(double));
        if (!rc) rc = dev_alloc(h, h->ms_defect, (size_t)d.B * sizeof(double));
        if (rc) return rc;
        ms.Xhat = (double*)h->ms_X.p; ms.defect = (double*)h->ms_defect.p;
        {   // horizon-long data of the resident wavefronts when they do not fit the LDS share (ms_kernels.hip)
            int nslots = 0;
            const size_t sb = ms_scratch_bytes(d, h->m, &nslots);
            if (sb) {
                rc = dev_alloc(h, h->ms_scratch, sb);
                if (rc) return rc;
                ms.scratch = (double*)h->ms_scratch.p; ms.nslots = nslots;
                rc = dev_alloc(h, h->ms_next, sizeof(int));
                if (rc) return rc;
                ms.next = (int*)h->ms_next.p;
            }
        }
        // (dual regularisation: the handle's, default 1e-12 like the condensed kernels.  Measured on 8192 C3 controllers
        //  against the condensed kernel once the gains of the Riccati recursion are refined (ms_bodies.h: factor):
        //  delta 1e-12 / 1e-10 / 1e-9: not OPTIMAL 0 / 3 / 5, worst dU difference 2.7e-6 / 1.4e-2 / 1 (error branch), 99.9 %
        //  quantile 2e-7 / 3e-8 / 2e-7; profiles/r4/ms_delta_sweep.txt)
        // stage-separable weights of mpcqp_set_dense_weights: M_Hp on the block path (its blocks, extracted at the setter),
        // N_Hc and L_Hp read block by block out of the dense matrices
        Model mm = h->m;
        if (mm.Mfull && h->sepM) mm.Mblk = (const double*)h->ms_Mblk.p;
        if (mm.Ndense && h->sepN) ms.blocks |= MS_BLK_N;
        if (mm.Ldense && h->sepL) ms.blocks |= MS_BLK_L;
        Dims dm = d;
        HIPCHK(launch_ms_step(dm, mm, io, ms, st));
    } else {
        { int rc = ensure_hessian(h, st); if (rc) return rc; }      // (skipped while the problem did not fit the LDS: see hessian_valid)
        if (h->est == EST_IM) {       // InternalModel: the same kernels on B + Ŷs (k_im_correct keeps it current)
            Model mm = h->m;
            mm.Bvec = (double*)h->im_Beff.p;
            HIPCHK(launch_step(d, mm, io, st));
        } else {
            HIPCHK(launch_step(d, h->m, io, st));
        }
    }
    HIPCHK(hipEventRecord(h->ev_s1, st));
    h->step_timed = true;
    return MPCQP_OK;
}

int mpcqp_step_device(mpcqp_handle h, const double* xhat0, const double* lastu0,
                      const double* Ry, const double* Ru, const double* d0, const double* Dhat0,
                      double* Ztilde, double* u0, int32_t* status, int32_t* iters,
                      double* Yhat0, void* stream) {
    return step_device_impl(h, xhat0, lastu0, Ry, Ru, d0, Dhat0, Ztilde, u0, status, iters, Yhat0, stream,
                            nullptr, nullptr, 0);
}

int mpcqp_loop_device(mpcqp_handle h, double* xhat0, const double* y0m, const double* lastu0,
                      const double* Ry, const double* Ru, const double* d0, const double* Dhat0,
                      double* Ztilde, double* u0, int32_t* status, int32_t* iters, double* Yhat0,
                      void* stream) {
    if (!h || !y0m || !xhat0) return MPCQP_ERR_NULL;
    if (h->est == EST_IM) {
        // InternalModel: correct (ŷs, Ŷs, B + Ŷs), the step on x̂0 = x̂d, update (x̂d in place, x̂s), three calls on the caller's
        // stream.  Refusals first: a step that does not run leaves the estimator alone
        if (!lastu0 || !Ry || !Ztilde || !u0 || !status || (h->d.nd > 0 && (!d0 || !Dhat0))) return MPCQP_ERR_NULL;
        if (!h->have_model || !h->have_weights) return MPCQP_ERR_ORDER;
        if (uses_stage_kernel(h) || h->d.nW > 0) return MPCQP_ERR_UNSUPPORTED;
        int rc = mpcqp_im_correct_device(h, xhat0, y0m, d0, stream);
        if (!rc) rc = step_device_impl(h, xhat0, lastu0, Ry, Ru, d0, Dhat0, Ztilde, u0, status, iters, Yhat0, stream, nullptr, nullptr, 0);
        return rc ? rc : mpcqp_im_update_device(h, xhat0, u0, d0, stream);
    }
    if (h->est == EST_MHE) {
        // a MovingHorizonEstimator behind the controller: preparestate!, the step on the estimator's own x̂0 (read in place),
        // updatestate!, three calls on the caller's stream.  Refusals first: a step that does not run leaves the windows alone
        if (!lastu0 || !Ry || !Ztilde || !u0 || !status || (h->d.nd > 0 && (!d0 || !Dhat0))) return MPCQP_ERR_NULL;
        if (!h->have_model || !h->have_weights) return MPCQP_ERR_ORDER;
        if (uses_stage_kernel(h) && ms_unsupported(h)) return MPCQP_ERR_UNSUPPORTED;
        const double* xe = (const double*)mpcqp_mhe_device_ptr(h->mhe, MPCQP_MHE_XHAT0);
        int rc = mpcqp_mhe_prepare_stream(h->mhe, y0m, d0, stream);
        if (!rc) rc = step_device_impl(h, xe, lastu0, Ry, Ru, d0, Dhat0, Ztilde, u0, status, iters, Yhat0, stream, nullptr, nullptr, 0);
        if (rc) return rc;
        {
            ON_DEVICE(h);
            HIPCHK(hipMemcpyAsync(xhat0, xe, (size_t)h->d.B * h->d.nxh * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        }
        return mpcqp_mhe_update_stream(h->mhe, u0, y0m, d0, stream);
    }
    if (!est_is_kf(h)) return MPCQP_ERR_ORDER;
    if (h->d.nxh > 4 * WAVE) return MPCQP_ERR_UNSUPPORTED;
    // K̂(k) and P̂(k+1|k) first, in either form: the recursion depends on which measurements are missing and on nothing else
    // (a refused step leaves P̂ one period ahead)
    if (h->est == EST_KF_TV) {
        if (!lastu0 || !Ry || !Ztilde || !u0 || !status || (h->d.nd > 0 && (!d0 || !Dhat0))) return MPCQP_ERR_NULL;
        if (!h->have_model || !h->have_weights) return MPCQP_ERR_ORDER;
        if (uses_stage_kernel(h) && ms_unsupported(h)) return MPCQP_ERR_UNSUPPORTED;
        int rc = kf_cov_launch(h, kf::COV_CORRECT | kf::COV_PREDICT, y0m, (hipStream_t)stream);
        if (rc) return rc;
    }
    return step_device_impl(h, xhat0, lastu0, Ry, Ru, d0, Dhat0, Ztilde, u0, status, iters, Yhat0, stream,
                            y0m, xhat0, 1);
}

// The host-pointer step of one handle on its own stream, up to and without the wait: mpcqp_step waits for its handle,
// mpcqp_multi_step for every shard after all of them are enqueued.  The caller has checked the pointers and holds the device.
static int step_staged(mpcqp_handle h, const double* xhat0, const double* lastu0, const double* Ry, const double* Ru,
                       const double* d0, const double* Dhat0, double* Ztilde, double* u0, int32_t* status, int32_t* iters,
                       double* Yhat0) {
    const Dims& d = h->d;
    const size_t B = d.B, sz = sizeof(double);
    const size_t nry = (d.flags & MPCQP_FLAG_RY_CONSTANT) ? d.ny : d.nY;
    Staging s{h};
    const double* dx = s.in(h->s_x, xhat0, B * d.nxh);
    const double* dlu = s.in(h->s_lu, lastu0, B * d.nu);
    const double* dry = s.in(h->s_ry, Ry, B * nry);
    const double* dru = s.in(h->s_ru, Ru, B * d.nU);
    const double* dd0 = s.in(h->s_d0, d.nd > 0 ? d0 : nullptr, B * d.nd);
    const double* ddh = s.in(h->s_dh, d.nd > 0 ? Dhat0 : nullptr, B * d.nD);
    double* dZ = s.in(h->s_Z, Ztilde, B * d.nZ);
    double* du0 = s.out<double>(h->s_u0, B * d.nu);
    int32_t* dst = s.out<int32_t>(h->s_st, B);
    int32_t* dit = s.out<int32_t>(h->s_it, B);
    double* dyh = Yhat0 ? s.out<double>(h->s_yh, B * d.nY) : nullptr;
    if (s.rc) return s.rc;
    s.rc = mpcqp_step_device(h, dx, dlu, dry, dru, dd0, ddh, dZ, du0, dst, dit, dyh, h->stream);
    s.down(Ztilde, h->s_Z, B * d.nZ * sz);
    s.down(u0, h->s_u0, B * d.nu * sz);
    s.down(status, h->s_st, B * sizeof(int32_t));
    s.down(iters, h->s_it, B * sizeof(int32_t));
    s.down(Yhat0, h->s_yh, B * d.nY * sz);
    return s.rc;
}

int mpcqp_step(mpcqp_handle h, const double* xhat0, const double* lastu0, const double* Ry,
               const double* Ru, const double* d0, const double* Dhat0, double* Ztilde,
               double* u0, int32_t* status, int32_t* iters, double* Yhat0) {
    if (!h || !xhat0 || !lastu0 || !Ry || !Ztilde || !u0 || !status) return MPCQP_ERR_NULL;
    if (h->d.nd > 0 && (!d0 || !Dhat0)) return MPCQP_ERR_NULL;
    ON_DEVICE(h);
    int rc = step_staged(h, xhat0, lastu0, Ry, Ru, d0, Dhat0, Ztilde, u0, status, iters, Yhat0);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

int mpcqp_recondense_device(mpcqp_handle h, void* stream) {
    if (!h) return MPCQP_ERR_NULL;
    if (!h->have_model || !h->have_weights) return MPCQP_ERR_ORDER;
    ON_DEVICE(h);
    int rc = condense(h, (hipStream_t)stream, true);
    if (!rc) rc = im_refresh(h, (hipStream_t)stream);
    return rc ? rc : explicit_refresh(h, (hipStream_t)stream);
}

// ---- LinModel(sys, Ts) + augment_model for the whole batch (linmodel.jl:165-198, construct.jl:305-323; c2d_bodies.h) ----

// Dimensions, options and the table of stochastic states of a call; everything but the arrays of C2dArgs.
static int c2d_fill(const mpcqp_c2d_spec* s, c2d::C2dArgs& a) {
    if (!s) return MPCQP_ERR_NULL;
    if (s->batch < 1 || s->nx < 1 || s->nu < 1 || s->ny < 1 || s->nd < 0 || s->nym < 0 || s->nym > s->ny) return MPCQP_ERR_DIMS;
    if (s->d_method != MPCQP_C2D_TUSTIN && s->d_method != MPCQP_C2D_ZOH) return MPCQP_ERR_ARG;
    if (s->nint_ym && s->nym < 1) return MPCQP_ERR_DIMS;
    a.B = s->batch; a.nx = s->nx; a.nu = s->nu; a.ny = s->ny; a.nd = s->nd;
    a.method = s->d_method == MPCQP_C2D_ZOH ? c2d::C2D_ZOH : c2d::C2D_TUSTIN;
    long nsu = 0, nsy = 0;
    for (int i = 0; s->nint_u && i < s->nu; ++i) {
        if (s->nint_u[i] < 0) return MPCQP_ERR_ARG;
        nsu += s->nint_u[i];
    }
    for (int i = 0; i < s->nym; ++i) {
        const int q = s->i_ym ? s->i_ym[i] : i;
        if (q < 0 || q >= s->ny) return MPCQP_ERR_ARG;          // validate_ym, construct.jl:188-194
        for (int j = 0; j < i; ++j)
            if ((s->i_ym ? s->i_ym[j] : j) == q) return MPCQP_ERR_ARG;
        if (s->nint_ym) {
            if (s->nint_ym[i] < 0) return MPCQP_ERR_ARG;
            nsy += s->nint_ym[i];
        }
    }
    const bool tust = a.nd > 0 && a.method == c2d::C2D_TUSTIN;
    const long nxd = tust ? 2L * a.nx : a.nx, nxh = nxd + nsu + nsy;
    if (nxh > c2d::C2D_NXH_MAX || nsu + nsy > c2d::C2D_NXH_MAX) return MPCQP_ERR_UNSUPPORTED;
    a.nsu = (int)nsu; a.nsy = (int)nsy; a.nxd = (int)nxd; a.nxh = (int)nxh;
    if (!c2d::c2d_supported(a) || !c2d::c2d_available()) return MPCQP_ERR_UNSUPPORTED;
    int p = 0;
    for (int i = 0; s->nint_u && i < s->nu; ++i)
        for (int k = 0; k < s->nint_u[i]; ++k, ++p) {
            a.s_in[p] = (signed char)(k == s->nint_u[i] - 1 ? i : -1);
            a.s_out[p] = -1;
            a.s_prev[p] = k > 0;
        }
    for (int i = 0; s->nint_ym && i < s->nym; ++i)
        for (int k = 0; k < s->nint_ym[i]; ++k, ++p) {
            a.s_in[p] = -1;
            a.s_out[p] = (signed char)(k == s->nint_ym[i] - 1 ? (s->i_ym ? s->i_ym[i] : i) : -1);
            a.s_prev[p] = k > 0;
        }
    return MPCQP_OK;
}

static bool c2d_in_ok(const c2d::C2dArgs& a, const mpcqp_c2d_in* in) {
    return in && in->A && in->Bu && in->C && in->Ts && (a.nd == 0 || (in->Bd && in->Dd));
}

int mpcqp_c2d_sizes(const mpcqp_c2d_spec* spec, int32_t* nx_dis, int32_t* nxhat) {
    c2d::C2dArgs a{};
    const int rc = c2d_fill(spec, a);
    if (rc && rc != MPCQP_ERR_UNSUPPORTED) return rc;
    if (rc && a.nxh == 0) return rc;                            // (beyond 64 states: no size to report)
    if (nx_dis) *nx_dis = a.nxd;
    if (nxhat) *nxhat = a.nxh;
    return rc;
}

int mpcqp_c2d_device(const mpcqp_c2d_spec* spec, const mpcqp_c2d_in* in, const mpcqp_c2d_out* out, int32_t* status, void* stream) {
    c2d::C2dArgs a{};
    if (!spec || !in || !out || !status) return MPCQP_ERR_NULL;
    int rc = c2d_fill(spec, a);
    if (rc) return rc;
    if (!c2d_in_ok(a, in) || !out->Ahat || !out->Bu || !out->C || (a.nd > 0 && (!out->Bd || !out->Dd)) || (in->dop && !out->dop))
        return MPCQP_ERR_NULL;
    a.A = in->A; a.Bu = in->Bu; a.C = in->C; a.Bd = in->Bd; a.Dd = in->Dd; a.Ts = in->Ts; a.dop = in->dop;
    a.Ahat = out->Ahat; a.Bhu = out->Bu; a.Chat = out->C; a.Bhd = out->Bd; a.Dhd = out->Dd;
    a.dophat = in->dop ? out->dop : nullptr;
    a.status = status;
    HIPCHK(c2d::launch_c2d(a, (hipStream_t)stream));
    return MPCQP_OK;
}

int mpcqp_c2d(const mpcqp_c2d_spec* spec, const mpcqp_c2d_in* in, const mpcqp_c2d_out* out, int32_t* status) {
    c2d::C2dArgs a{};
    if (!spec || !in || !out || !status) return MPCQP_ERR_NULL;
    int rc = c2d_fill(spec, a);
    if (rc) return rc;
    if (!c2d_in_ok(a, in) || !out->Ahat || !out->Bu || !out->C || (a.nd > 0 && (!out->Bd || !out->Dd)) || (in->dop && !out->dop))
        return MPCQP_ERR_NULL;
    const size_t B = a.B, sz = sizeof(double);
    // device copies of the inputs and of the outputs AS THE CALLER HAS THEM: a refused member's outputs come back unchanged
    struct Tmp {
        std::vector<void*> p;
        ~Tmp() { for (void* q : p) (void)hipFree(q); }
    } tmp;
    auto dev = [&](const void* src, size_t bytes, void** dst) -> int {
        *dst = nullptr;
        if (!src) return MPCQP_OK;
        hipError_t e = hipMalloc(dst, bytes ? bytes : 8);
        if (e != hipSuccess) { g_hip_err = std::string("hipMalloc: ") + hipGetErrorString(e); return e == hipErrorOutOfMemory ? MPCQP_ERR_NOMEM : MPCQP_ERR_DEVICE; }
        tmp.p.push_back(*dst);
        HIPCHK(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
        return MPCQP_OK;
    };
    const size_t nin[7] = {B * a.nx * a.nx * sz, B * a.nx * a.nu * sz, B * a.ny * a.nx * sz, B * a.nx * a.nd * sz, B * a.ny * a.nd * sz,
                           B * sz, B * a.nxd * sz};
    const size_t nout[6] = {B * a.nxh * a.nxh * sz, B * a.nxh * a.nu * sz, B * a.ny * a.nxh * sz, B * a.nxh * a.nd * sz,
                            B * a.ny * a.nd * sz, B * a.nxh * sz};
    const void* hin[7] = {in->A, in->Bu, in->C, a.nd > 0 ? in->Bd : nullptr, a.nd > 0 ? in->Dd : nullptr, in->Ts, in->dop};
    void* hout[6] = {out->Ahat, out->Bu, out->C, a.nd > 0 ? out->Bd : nullptr, a.nd > 0 ? out->Dd : nullptr, in->dop ? out->dop : nullptr};
    void *din[7], *dout[6], *dst = nullptr;
    for (int i = 0; i < 7 && !rc; ++i) rc = dev(hin[i], nin[i], &din[i]);
    for (int i = 0; i < 6 && !rc; ++i) rc = dev(hout[i], nout[i], &dout[i]);
    if (!rc) rc = dev(status, B * sizeof(int32_t), &dst);
    if (rc) return rc;
    mpcqp_c2d_in di{(const double*)din[0], (const double*)din[1], (const double*)din[2], (const double*)din[3], (const double*)din[4],
                    (const double*)din[5], (const double*)din[6]};
    mpcqp_c2d_out dout_{(double*)dout[0], (double*)dout[1], (double*)dout[2], (double*)dout[3], (double*)dout[4], (double*)dout[5]};
    rc = mpcqp_c2d_device(spec, &di, &dout_, (int32_t*)dst, nullptr);
    if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    for (int i = 0; i < 6; ++i)
        if (hout[i]) HIPCHK(hipMemcpy(hout[i], dout[i], nout[i], hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(status, dst, B * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MPCQP_OK;
}

int mpcqp_set_model_continuous_device(mpcqp_handle h, const mpcqp_c2d_spec* spec, const mpcqp_c2d_in* in, int32_t* status, void* stream) {
    if (!h || !spec || !in || !status) return MPCQP_ERR_NULL;
    c2d::C2dArgs a{};
    int rc = c2d_fill(spec, a);
    if (rc) return rc;
    const Dims& d = h->d;
    if (a.B != d.B || a.nxh != d.nxh || a.nu != d.nu || a.ny != d.ny || a.nd != d.nd) return MPCQP_ERR_ARG;
    if (h->in_multi) return MPCQP_ERR_UNSUPPORTED;
    if (!c2d_in_ok(a, in)) return MPCQP_ERR_NULL;
    ON_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    const size_t B = d.B, sz = sizeof(double);
    const bool first = !h->have_model;                          // (no model to keep: a refused member then has a zero model)
    struct { DBuf* b; size_t n; bool on; } bufs[6] = {
        {&h->Ahat, B * d.nxh * d.nxh * sz, true}, {&h->Bu, B * d.nxh * d.nu * sz, true}, {&h->C, B * d.ny * d.nxh * sz, true},
        {&h->Bd, B * d.nxh * d.nd * sz, d.nd > 0}, {&h->Dd, B * d.ny * d.nd * sz, d.nd > 0}, {&h->dop, B * d.nxh * sz, in->dop != nullptr}};
    for (auto& e : bufs) {
        if (!e.on) continue;
        const bool fresh = !e.b->p || e.b->bytes < e.n;
        rc = dev_alloc(h, *e.b, e.n);
        if (rc) return rc;
        if (first || fresh) HIPCHK(hipMemsetAsync(e.b->p, 0, e.n, st));
    }
    if (h->step_timed) HIPCHK(hipStreamWaitEvent(st, h->ev_s1, 0));    // (a step on another stream may still read the model)
    a.A = in->A; a.Bu = in->Bu; a.C = in->C; a.Bd = in->Bd; a.Dd = in->Dd; a.Ts = in->Ts; a.dop = in->dop;
    a.Ahat = (double*)h->Ahat.p; a.Bhu = (double*)h->Bu.p; a.Chat = (double*)h->C.p;
    a.Bhd = d.nd > 0 ? (double*)h->Bd.p : nullptr; a.Dhd = d.nd > 0 ? (double*)h->Dd.p : nullptr;
    a.dophat = in->dop ? (double*)h->dop.p : nullptr;
    a.status = status;
    HIPCHK(c2d::launch_c2d(a, st));
    return model_resident(h, in->dop != nullptr, st);       // (no wait: everything is on the caller's stream)
}

int mpcqp_set_model_continuous(mpcqp_handle h, const mpcqp_c2d_spec* spec, const mpcqp_c2d_in* in, int32_t* status) {
    if (!h || !spec || !in || !status) return MPCQP_ERR_NULL;
    c2d::C2dArgs a{};
    int rc = c2d_fill(spec, a);
    if (rc) return rc;
    const Dims& d = h->d;
    if (a.B != d.B || a.nxh != d.nxh || a.nu != d.nu || a.ny != d.ny || a.nd != d.nd) return MPCQP_ERR_ARG;
    if (h->in_multi) return MPCQP_ERR_UNSUPPORTED;
    if (!c2d_in_ok(a, in)) return MPCQP_ERR_NULL;
    ON_DEVICE(h);
    const size_t B = d.B;
    const size_t nin[7] = {B * a.nx * a.nx, B * a.nx * a.nu, B * a.ny * a.nx, B * a.nx * a.nd, B * a.ny * a.nd, B, B * a.nxd};
    const double* hin[7] = {in->A, in->Bu, in->C, a.nd > 0 ? in->Bd : nullptr, a.nd > 0 ? in->Dd : nullptr, in->Ts, in->dop};
    const double* din[7];
    Staging s{h};
    for (int i = 0; i < 7; ++i) din[i] = s.in(h->c2d_s[i], hin[i], nin[i]);
    int32_t* dst = s.out<int32_t>(h->c2d_st, B);
    if (s.rc) return s.rc;
    mpcqp_c2d_in di{din[0], din[1], din[2], din[3], din[4], din[5], din[6]};
    s.rc = mpcqp_set_model_continuous_device(h, spec, &di, dst, h->stream);
    s.down(status, h->c2d_st, B * sizeof(int32_t));
    return s.finish();
}

int mpcqp_get(mpcqp_handle h, int which, double* out) {
    if (!h || !out) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    ON_DEVICE(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipDeviceSynchronize());
    const size_t B = d.B;
    auto fetch = [&](const void* src, size_t n, std::vector<double>& tmp) -> int {
        tmp.resize(n);
        HIPCHK(hipMemcpy(tmp.data(), src, n * sizeof(double), hipMemcpyDeviceToHost));
        return MPCQP_OK;
    };
    // the arrays that go out as they lie on the device: the refusal of the case if there is one, else B * n doubles from src
    auto plain = [&](int refuse, const void* src, size_t n) -> int {
        if (refuse) return refuse;
        HIPCHK(hipMemcpy(out, src, B * n * sizeof(double), hipMemcpyDeviceToHost));
        return MPCQP_OK;
    };
    const int no_tables = h->stage_only ? MPCQP_ERR_UNSUPPORTED : !h->have_model ? MPCQP_ERR_ORDER : 0;   // (K1's tables)
    const int no_im = h->est == EST_IM ? 0 : MPCQP_ERR_ORDER;
    std::vector<double> tmp;
    switch (which) {
        case MPCQP_GET_HESSIAN: {
            if (h->stage_only || !condensed_fits(d)) return MPCQP_ERR_UNSUPPORTED;       // (nothing is condensed for nZ~ > 256; no Hessian kernel beyond the LDS)
            if (!h->have_model || !h->have_weights) return MPCQP_ERR_ORDER;
            int rc = ensure_hessian(h, h->stream);
            if (rc) return rc;
            HIPCHK(hipStreamSynchronize(h->stream));
            rc = fetch(h->m.Hpk, B * d.npk, tmp);
            if (rc) return rc;
            for (size_t b = 0; b < B; ++b)
                for (int i = 0; i < d.nZ; ++i)
                    for (int j = 0; j <= i; ++j) {
                        double v = tmp[b * d.npk + pk(i, j)];
                        out[b * d.nZ * d.nZ + i + (size_t)d.nZ * j] = v;
                        out[b * d.nZ * d.nZ + j + (size_t)d.nZ * i] = v;
                    }
            return MPCQP_OK;
        }
        case MPCQP_GET_STEPRESP: {
            if (h->stage_only) return MPCQP_ERR_UNSUPPORTED;
            if (!h->have_model) return MPCQP_ERR_ORDER;
            int rc = fetch(h->m.Stab, B * d.Hp * d.ny * d.nu, tmp);
            if (rc) return rc;
            for (size_t b = 0; b < B; ++b)
                for (int mm = 0; mm < d.Hp; ++mm)
                    for (int a = 0; a < d.ny; ++a)
                        for (int c = 0; c < d.nu; ++c)
                            out[((b * d.Hp + mm) * d.nu + c) * d.ny + a] =
                                tmp[((b * d.Hp + mm) * d.ny + a) * d.nu + c];
            return MPCQP_OK;
        }
        case MPCQP_GET_KMAT: return plain(no_tables, h->m.Ktab, (size_t)d.nxh * d.nY);
        case MPCQP_GET_BVEC: return plain(no_tables, h->m.Bvec, d.nY);
        case MPCQP_GET_QTILDE: return plain(h->keep_q.p ? 0 : MPCQP_ERR_ORDER, h->keep_q.p, d.nZ);
        case MPCQP_GET_FVEC: return plain(h->keep_F.p ? 0 : MPCQP_ERR_ORDER, h->keep_F.p, d.nY);
        case MPCQP_GET_XHAT_MS: return plain(h->ms_X.p ? 0 : MPCQP_ERR_ORDER, h->ms_X.p, (size_t)d.nxh * d.Hp);
        case MPCQP_GET_MS_DEFECT: return plain(h->ms_defect.p ? 0 : MPCQP_ERR_ORDER, h->ms_defect.p, 1);
        case MPCQP_GET_AUDIT: return plain(h->audit.p ? 0 : MPCQP_ERR_ORDER, h->audit.p, 4);
        case MPCQP_GET_KF_COV: return plain(est_has_cov(h) ? 0 : MPCQP_ERR_ORDER, h->kf_P.p, (size_t)d.nxh * d.nxh);
        case MPCQP_GET_KF_GAIN: return plain(est_is_kf(h) ? 0 : MPCQP_ERR_ORDER, h->kf_K.p, (size_t)d.nxh * h->kf.nym);
        case MPCQP_GET_IM_XS: return plain(no_im, h->im_xs.p, h->im_nxs);
        case MPCQP_GET_IM_YS: return plain(no_im, h->im_ys.p, d.ny);
        case MPCQP_GET_IM_YHATS: return plain(no_im, h->im_Yhs.p, d.nY);
        case MPCQP_GET_EXPLICIT_LAW: {
            if (!h->ex_prepared || !h->ex_law) return MPCQP_ERR_ORDER;
            const int n = d.nZ, ncol = ex::law_ncol(d), kp = ex::law_kp(d);
            int rc = fetch(h->ex_law_z.p, ex::law_doubles(d, n), tmp);
            if (rc) return rc;
            for (size_t R = 0; R < B * n; ++R)
                for (int k = 0; k < ncol; ++k)
                    out[(R / n) * (size_t)n * ncol + (size_t)k * n + R % n] = tmp[ex::law_index(R, k, kp)];
            return MPCQP_OK;
        }
        case MPCQP_GET_MODEL_AHAT: case MPCQP_GET_MODEL_BU: case MPCQP_GET_MODEL_C: case MPCQP_GET_MODEL_BD: case MPCQP_GET_MODEL_DD:
        case MPCQP_GET_MODEL_DOP: {
            if (!h->have_model) return MPCQP_ERR_ORDER;
            const void* src = which == MPCQP_GET_MODEL_AHAT ? h->m.Ahat : which == MPCQP_GET_MODEL_BU ? h->m.Bu
                            : which == MPCQP_GET_MODEL_C ? h->m.C : which == MPCQP_GET_MODEL_BD ? h->m.Bd
                            : which == MPCQP_GET_MODEL_DD ? h->m.Dd : h->m.dop;
            const size_t n = which == MPCQP_GET_MODEL_AHAT ? (size_t)d.nxh * d.nxh : which == MPCQP_GET_MODEL_BU ? (size_t)d.nxh * d.nu
                           : which == MPCQP_GET_MODEL_C ? (size_t)d.ny * d.nxh : which == MPCQP_GET_MODEL_BD ? (size_t)d.nxh * d.nd
                           : which == MPCQP_GET_MODEL_DD ? (size_t)d.ny * d.nd : (size_t)d.nxh;
            if (!src) {                                     // (no measured disturbance: nothing to read; no f̂op - x̂op: zeros)
                if (which != MPCQP_GET_MODEL_DOP) return MPCQP_ERR_ARG;
                std::fill(out, out + B * n, 0.0);
                return MPCQP_OK;
            }
            return plain(0, src, n);
        }
        // K1's remaining tables, in their device layouts; the terminal ones exist once a finite x̂ bound had them built
        case MPCQP_GET_GDTAB: return plain(no_tables ? no_tables : d.nd == 0 ? MPCQP_ERR_ARG : 0, h->m.Gdtab, (size_t)d.Hp * d.ny * d.nd);
        case MPCQP_GET_XDTAB: case MPCQP_GET_EXHAT: case MPCQP_GET_KXHAT: case MPCQP_GET_BXHAT: {
            if (no_tables) return no_tables;
            if (!h->terminal_built) return MPCQP_ERR_ORDER;
            if (which == MPCQP_GET_XDTAB) return plain(d.nd == 0 ? MPCQP_ERR_ARG : 0, h->m.Xdtab, (size_t)d.Hp * d.nxh * d.nd);
            if (which == MPCQP_GET_EXHAT) return plain(0, h->m.exT, (size_t)d.Hc * d.nxh * d.nu);
            if (which == MPCQP_GET_KXHAT) return plain(0, h->m.kxT, (size_t)d.nxh * d.nxh);
            return plain(0, h->m.bxv, d.nxh);
        }
#ifdef MPCQP_PROFILE
        case 99:    /* per-phase cycle counters of profiling builds (-DMPCQP_PROFILE): (16,B) */
            return plain(h->prof.p ? 0 : MPCQP_ERR_ORDER, h->prof.p, 16);
#endif
        default:
            return MPCQP_ERR_ARG;
    }
}

// ---- ExplicitMPC: the entry points (the factor and the law build are explicit_refresh, above) --------------------------------

int mpcqp_explicit_prepare(mpcqp_handle h, int32_t with_law) {
    if (!h) return MPCQP_ERR_NULL;
    if (with_law & ~MPCQP_EXPLICIT_LAW) return MPCQP_ERR_ARG;
    if (h->est == EST_IM) return MPCQP_ERR_UNSUPPORTED;               // (the law has no Ŷs term)
    if (!h->have_model || !h->have_weights) return MPCQP_ERR_ORDER;
    if (explicit_constrained(h)) return MPCQP_ERR_ARG;          // "ExplicitMPC does not support constraints"
    const Dims& d = h->d;
    if (h->stage_only || !condensed_fits(d) || !ex::explicit_available()) return MPCQP_ERR_UNSUPPORTED;
    if (d.nZ > ex::EX_NMAX) return MPCQP_ERR_UNSUPPORTED;
    // (cannot happen: the step's LDS is below the condensed kernels' carve-up, explicit_launch.h)
    if (ex::step_lds_doubles(d) * sizeof(double) > ex::EX_LDS_MAX) return MPCQP_ERR_UNSUPPORTED;
    ON_DEVICE(h);
    const size_t B = d.B, n = d.nZ, sz = sizeof(double);
    const bool law = with_law & MPCQP_EXPLICIT_LAW;
    int rc = dev_alloc(h, h->ex_Hinv, B * ex::tri((int)n) * sz);
    if (!rc) rc = dev_alloc(h, h->ex_Lsum, B * n * sz);
    if (!rc) rc = dev_alloc(h, h->ex_st, B * sizeof(int32_t));
    if (!rc && law) {
        const size_t nz = ex::law_doubles(d, d.nZ) * sz, nu_ = ex::law_doubles(d, d.nu) * sz;
        const bool fresh = !h->ex_law_z.p;
        rc = dev_alloc(h, h->ex_law_z, nz);
        if (!rc) rc = dev_alloc(h, h->ex_law_u, nu_);
        if (!rc) rc = dev_alloc(h, h->ex_bx, B * d.nxh * sz);
        if (!rc) rc = dev_alloc(h, h->ex_blu, B * d.nu * sz);
        if (!rc) rc = dev_alloc(h, h->ex_bry, B * d.ny * sz);
        if (!rc && d.nd > 0) rc = dev_alloc(h, h->ex_bd0, B * d.nd * sz);
        if (!rc && d.nd > 0) rc = dev_alloc(h, h->ex_bdh, B * d.nD * sz);
        if (!rc) rc = dev_alloc(h, h->ex_bZ0, B * n * sz);
        if (!rc) rc = dev_alloc(h, h->ex_bZk, B * n * sz);
        if (!rc) rc = dev_alloc(h, h->ex_bu0, B * d.nu * sz);
        if (!rc) rc = dev_alloc(h, h->ex_bst, B * sizeof(int32_t));
        if (rc) return rc;
        // the padding of the tables -- the column of an odd count, the rows behind the batch -- is read and has to be finite: zeroed
        // where the tables are allocated and never written.  (Not again by a repeated prepare: a law call of the caller's may
        // be reading the tables; the build of explicit_refresh waits for it.)
        if (fresh) {
            HIPCHK(hipMemsetAsync(h->ex_law_z.p, 0, nz, h->stream));
            HIPCHK(hipMemsetAsync(h->ex_law_u.p, 0, nu_, h->stream));
        }
        h->ex_waves_z = ex::explicit_law_waves_for(h->device, (long)((B * n + WAVE - 1) / WAVE));
        h->ex_waves_u = ex::explicit_law_waves_for(h->device, (long)((B * d.nu + WAVE - 1) / WAVE));
    }
    if (rc) return rc;
    h->ex_prepared = true; h->ex_law = law;
    rc = explicit_refresh(h, h->stream);
    if (rc) { h->ex_prepared = false; return rc; }
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

int mpcqp_explicit_status(mpcqp_handle h, int32_t* out) {
    if (!h || !out) return MPCQP_ERR_NULL;
    if (h->est == EST_IM) return MPCQP_ERR_UNSUPPORTED;
    if (!h->ex_prepared || explicit_constrained(h)) return MPCQP_ERR_ORDER;
    ON_DEVICE(h);
    { int rc = explicit_current(h, h->stream); if (rc) return rc; }
    return read_back_i32(h, h->ex_st, h->d.B, out);
}

int mpcqp_explicit_step_device(mpcqp_handle h, const double* xhat0, const double* lastu0, const double* Ry,
                               const double* Ru, const double* d0, const double* Dhat0, double* Ztilde, double* u0,
                               int32_t* status, double* Yhat0, void* stream) {
    if (!h || !xhat0 || !lastu0 || !Ry || !Ztilde || !u0 || !status) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    if (d.nd > 0 && (!d0 || !Dhat0)) return MPCQP_ERR_NULL;
    if (h->est == EST_IM) return MPCQP_ERR_UNSUPPORTED;
    if (!h->ex_prepared || explicit_constrained(h)) return MPCQP_ERR_ORDER;
    ON_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    { int rc = explicit_current(h, st); if (rc) return rc; }
    ex::StepArgs a{};
    explicit_step_args(h, a, d.flags);
    a.xhat0 = xhat0; a.lastu0 = lastu0; a.Ry = Ry; a.Ru = Ru; a.d0 = d0; a.Dhat0 = Dhat0;
    a.Z = Ztilde; a.u0 = u0; a.status = status; a.Yhat0 = Yhat0;
    if (d.flags & MPCQP_FLAG_KEEP_QP) {
        int rc = dev_alloc(h, h->keep_q, (size_t)d.B * d.nZ * sizeof(double));
        if (!rc) rc = dev_alloc(h, h->keep_F, (size_t)d.B * d.nY * sizeof(double));
        if (rc) return rc;
        a.q_keep = (double*)h->keep_q.p;
        a.F_keep = (double*)h->keep_F.p;
    }
    HIPCHK(hipEventRecord(h->ev_s0, st));
    HIPCHK(ex::launch_explicit_step(a, st));
    HIPCHK(hipEventRecord(h->ev_s1, st));
    h->step_timed = true;
    return MPCQP_OK;
}

int mpcqp_explicit_law_device(mpcqp_handle h, const double* xhat0, const double* lastu0, const double* ry,
                              const double* d0, double* Ztilde, double* u0, int32_t* status, void* stream) {
    if (!h || !xhat0 || !lastu0 || !ry || !u0 || !status) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    if (d.nd > 0 && !d0) return MPCQP_ERR_NULL;
    if (h->est == EST_IM) return MPCQP_ERR_UNSUPPORTED;
    if (!h->ex_prepared || !h->ex_law || explicit_constrained(h)) return MPCQP_ERR_ORDER;
    ON_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    { int rc = explicit_current(h, st); if (rc) return rc; }
    ex::LawArgs a{};
    a.table = (const double*)(Ztilde ? h->ex_law_z.p : h->ex_law_u.p);
    a.xhat0 = xhat0; a.lastu0 = lastu0; a.ry = ry; a.d0 = d0;
    a.Z = Ztilde; a.u0 = u0; a.status = status; a.fstatus = (const int32_t*)h->ex_st.p;
    a.B = d.B; a.rows = Ztilde ? d.nZ : d.nu; a.nx = d.nxh; a.nu = d.nu; a.ny = d.ny; a.nd = d.nd; a.kp = ex::law_kp(d);
    a.nwaves = Ztilde ? h->ex_waves_z : h->ex_waves_u;
    HIPCHK(hipEventRecord(h->ev_s0, st));
    HIPCHK(ex::launch_explicit_law(a, st));
    HIPCHK(hipEventRecord(h->ev_s1, st));
    h->step_timed = true;
    return MPCQP_OK;
}

int mpcqp_explicit_step(mpcqp_handle h, const double* xhat0, const double* lastu0, const double* Ry, const double* Ru,
                        const double* d0, const double* Dhat0, double* Ztilde, double* u0, int32_t* status, double* Yhat0) {
    if (!h || !xhat0 || !lastu0 || !Ry || !Ztilde || !u0 || !status) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    if (d.nd > 0 && (!d0 || !Dhat0)) return MPCQP_ERR_NULL;
    if (h->est == EST_IM) return MPCQP_ERR_UNSUPPORTED;
    if (!h->ex_prepared || explicit_constrained(h)) return MPCQP_ERR_ORDER;
    ON_DEVICE(h);
    const size_t B = d.B, sz = sizeof(double);
    const size_t nry = (d.flags & MPCQP_FLAG_RY_CONSTANT) ? d.ny : d.nY;
    Staging s{h};
    const double* dx = s.in(h->s_x, xhat0, B * d.nxh);
    const double* dlu = s.in(h->s_lu, lastu0, B * d.nu);
    const double* dry = s.in(h->s_ry, Ry, B * nry);
    const double* dru = s.in(h->s_ru, Ru, B * d.nU);
    const double* dd0 = s.in(h->s_d0, d.nd > 0 ? d0 : nullptr, B * d.nd);
    const double* ddh = s.in(h->s_dh, d.nd > 0 ? Dhat0 : nullptr, B * d.nD);
    double* dZ = s.out<double>(h->s_Z, B * d.nZ);
    double* du0 = s.out<double>(h->s_u0, B * d.nu);
    int32_t* dst = s.out<int32_t>(h->s_st, B);
    double* dyh = Yhat0 ? s.out<double>(h->s_yh, B * d.nY) : nullptr;
    if (s.rc) return s.rc;
    s.rc = mpcqp_explicit_step_device(h, dx, dlu, dry, dru, dd0, ddh, dZ, du0, dst, dyh, h->stream);
    s.down(Ztilde, h->s_Z, B * d.nZ * sz);
    s.down(u0, h->s_u0, B * d.nu * sz);
    s.down(status, h->s_st, B * sizeof(int32_t));
    s.down(Yhat0, h->s_yh, B * d.nY * sz);
    return s.finish();
}

int mpcqp_explicit_law(mpcqp_handle h, const double* xhat0, const double* lastu0, const double* ry, const double* d0,
                       double* Ztilde, double* u0, int32_t* status) {
    if (!h || !xhat0 || !lastu0 || !ry || !u0 || !status) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    if (d.nd > 0 && !d0) return MPCQP_ERR_NULL;
    if (h->est == EST_IM) return MPCQP_ERR_UNSUPPORTED;
    if (!h->ex_prepared || !h->ex_law || explicit_constrained(h)) return MPCQP_ERR_ORDER;
    ON_DEVICE(h);
    const size_t B = d.B, sz = sizeof(double);
    Staging s{h};
    const double* dx = s.in(h->s_x, xhat0, B * d.nxh);
    const double* dlu = s.in(h->s_lu, lastu0, B * d.nu);
    const double* dry = s.in(h->s_ry, ry, B * d.ny);
    const double* dd0 = s.in(h->s_d0, d.nd > 0 ? d0 : nullptr, B * d.nd);
    double* dZ = Ztilde ? s.out<double>(h->s_Z, B * d.nZ) : nullptr;
    double* du0 = s.out<double>(h->s_u0, B * d.nu);
    int32_t* dst = s.out<int32_t>(h->s_st, B);
    if (s.rc) return s.rc;
    s.rc = mpcqp_explicit_law_device(h, dx, dlu, dry, dd0, dZ, du0, dst, h->stream);
    s.down(Ztilde, h->s_Z, B * d.nZ * sz);
    s.down(u0, h->s_u0, B * d.nu * sz);
    s.down(status, h->s_st, B * sizeof(int32_t));
    return s.finish();
}

int mpcqp_kf_set(mpcqp_handle h, const double* Khat, const int32_t* i_ym, int32_t nym) {
    if (!h || !Khat || !i_ym) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    if (nym < 1 || nym > d.ny) return MPCQP_ERR_DIMS;
    if (d.nxh > 64) return MPCQP_ERR_UNSUPPORTED;
    { int rc = check_iym(d, i_ym, nym); if (rc) return rc; }
    ON_DEVICE(h);
    int rc = upload(h, h->kf_K, Khat, (size_t)d.B * d.nxh * nym * sizeof(double));
    if (!rc) rc = upload(h, h->kf_iym, i_ym, (size_t)nym * sizeof(int32_t));
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    // (a Kalman handle again, on a gain of the caller's: the covariance kernel no longer runs, nothing to re-solve)
    adopt_estimator(h, EST_KF_GAIN, (const double*)h->kf_K.p, nym);
    return MPCQP_OK;
}

// every member of a (n,n,B) array symmetric up to 1e-12 of its largest entry (a NaN fails)
static bool kf_symmetric(const double* M, size_t B, int n) {
    for (size_t b = 0; b < B; ++b) {
        const double* A = M + b * (size_t)n * n;
        double big = 0.0;
        for (int i = 0; i < n * n; ++i) big = std::fmax(big, std::fabs(A[i]));
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < i; ++j)
                if (!(std::fabs(A[i + (size_t)n * j] - A[j + (size_t)n * i]) <= 1e-12 * big)) return false;
        if (!(big == big)) return false;
    }
    return true;
}

int mpcqp_kf_set_covariances(mpcqp_handle h, const double* Qhat, const double* Rhat, const double* P0,
                             const int32_t* i_ym, int32_t nym) {
    if (!h || !Qhat || !Rhat || !i_ym) return MPCQP_ERR_NULL;
    if (!P0 && h->est != EST_KF_TV) return MPCQP_ERR_NULL;        // (Q̂ / R̂ alone: only on a handle that carries a P̂)
    const Dims& d = h->d;
    if (nym < 1 || nym > d.ny) return MPCQP_ERR_DIMS;
    if (!P0 && nym != h->kf.nym) return MPCQP_ERR_DIMS;
    { int rc = check_iym(d, i_ym, nym); if (rc) return rc; }
    if (std::max(d.nxh, (int)nym) > mhe::NX_MAX || !kf::kf_cov_available()) return MPCQP_ERR_UNSUPPORTED;
    const size_t B = d.B, nn = (size_t)d.nxh * d.nxh, sz = sizeof(double);
    if (!kf_symmetric(Qhat, B, d.nxh) || !kf_symmetric(Rhat, B, nym) || (P0 && !kf_symmetric(P0, B, d.nxh))) return MPCQP_ERR_ARG;
    ON_DEVICE(h);
    int rc = upload(h, h->kf_Q, Qhat, B * nn * sz);
    if (!rc) rc = upload(h, h->kf_R, Rhat, B * (size_t)nym * nym * sz);
    if (!rc) rc = upload(h, h->kf_iym, i_ym, (size_t)nym * sizeof(int32_t));
    if (!rc && P0) rc = upload(h, h->kf_P, P0, B * nn * sz);
    if (!rc && P0) rc = dev_alloc(h, h->kf_K, B * (size_t)d.nxh * nym * sz);
    if (!rc && P0) rc = dev_alloc(h, h->kf_st, B * sizeof(int32_t));
    if (rc) return rc;
    if (P0) {
        HIPCHK(hipMemsetAsync(h->kf_K.p, 0, B * (size_t)d.nxh * nym * sz, h->stream));
        HIPCHK(hipMemsetAsync(h->kf_st.p, 0, B * sizeof(int32_t), h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    h->kf_NX = kf::kf_cov_columns_for(std::max(d.nxh, (int)nym));
    h->kf_waves = kf::kf_cov_waves_for(h->device, d.B, h->kf_NX);
    adopt_estimator(h, EST_KF_TV, (const double*)h->kf_K.p, nym);
    return MPCQP_OK;
}

// One Riccati solve of a handle in steady mode (kf_kernels.hip: k_kf_dare*) on the model that is resident now: the definite
// body for the whole batch, then (a library that has it) the square-root body, which reads and factors every Q̂ and solves
// again the estimators that the definite body left broken down or whose Q̂ is numerically singular (kf_dare_launch.h).
// A handle beyond 32 states or measured outputs (kf_dare_lds): one launch of the LDS-resident kernel, which refuses such
// estimators itself; path stays 0.  MPCQP_KF_DARE_TEAM = 1, 2, 4 picks another of its compiled teams (a test hook, read at
// every solve; anything else is ignored).
static int kf_dare_launch(mpcqp_handle h, hipStream_t st) {
    if (h->kf_dare_lds ? !kf::kf_dare_lds_available() : !kf::kf_dare_available()) return MPCQP_ERR_UNSUPPORTED;
    ON_DEVICE(h);
    const Dims& d = h->d;
    kf::DareArgs a{};
    a.Ahat = h->m.Ahat; a.C = h->m.C; a.i_ym = h->kf.i_ym;
    a.Q = (const double*)h->kf_Q.p; a.R = (const double*)h->kf_R.p;
    a.K = (double*)h->kf_K.p; a.P = (double*)h->kf_P.p;
    a.status = (int32_t*)h->kf_st.p; a.iters = (int32_t*)h->kf_it.p;
    a.B = d.B; a.nx = d.nxh; a.ny = d.ny; a.nym = h->kf.nym;
    a.NX = h->kf_NX; a.nwaves = h->kf_dare_waves;
    a.path = (int32_t*)h->kf_path.p;
    HIPCHK(hipMemsetAsync(h->kf_path.p, 0, (size_t)d.B * sizeof(int32_t), st));
    if (h->kf_dare_lds) {
        const char* e = getenv("MPCQP_KF_DARE_TEAM");
        h->kf_dare_team = kf::kf_dare_lds_team_for(e ? atoi(e) : 0);
        HIPCHK(kf::launch_kf_dare_lds(a, h->kf_dare_team, st));
        return MPCQP_OK;
    }
    HIPCHK(kf::launch_kf_dare(a, st));
    if (kf::kf_dare_psd_available()) HIPCHK(kf::launch_kf_dare_psd(a, st));
    return MPCQP_OK;
}

int mpcqp_kf_set_steady(mpcqp_handle h, const double* Qhat, const double* Rhat, const int32_t* i_ym, int32_t nym) {
    if (!h || !Qhat || !Rhat || !i_ym) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    if (nym < 1 || nym > d.ny) return MPCQP_ERR_DIMS;
    { int rc = check_iym(d, i_ym, nym); if (rc) return rc; }
    const int nmax = std::max(d.nxh, (int)nym);
    const bool lds = nmax > mhe::NX_MAX;              // beyond the row-lane kernels: operands in LDS, up to DARE_LDS_NMAX
    if (lds ? nmax > kf::DARE_LDS_NMAX || !kf::kf_dare_lds_available() : !kf::kf_dare_available()) return MPCQP_ERR_UNSUPPORTED;
    const size_t B = d.B, nn = (size_t)d.nxh * d.nxh, nk = (size_t)d.nxh * nym, sz = sizeof(double);
    if (!kf_symmetric(Qhat, B, d.nxh) || !kf_symmetric(Rhat, B, nym)) return MPCQP_ERR_ARG;
    if (!h->have_model) return MPCQP_ERR_ORDER;
    ON_DEVICE(h);
    int rc = upload(h, h->kf_Q, Qhat, B * nn * sz);
    if (!rc) rc = upload(h, h->kf_R, Rhat, B * (size_t)nym * nym * sz);
    if (!rc) rc = upload(h, h->kf_iym, i_ym, (size_t)nym * sizeof(int32_t));
    if (!rc) rc = dev_alloc(h, h->kf_P, B * nn * sz);
    if (!rc) rc = dev_alloc(h, h->kf_K, B * nk * sz);
    if (!rc) rc = dev_alloc(h, h->kf_st, B * sizeof(int32_t));
    if (!rc) rc = dev_alloc(h, h->kf_it, B * sizeof(int32_t));
    if (!rc) rc = dev_alloc(h, h->kf_path, B * sizeof(int32_t));
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(h->kf_P.p, 0, B * nn * sz, h->stream));
    HIPCHK(hipMemsetAsync(h->kf_K.p, 0, B * nk * sz, h->stream));
    HIPCHK(hipMemsetAsync(h->kf_st.p, 0, B * sizeof(int32_t), h->stream));
    HIPCHK(hipMemsetAsync(h->kf_it.p, 0, B * sizeof(int32_t), h->stream));
    h->kf_dare_lds = lds;
    h->kf_NX = lds ? kf::kf_dare_lds_order_for(nmax) : kf::kf_cov_columns_for(nmax);
    h->kf_dare_waves = lds ? kf::kf_dare_lds_waves_for(h->device, d.B, h->kf_NX) : kf::kf_dare_waves_for(h->device, d.B, h->kf_NX);
    h->kf_dare_team = lds ? kf::kf_dare_lds_team_for(0) : 0;
    adopt_estimator(h, EST_KF_STEADY, (const double*)h->kf_K.p, nym);
    return mpcqp_kf_solve_steady(h);
}

int mpcqp_kf_solve_steady_device(mpcqp_handle h, void* stream) {
    if (!h) return MPCQP_ERR_NULL;
    if (h->est != EST_KF_STEADY || !h->have_model) return MPCQP_ERR_ORDER;
    return kf_dare_launch(h, (hipStream_t)stream);
}

int mpcqp_kf_solve_steady(mpcqp_handle h) {
    if (!h) return MPCQP_ERR_NULL;
    int rc = mpcqp_kf_solve_steady_device(h, h->stream);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

int mpcqp_kf_steady_iters(mpcqp_handle h, int32_t* out) {
    if (!h || !out) return MPCQP_ERR_NULL;
    if (h->est != EST_KF_STEADY) return MPCQP_ERR_ORDER;
    return read_back_i32(h, h->kf_it, h->d.B, out);
}

int mpcqp_kf_steady_path(mpcqp_handle h, int32_t* out) {
    if (!h || !out) return MPCQP_ERR_NULL;
    if (h->est != EST_KF_STEADY) return MPCQP_ERR_ORDER;
    return read_back_i32(h, h->kf_path, h->d.B, out);
}

// One placement of a handle in pole mode (kf_place_kernels.hip: k_kf_place) on the model that is resident now.
static int kf_place_launch(mpcqp_handle h, hipStream_t st) {
    if (!kf::kf_place_available()) return MPCQP_ERR_UNSUPPORTED;
    ON_DEVICE(h);
    const Dims& d = h->d;
    kf::PlaceArgs a{};
    a.Ahat = h->m.Ahat; a.C = h->m.C; a.i_ym = h->kf.i_ym;
    a.poles = (const double*)h->kf_poles.p;
    a.K = (double*)h->kf_K.p;
    a.status = (int32_t*)h->kf_st.p; a.sweeps = (int32_t*)h->kf_it.p;
    a.B = d.B; a.nx = d.nxh; a.ny = d.ny; a.nym = h->kf.nym;
    a.cap = h->kf_place_cap;
    a.stored = kf::place_stored_for(a.nx, a.nym) ? 1 : 0;
    HIPCHK(kf::launch_kf_place(a, st));
    return MPCQP_OK;
}

int mpcqp_kf_set_poles(mpcqp_handle h, const double* poles, const int32_t* i_ym, int32_t nym) {
    if (!h || !poles || !i_ym) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    if (nym < 1 || nym > d.ny) return MPCQP_ERR_DIMS;
    { int rc = check_iym(d, i_ym, nym); if (rc) return rc; }
    if (std::max(d.nxh, (int)nym) > kf::PLACE_NMAX || !kf::kf_place_available()) return MPCQP_ERR_UNSUPPORTED;
    const size_t B = d.B, nk = (size_t)d.nxh * nym, sz = sizeof(double);
    for (size_t i = 0; i < B * d.nxh; ++i)
        if (!(std::fabs(poles[i]) < 1.0)) return MPCQP_ERR_ARG;      // inside the unit circle (luenberger.jl:108-115); a NaN fails
    if (!h->have_model) return MPCQP_ERR_ORDER;
    ON_DEVICE(h);
    int rc = upload(h, h->kf_poles, poles, B * d.nxh * sz);
    if (!rc) rc = upload(h, h->kf_iym, i_ym, (size_t)nym * sizeof(int32_t));
    if (!rc) rc = dev_alloc(h, h->kf_K, B * nk * sz);
    if (!rc) rc = dev_alloc(h, h->kf_st, B * sizeof(int32_t));
    if (!rc) rc = dev_alloc(h, h->kf_it, B * sizeof(int32_t));
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(h->kf_K.p, 0, B * nk * sz, h->stream));
    HIPCHK(hipMemsetAsync(h->kf_st.p, 0, B * sizeof(int32_t), h->stream));
    HIPCHK(hipMemsetAsync(h->kf_it.p, 0, B * sizeof(int32_t), h->stream));
    adopt_estimator(h, EST_KF_PLACE, (const double*)h->kf_K.p, nym);
    return mpcqp_kf_place(h);
}

int mpcqp_kf_place_device(mpcqp_handle h, void* stream) {
    if (!h) return MPCQP_ERR_NULL;
    if (h->est != EST_KF_PLACE || !h->have_model) return MPCQP_ERR_ORDER;
    return kf_place_launch(h, (hipStream_t)stream);
}

int mpcqp_kf_place(mpcqp_handle h) {
    if (!h) return MPCQP_ERR_NULL;
    int rc = mpcqp_kf_place_device(h, h->stream);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

int mpcqp_kf_set_place_cap(mpcqp_handle h, int32_t cap) {
    if (!h) return MPCQP_ERR_NULL;
    if (h->est != EST_KF_PLACE) return MPCQP_ERR_ORDER;
    if (cap < 0 || cap > kf::PLACE_CAP_MAX) return MPCQP_ERR_ARG;
    h->kf_place_cap = cap;
    return MPCQP_OK;
}

int mpcqp_kf_place_sweeps(mpcqp_handle h, int32_t* out) {
    if (!h || !out) return MPCQP_ERR_NULL;
    if (h->est != EST_KF_PLACE) return MPCQP_ERR_ORDER;
    return read_back_i32(h, h->kf_it, h->d.B, out);
}

int mpcqp_kf_set_state_covariance(mpcqp_handle h, const double* P) {
    if (!h || !P) return MPCQP_ERR_NULL;
    if (h->est != EST_KF_TV) return MPCQP_ERR_ORDER;
    const Dims& d = h->d;
    if (!kf_symmetric(P, d.B, d.nxh)) return MPCQP_ERR_ARG;
    ON_DEVICE(h);
    int rc = upload(h, h->kf_P, P, (size_t)d.B * d.nxh * d.nxh * sizeof(double));
    if (rc) return rc;
    HIPCHK(hipMemsetAsync(h->kf_st.p, 0, (size_t)d.B * sizeof(int32_t), h->stream));     // (a P̂ the caller vouches for)
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

int mpcqp_kf_status(mpcqp_handle h, int32_t* out) {
    if (!h || !out) return MPCQP_ERR_NULL;
    if (!est_has_cov(h) && h->est != EST_KF_PLACE) return MPCQP_ERR_ORDER;     // (a gain of the caller's has no status)
    return read_back_i32(h, h->kf_st, h->d.B, out);
}

int mpcqp_kf_lanes_per_estimator(mpcqp_handle h) {
    if (!h) return MPCQP_ERR_NULL;
    if (h->est == EST_KF_PLACE) return WAVE;       // (the placement: one member per wavefront at every size)
    if (h->est == EST_KF_STEADY && h->kf_dare_lds) return WAVE * h->kf_dare_team;     // (a team of wavefronts per estimator)
    return est_has_cov(h) ? kf::kf_cov_lanes_for(h->kf_NX) : 0;
}

int mpcqp_kf_correct_device(mpcqp_handle h, double* xhat0, const double* y0m, const double* d0, void* stream) {
    if (!h || !xhat0) return MPCQP_ERR_NULL;
    if (h->d.nd > 0 && !d0) return MPCQP_ERR_NULL;
    if (!h->have_model || !est_is_kf(h)) return MPCQP_ERR_ORDER;
    ON_DEVICE(h);
    if (!y0m)       // ym = nothing: every estimator misses; x̂0, P̂ and K̂ stay, a time-varying handle records status 1
        return h->est == EST_KF_TV ? kf_cov_launch(h, kf::COV_NO_YM, nullptr, (hipStream_t)stream) : MPCQP_OK;
    if (h->est == EST_KF_TV) { int rc = kf_cov_launch(h, kf::COV_CORRECT, y0m, (hipStream_t)stream); if (rc) return rc; }
    HIPCHK(launch_kf_correct(h->d, h->m, h->kf, xhat0, y0m, d0, (hipStream_t)stream));
    return MPCQP_OK;
}

int mpcqp_kf_predict_device(mpcqp_handle h, double* xhat0, const double* u0, const double* d0, void* stream) {
    if (!h || !xhat0 || !u0) return MPCQP_ERR_NULL;
    if (h->d.nd > 0 && !d0) return MPCQP_ERR_NULL;
    if (!h->have_model) return MPCQP_ERR_ORDER;
    if (h->d.nxh > 64) return MPCQP_ERR_UNSUPPORTED;
    ON_DEVICE(h);
    HIPCHK(launch_kf_predict(h->d, h->m, xhat0, u0, d0, (hipStream_t)stream));
    if (h->est == EST_KF_TV) { int rc = kf_cov_launch(h, kf::COV_PREDICT, nullptr, (hipStream_t)stream); if (rc) return rc; }
    return MPCQP_OK;
}

int mpcqp_kf_set_direct(mpcqp_handle h, int32_t direct) {
    if (!h) return MPCQP_ERR_NULL;
    if (direct != 0 && direct != 1) return MPCQP_ERR_ARG;
    if (h->est == EST_IM && direct == 0) return MPCQP_ERR_ARG;        // (InternalModel: always the filter form)
    h->kf_direct = direct;
    return MPCQP_OK;
}

// updatestate! of a direct = false estimator (kalman.jl:276-281, 520-525): correction, then prediction.  One covariance
// launch (mode 3: P̂(k|k) stays in registers, bit-equal to modes 1 and 2 in turn), then the two state kernels.
int mpcqp_kf_update_device(mpcqp_handle h, double* xhat0, const double* u0, const double* y0m, const double* d0, void* stream) {
    if (!h || !xhat0 || !u0) return MPCQP_ERR_NULL;
    if (h->d.nd > 0 && !d0) return MPCQP_ERR_NULL;
    if (!h->have_model || !est_is_kf(h)) return MPCQP_ERR_ORDER;
    if (h->d.nxh > 64) return MPCQP_ERR_UNSUPPORTED;
    ON_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    if (h->est == EST_KF_TV) {
        int rc = kf_cov_launch(h, (y0m ? kf::COV_CORRECT : kf::COV_NO_YM) | kf::COV_PREDICT, y0m, st);
        if (rc) return rc;
    }
    if (y0m) HIPCHK(launch_kf_correct(h->d, h->m, h->kf, xhat0, y0m, d0, st));
    HIPCHK(launch_kf_predict(h->d, h->m, xhat0, u0, d0, st));
    return MPCQP_OK;
}

int mpcqp_kf_update(mpcqp_handle h, double* xhat0, const double* u0, const double* y0m, const double* d0) {
    if (!h || !xhat0 || !u0) return MPCQP_ERR_NULL;
    if (!h->have_model || !est_is_kf(h)) return MPCQP_ERR_ORDER;
    const Dims& d = h->d;
    if (d.nd > 0 && !d0) return MPCQP_ERR_NULL;
    ON_DEVICE(h);
    const size_t B = d.B;
    Staging s{h};
    double* dx = s.in(h->kf_x, xhat0, B * d.nxh);
    const double* du = s.in(h->kf_u, u0, B * d.nu);
    const double* dy = s.in(h->kf_y, y0m, B * (size_t)h->kf.nym);
    const double* dd = s.in(h->kf_d, d.nd > 0 ? d0 : nullptr, B * d.nd);
    if (s.rc) return s.rc;
    s.rc = mpcqp_kf_update_device(h, dx, du, dy, dd, h->stream);
    s.down(xhat0, h->kf_x, B * d.nxh * sizeof(double));
    return s.finish();
}

static int kf_host(mpcqp_handle h, double* xhat0, const double* a, size_t na, const double* d0, bool correct) {
    if (!h || !xhat0 || (!a && !correct)) return MPCQP_ERR_NULL;      // (a correction without y0m: every estimator misses)
    const Dims& d = h->d;
    if (d.nd > 0 && !d0) return MPCQP_ERR_NULL;
    ON_DEVICE(h);
    const size_t B = d.B;
    Staging s{h};
    double* dx = s.in(h->kf_x, xhat0, B * d.nxh);
    const double* da = s.in(correct ? h->kf_y : h->kf_u, a, B * na);
    const double* dd = s.in(h->kf_d, d.nd > 0 ? d0 : nullptr, B * d.nd);
    if (s.rc) return s.rc;
    s.rc = correct ? mpcqp_kf_correct_device(h, dx, da, dd, h->stream) : mpcqp_kf_predict_device(h, dx, da, dd, h->stream);
    s.down(xhat0, h->kf_x, B * d.nxh * sizeof(double));
    return s.finish();
}

int mpcqp_kf_correct(mpcqp_handle h, double* xhat0, const double* y0m, const double* d0) {
    if (h && !est_is_kf(h)) return MPCQP_ERR_ORDER;
    return kf_host(h, xhat0, y0m, h ? (size_t)h->kf.nym : 0, d0, true);
}

int mpcqp_kf_predict(mpcqp_handle h, double* xhat0, const double* u0, const double* d0) {
    return kf_host(h, xhat0, u0, h ? (size_t)h->d.nu : 0, d0, false);
}

// ---- InternalModel: the entry points (im_args and im_refresh are above) --------------------------------------------------------

int mpcqp_im_set(mpcqp_handle h, int32_t nxs, const double* As, const double* Bs, const double* Cs, const double* Ds,
                 const int32_t* i_ym, int32_t nym) {
    if (!h || !i_ym) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    if (nym < 1 || nym > d.ny) return MPCQP_ERR_DIMS;
    const int given = (As != nullptr) + (Bs != nullptr) + (Cs != nullptr) + (Ds != nullptr);
    if (given != 0 && given != 4) return MPCQP_ERR_ARG;
    if (given == 0) nxs = nym;      // the default: the identity in all four
    if (nxs < 1) return MPCQP_ERR_ARG;
    { int rc = check_iym(d, i_ym, nym); if (rc) return rc; }
    if (!im::im_available() || !im::dims_ok(d.nxh, d.nu, d.ny, d.nd, nym, nxs)) return MPCQP_ERR_UNSUPPORTED;
    if (h->in_multi || h->ex_prepared || d.nW > 0 || uses_stage_kernel(h)) return MPCQP_ERR_UNSUPPORTED;
    ON_DEVICE(h);
    const size_t B = d.B, sz = sizeof(double), n = (size_t)nxs, m = (size_t)nym;
    std::vector<double> eye;
    if (given == 0) {
        eye.assign(B * m * m, 0.0);
        for (size_t b = 0; b < B; ++b)
            for (size_t i = 0; i < m; ++i) eye[b * m * m + i * m + i] = 1.0;
        As = Bs = Cs = Ds = eye.data();
    }
    // (a step enqueued on a caller's stream may still read x̂s, Ŷs or B_eff: upload() orders the copies behind it, and the
    //  set-up kernel follows them on the same stream)
    int rc = upload(h, h->im_As, As, B * n * n * sz);
    if (!rc) rc = upload(h, h->im_Bs, Bs, B * n * m * sz);
    if (!rc) rc = upload(h, h->im_Cs, Cs, B * m * n * sz);
    if (!rc) rc = upload(h, h->im_Ds, Ds, B * m * m * sz);
    if (!rc) rc = upload(h, h->kf_iym, i_ym, m * sizeof(int32_t));
    if (!rc) rc = dev_alloc(h, h->im_Ahs, B * n * n * sz);
    if (!rc) rc = dev_alloc(h, h->im_Bhs, B * n * m * sz);
    if (!rc) rc = dev_alloc(h, h->im_xs, B * n * sz);
    if (!rc) rc = dev_alloc(h, h->im_z, B * n * sz);
    if (!rc) rc = dev_alloc(h, h->im_ys, B * d.ny * sz);
    if (!rc) rc = dev_alloc(h, h->im_Yhs, B * d.nY * sz);
    if (!rc) rc = dev_alloc(h, h->im_Beff, B * d.nY * sz);
    if (!rc) rc = dev_alloc(h, h->im_st, B * sizeof(int32_t));
    if (rc) {       // (its buffers may be half replaced: an InternalModel is dropped, any other estimator is left alone)
        if (h->est == EST_IM) h->est = EST_NONE;
        return rc;
    }
    h->im_nxs = nxs;
    adopt_estimator(h, EST_IM, nullptr, nym);       // (replaces a Kalman filter or an attached MovingHorizonEstimator)
    h->kf_direct = 1;
    im::ImArgs a{};
    im_args(h, a);
    const hipError_t e = im::launch_im(a, im::IM_SETUP, h->stream);
    if (e != hipSuccess) { h->est = EST_NONE; HIPCHK(e); }
    HIPCHK(hipStreamSynchronize(h->stream));
    return MPCQP_OK;
}

int mpcqp_im_status(mpcqp_handle h, int32_t* out) {
    if (!h || !out) return MPCQP_ERR_NULL;
    if (h->est != EST_IM) return MPCQP_ERR_ORDER;
    return read_back_i32(h, h->im_st, h->d.B, out);
}

int mpcqp_im_correct_device(mpcqp_handle h, const double* xhat0, const double* y0m, const double* d0, void* stream) {
    if (!h || !xhat0 || !y0m) return MPCQP_ERR_NULL;
    if (h->d.nd > 0 && !d0) return MPCQP_ERR_NULL;
    if (!h->have_model || h->est != EST_IM) return MPCQP_ERR_ORDER;
    ON_DEVICE(h);
    im::ImArgs a{};
    im_args(h, a);
    a.xhat0 = const_cast<double*>(xhat0); a.y0m = y0m; a.d0 = h->d.nd > 0 ? d0 : nullptr;
    HIPCHK(im::launch_im(a, im::IM_CORRECT, (hipStream_t)stream));
    return MPCQP_OK;
}

int mpcqp_im_update_device(mpcqp_handle h, double* xhat0, const double* u0, const double* d0, void* stream) {
    if (!h || !xhat0 || !u0) return MPCQP_ERR_NULL;
    if (h->d.nd > 0 && !d0) return MPCQP_ERR_NULL;
    if (!h->have_model || h->est != EST_IM) return MPCQP_ERR_ORDER;
    ON_DEVICE(h);
    im::ImArgs a{};
    im_args(h, a);
    a.xhat0 = xhat0; a.u0 = u0; a.d0 = h->d.nd > 0 ? d0 : nullptr;
    HIPCHK(im::launch_im(a, im::IM_UPDATE, (hipStream_t)stream));
    return MPCQP_OK;
}

static int im_host(mpcqp_handle h, double* xhat0, const double* v, const double* d0, bool correct) {
    if (!h || !xhat0 || !v) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    if (d.nd > 0 && !d0) return MPCQP_ERR_NULL;
    if (!h->have_model || h->est != EST_IM) return MPCQP_ERR_ORDER;
    ON_DEVICE(h);
    const size_t B = d.B;
    Staging s{h};
    double* dx = s.in(h->kf_x, xhat0, B * d.nxh);
    const double* dv = s.in(correct ? h->kf_y : h->kf_u, v, B * (size_t)(correct ? h->kf.nym : d.nu));
    const double* dd = s.in(h->kf_d, d.nd > 0 ? d0 : nullptr, B * d.nd);
    if (s.rc) return s.rc;
    s.rc = correct ? mpcqp_im_correct_device(h, dx, dv, dd, h->stream) : mpcqp_im_update_device(h, dx, dv, dd, h->stream);
    s.down(correct ? nullptr : xhat0, h->kf_x, B * d.nxh * sizeof(double));      // (the correction leaves x̂0 as it is)
    return s.finish();
}

int mpcqp_im_correct(mpcqp_handle h, const double* xhat0, const double* y0m, const double* d0) {
    return im_host(h, const_cast<double*>(xhat0), y0m, d0, true);
}

int mpcqp_im_update(mpcqp_handle h, double* xhat0, const double* u0, const double* d0) { return im_host(h, xhat0, u0, d0, false); }

// ---- LinMPC(MovingHorizonEstimator): attachment, and the estimator half of initstate! (include/mpcqp_mhe.h) ------------------

int mpcqp_mhe_attach(mpcqp_handle h, mpcqp_mhe e, const int32_t* i_ym, int32_t nym) {
    if (!h) return MPCQP_ERR_NULL;
    if (!e) {       // detach only: an attachment goes, any other estimator stays
        if (h->est == EST_MHE) { h->est = EST_NONE; h->mhe = nullptr; }
        return MPCQP_OK;
    }
    if (!i_ym) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    mpcqp_mhe_dims ed{};
    { int rc = mpcqp_mhe_get_dims(e, &ed); if (rc) return rc; }
    if (ed.batch != d.B || ed.nxhat != d.nxh || ed.nu != d.nu || ed.nd != d.nd || ed.nym != nym || ed.device != h->device ||
        nym < 1 || nym > d.ny)
        return MPCQP_ERR_DIMS;
    { int rc = check_iym(d, i_ym, nym); if (rc) return rc; }
    ON_DEVICE(h);
    int rc = upload(h, h->kf_iym, i_ym, (size_t)nym * sizeof(int32_t));
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(h->stream));
    adopt_estimator(h, EST_MHE, nullptr, nym);      // (the attachment replaces a Kalman filter or an InternalModel)
    h->mhe = e;
    return MPCQP_OK;
}

int mpcqp_est_initstate_device(mpcqp_handle h, double* xhat0, const double* u0, const double* y0m, const double* d0,
                               int32_t* status, void* stream) {
    if (!h || !xhat0 || !u0 || !y0m || !status) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    if (d.nd > 0 && !d0) return MPCQP_ERR_NULL;
    if (h->est == EST_IM) {           // init_estimate! of the InternalModel: x̂d, ŷs and x̂s (k_im_init)
        if (!h->have_model) return MPCQP_ERR_ORDER;
        ON_DEVICE(h);
        im::ImArgs a{};
        im_args(h, a);
        a.u0 = u0; a.y0m = y0m; a.d0 = d.nd > 0 ? d0 : nullptr; a.xhat0 = xhat0; a.init_status = status;
        HIPCHK(im::launch_im(a, im::IM_INIT, (hipStream_t)stream));
        return MPCQP_OK;
    }
    if (!est_any(h) || !h->have_model) return MPCQP_ERR_ORDER;
    if (std::max(d.nxh, h->kf.nym) > est::EST_INIT_NMAX || !est::est_init_available()) return MPCQP_ERR_UNSUPPORTED;
    ON_DEVICE(h);
    est::InitArgs a{};
    a.Ahat = h->m.Ahat; a.Bu = h->m.Bu; a.C = h->m.C; a.Bd = d.nd > 0 ? h->m.Bd : nullptr; a.Dd = d.nd > 0 ? h->m.Dd : nullptr;
    a.fx = h->m.dop; a.i_ym = h->kf.i_ym;
    a.B = d.B; a.nx = d.nxh; a.nu = d.nu; a.ny = d.ny; a.nd = d.nd; a.nym = h->kf.nym;
    a.u0 = u0; a.y0m = y0m; a.d0 = d.nd > 0 ? d0 : nullptr; a.xhat0 = xhat0; a.status = status;
    HIPCHK(est::launch_est_init(a, (hipStream_t)stream));
    return MPCQP_OK;
}

int mpcqp_est_initstate(mpcqp_handle h, double* xhat0, const double* u0, const double* y0m, const double* d0, int32_t* status) {
    if (!h || !xhat0 || !u0 || !y0m || !status) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    if (d.nd > 0 && !d0) return MPCQP_ERR_NULL;
    if (!est_any(h) || !h->have_model) return MPCQP_ERR_ORDER;
    ON_DEVICE(h);
    const size_t B = d.B;
    Staging s{h};
    double* dx = s.in(h->ei_x, xhat0, B * d.nxh);
    const double* du = s.in(h->ei_u, u0, B * d.nu);
    const double* dy = s.in(h->ei_y, y0m, B * (size_t)h->kf.nym);
    const double* dd = s.in(h->ei_d, d.nd > 0 ? d0 : nullptr, B * d.nd);
    int32_t* dst = s.out<int32_t>(h->ei_st, B);
    if (s.rc) return s.rc;
    s.rc = mpcqp_est_initstate_device(h, dx, du, dy, dd, dst, h->stream);
    s.down(xhat0, h->ei_x, B * d.nxh * sizeof(double));
    s.down(status, h->ei_st, B * sizeof(int32_t));
    return s.finish();
}

// ---- sim!: the closed loop of the whole batch, plant included (include/mpcqp.h; kernel: sim_bodies.h) ----------------------

int mpcqp_sim_set_plant(mpcqp_handle h, int32_t nxp, const double* A, const double* Bu, const double* C, const double* Bd,
                        const double* Dd, const double* fx) {
    if (!h || !A || !Bu || !C) return MPCQP_ERR_NULL;
    const Dims& d = h->d;
    if (nxp < 1) return MPCQP_ERR_ARG;
    if (nxp > sim::SIM_NMAX || d.nu > sim::SIM_NMAX || d.ny > sim::SIM_NMAX || d.nd > sim::SIM_NMAX || !sim::sim_available())
        return MPCQP_ERR_UNSUPPORTED;
    ON_DEVICE(h);
    const size_t B = d.B, n = nxp, sz = sizeof(double);
    int rc = upload(h, h->sp_A, A, B * n * n * sz);
    if (!rc) rc = upload(h, h->sp_Bu, Bu, B * n * d.nu * sz);
    if (!rc) rc = upload(h, h->sp_C, C, B * d.ny * n * sz);
    if (!rc && Bd && d.nd > 0) rc = upload(h, h->sp_Bd, Bd, B * n * d.nd * sz);
    if (!rc && Dd && d.nd > 0) rc = upload(h, h->sp_Dd, Dd, B * d.ny * d.nd * sz);
    if (!rc && fx) rc = upload(h, h->sp_fx, fx, B * n * sz);
    if (rc) { h->have_plant = false; return rc; }
    HIPCHK(hipStreamSynchronize(h->stream));
    h->sim_nxp = nxp;
    h->sp_has_Bd = Bd && d.nd > 0; h->sp_has_Dd = Dd && d.nd > 0; h->sp_has_fx = fx != nullptr;
    h->have_plant = true;
    return MPCQP_OK;
}

// the handle's side of the fused path's eligibility (include/mpcqp.h); the call's side is sim_fused below
static bool sim_fused_handle(mpcqp_handle h) {
    if (!sim::sim_fused_available() || !h->have_plant || !est_is_kf(h) || h->est == EST_KF_TV) return false;
    if (!h->have_model || !h->have_weights || !h->ex_prepared || !h->ex_law || explicit_constrained(h)) return false;
    const Dims& d = h->d;
    sim::PlantArgs p{};
    p.nxh = d.nxh; p.nxp = h->sim_nxp; p.nu = d.nu; p.ny = d.ny; p.nd = d.nd; p.nym = h->kf.nym;
    return sim::fused_dims_ok(p) && sim::fused_lds_doubles(p, ex::law_ncol(d)) * sizeof(double) <= 160 * 1024;
}
static bool sim_fused(mpcqp_handle h, const mpcqp_sim_io* io) {
    return sim_fused_handle(h) && !io->Ru && !(io->flags & (MPCQP_SIM_FLAG_RY_PER_PERIOD | MPCQP_SIM_FLAG_NO_FUSE));
}

int mpcqp_sim_path(mpcqp_handle h) {
    if (!h) return MPCQP_ERR_NULL;
    return sim_fused_handle(h) ? MPCQP_SIM_PATH_FUSED : MPCQP_SIM_PATH_PERIOD;
}

// which controller call a period of the simulation makes
enum { SIM_CTRL_NONE = 0, SIM_CTRL_STEP, SIM_CTRL_EXPLICIT_STEP, SIM_CTRL_EXPLICIT_LAW };
static int sim_controller(mpcqp_handle h, const mpcqp_sim_io* io) {
    if (!h->have_model || !h->have_weights) return SIM_CTRL_NONE;
    if (h->ex_prepared) {
        if (explicit_constrained(h)) return SIM_CTRL_NONE;
        return (h->ex_law && !io->Ru) ? SIM_CTRL_EXPLICIT_LAW : SIM_CTRL_EXPLICIT_STEP;
    }
    return SIM_CTRL_STEP;
}

// the checks of both entry points, nothing enqueued
static int sim_check(mpcqp_handle h, const mpcqp_sim_io* io) {
    if (!h || !io) return MPCQP_ERR_NULL;
    if (io->N <= 0 || (io->flags & ~(MPCQP_SIM_FLAG_RY_PER_PERIOD | MPCQP_SIM_FLAG_NO_FUSE))) return MPCQP_ERR_ARG;
    const int ctrl = sim_controller(h, io);
    if (!h->have_plant || !est_any(h) || ctrl == SIM_CTRL_NONE) return MPCQP_ERR_ORDER;
    if (h->est == EST_IM && (ctrl != SIM_CTRL_STEP || uses_stage_kernel(h) || h->d.nW > 0)) return MPCQP_ERR_UNSUPPORTED;
    if (!io->ry || !io->x0 || !io->xhat0 || !io->lastu0 || (h->d.nd > 0 && !io->d)) return MPCQP_ERR_NULL;
    if (!io->Ztilde && ctrl != SIM_CTRL_EXPLICIT_LAW) return MPCQP_ERR_NULL;
    if ((io->sigma_u && !io->w_u) || (io->sigma_y && !io->w_y) || (io->sigma_x && !io->w_x) ||
        (h->d.nd > 0 && io->sigma_d && !io->w_d))
        return MPCQP_ERR_NULL;
    return MPCQP_OK;
}

int mpcqp_sim_device(mpcqp_handle h, const mpcqp_sim_io* io_in, void* stream) {
    { int rc = sim_check(h, io_in); if (rc) return rc; }
    const Dims& d = h->d;
    mpcqp_sim_io io_ = *io_in;
    if (d.nd == 0) { io_.d = io_.d_step = io_.sigma_d = io_.w_d = nullptr; io_.D = nullptr; }     // (no such channel)
    const mpcqp_sim_io* io = &io_;
    ON_DEVICE(h);
    hipStream_t st = (hipStream_t)stream;
    const int ctrl = sim_controller(h, io), N = io->N;
    const bool per_period = io->flags & MPCQP_SIM_FLAG_RY_PER_PERIOD;
    const bool horizon = ctrl != SIM_CTRL_EXPLICIT_LAW && d.nd > 0;      // the step kernels read D̂0 = repeat(d0, Hp)
    const size_t B = d.B, sz = sizeof(double);
    int rc = dev_alloc(h, h->sim_u0, B * d.nu * sz);
    if (!rc) rc = dev_alloc(h, h->sim_st, B * sizeof(int32_t));
    if (!rc) rc = dev_alloc(h, h->sim_it, B * sizeof(int32_t));
    if (!rc) rc = dev_alloc(h, h->sim_y0m, B * (size_t)h->kf.nym * sz);
    if (!rc && d.nd > 0) rc = dev_alloc(h, h->sim_d0, B * d.nd * sz);
    if (!rc && per_period) rc = dev_alloc(h, h->sim_ry, B * d.ny * sz);
    if (!rc && horizon) rc = dev_alloc(h, h->sim_dh, B * d.nD * sz);
    if (!rc && h->mhe) rc = dev_alloc(h, h->sim_est, B * (size_t)N * sizeof(int32_t));
    if (rc) return rc;
    // an attached MovingHorizonEstimator: the controller, the plant kernel and the X̂ / Ŷ records read its x̂0 in place
    mpcqp_mhe const est = h->mhe;
    double* const xh = est ? (double*)mpcqp_mhe_device_ptr(est, MPCQP_MHE_XHAT0) : io->xhat0;
    const int32_t* const est_st = est ? (const int32_t*)mpcqp_mhe_device_ptr(est, MPCQP_MHE_STATUS) : nullptr;
    h->sim_est_N = 0;
    double* u0 = (double*)h->sim_u0.p;
    int32_t *cst = (int32_t*)h->sim_st.p, *cit = (int32_t*)h->sim_it.p;
    double* y0m = (double*)h->sim_y0m.p;
    double* d0 = d.nd > 0 ? (double*)h->sim_d0.p : nullptr;
    double* Dh = horizon ? (double*)h->sim_dh.p : nullptr;
    const double* ry = per_period ? (const double*)h->sim_ry.p : io->ry;

    sim::PlantArgs a{};
    a.A = (const double*)h->sp_A.p; a.Bu = (const double*)h->sp_Bu.p; a.C = (const double*)h->sp_C.p;
    a.Bd = h->sp_has_Bd ? (const double*)h->sp_Bd.p : nullptr; a.Dd = h->sp_has_Dd ? (const double*)h->sp_Dd.p : nullptr;
    a.fx = h->sp_has_fx ? (const double*)h->sp_fx.p : nullptr;
    a.Chat = h->m.C; a.Dhd = d.nd > 0 ? h->m.Dd : nullptr; a.i_ym = h->kf.i_ym;
    a.yhs = h->est == EST_IM ? (const double*)h->im_ys.p : nullptr;       // evaloutput of the InternalModel: + ŷs
    a.B = d.B; a.nxp = h->sim_nxp; a.nu = d.nu; a.ny = d.ny; a.nd = d.nd; a.nym = h->kf.nym; a.nxh = d.nxh; a.Hp = d.Hp; a.N = N;
    a.G = sim::group_lanes(a.nxp, a.nu, a.ny, a.nd, a.nym);
    a.ry = io->ry; a.d = io->d; a.ry_per_period = per_period ? 1 : 0;
    a.u_step = io->u_step; a.y_step = io->y_step; a.d_step = io->d_step;
    a.su = io->sigma_u; a.sy = io->sigma_y; a.sd = io->sigma_d; a.sx = io->sigma_x;
    a.wu = io->w_u; a.wy = io->w_y; a.wd = io->w_d; a.wx = io->w_x;
    a.x = io->x0; a.xhat = xh; a.lastu0 = io->lastu0; a.u0 = u0; a.st = cst;
    a.d0 = d0; a.y0m = y0m; a.ry_cur = per_period ? (double*)h->sim_ry.p : nullptr; a.Dhat0 = Dh;
    a.Y = io->Y; a.X = io->X; a.D = io->D; a.Xhat = io->Xhat; a.Yhat = io->Yhat; a.U = io->U; a.Ud = io->Ud; a.status = io->status;
    if (sim_fused(h, io)) {         // the whole loop in one launch (k_sim_explicit); Z̃ is not computed on this path
        { int rc2 = explicit_current(h, st); if (rc2) return rc2; }
        sim::FusedArgs f{};
        f.p = a;
        f.p.i_est = f.p.i_tail = f.p.i_head = -1;
        f.Ahat = h->m.Ahat; f.Bhu = h->m.Bu; f.Bhd = d.nd > 0 ? h->m.Bd : nullptr; f.dop = h->m.dop;
        f.Khat = h->kf.Khat; f.law = (const double*)h->ex_law_u.p; f.fstatus = (const int32_t*)h->ex_st.p;
        f.kp = ex::law_kp(d); f.ncol = ex::law_ncol(d); f.direct = h->kf_direct;
        HIPCHK(hipEventRecord(h->ev_s0, st));
        HIPCHK(sim::launch_sim_explicit(f, st));
        HIPCHK(hipEventRecord(h->ev_s1, st));
        h->step_timed = true;
        return MPCQP_OK;
    }
    auto plant = [&](int i_est, int i_tail, int i_head) {
        sim::PlantArgs p = a;
        p.i_est = i_est; p.i_tail = i_tail; p.i_head = i_head;
        return sim::launch_sim_plant(p, st);
    };

    // the step reads the set point of the period as (ny,B), whatever the handle's flag says about the caller's own steps
    // (and r̂e(k) of the custom rows is that set point: no mpcqp_set_current_setpoint of an earlier period)
    struct FlagGuard {
        mpcqp_handle h; uint32_t keep; const double* ry_now;
        ~FlagGuard() { h->d.flags = keep; h->m.ry_now = ry_now; }
    } flag_guard{h, d.flags, h->m.ry_now};
    h->d.flags |= MPCQP_FLAG_RY_CONSTANT;
    h->m.ry_now = nullptr;

    if (est) { rc = mpcqp_mhe_set_state_stream(est, io->xhat0, stream); if (rc) return rc; }     // setstate!: x̂0 and nothing else
    HIPCHK(plant(-1, -1, 0));
    for (int i = 0; i < N; ++i) {
        if (est) { rc = mpcqp_mhe_prepare_stream(est, y0m, d0, stream); if (rc) return rc; }      // (predictor form: nothing)
        else if (h->est == EST_IM) { rc = mpcqp_im_correct_device(h, io->xhat0, y0m, d0, stream); if (rc) return rc; }
        else if (h->kf_direct) { rc = mpcqp_kf_correct_device(h, io->xhat0, y0m, d0, stream); if (rc) return rc; }
        if (io->Xhat || io->Yhat) HIPCHK(plant(i, -1, -1));
        switch (ctrl) {
            case SIM_CTRL_EXPLICIT_LAW:
                rc = mpcqp_explicit_law_device(h, xh, io->lastu0, ry, d0, io->Ztilde, u0, cst, stream);
                break;
            case SIM_CTRL_EXPLICIT_STEP:
                rc = mpcqp_explicit_step_device(h, xh, io->lastu0, ry, io->Ru, d0, Dh, io->Ztilde, u0, cst, nullptr, stream);
                break;
            default:
                rc = mpcqp_step_device(h, xh, io->lastu0, ry, io->Ru, d0, Dh, io->Ztilde, u0, cst, cit, nullptr, stream);
        }
        if (rc) return rc;
        if (est) {
            rc = mpcqp_mhe_update_stream(est, u0, y0m, d0, stream);
            if (rc) return rc;
            // the estimator's status of this period (the solve of preparestate! or, predictor form, of updatestate!)
            HIPCHK(hipMemcpyAsync((int32_t*)h->sim_est.p + (size_t)i * B, est_st, B * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        } else if (h->est == EST_IM) {
            rc = mpcqp_im_update_device(h, io->xhat0, u0, d0, stream);
            if (rc) return rc;
        } else {
            rc = h->kf_direct ? mpcqp_kf_predict_device(h, io->xhat0, u0, d0, stream)
                              : mpcqp_kf_update_device(h, io->xhat0, u0, y0m, d0, stream);
            if (rc) return rc;
        }
        HIPCHK(plant(-1, i, i + 1 < N ? i + 1 : -1));
    }
    if (est) {
        HIPCHK(hipMemcpyAsync(io->xhat0, xh, B * d.nxh * sz, hipMemcpyDeviceToDevice, st));
        h->sim_est_N = N;
    }
    return MPCQP_OK;
}

int mpcqp_sim_est_status(mpcqp_handle h, int32_t* out, int32_t N) {
    if (!h || !out) return MPCQP_ERR_NULL;
    if (h->sim_est_N < 1 || !h->sim_est.p) return MPCQP_ERR_ORDER;
    if (N < 1 || N > h->sim_est_N) return MPCQP_ERR_ARG;
    ON_DEVICE(h);
    return read_back_i32(h, h->sim_est, (size_t)N * h->d.B, out);
}

int mpcqp_sim(mpcqp_handle h, const mpcqp_sim_io* io) {
    { int rc = sim_check(h, io); if (rc) return rc; }
    const Dims& d = h->d;
    ON_DEVICE(h);
    const size_t B = d.B, N = (size_t)io->N, sz = sizeof(double), nxp = (size_t)h->sim_nxp;
    const size_t nry = (io->flags & MPCQP_SIM_FLAG_RY_PER_PERIOD) ? N * d.ny : (size_t)d.ny;
    mpcqp_sim_io dv = *io;
    Staging s{h};
    int k = 0;
    // inputs and the in/out state go up, records are allocated; every array has its own staging buffer
    auto in = [&](const double*& p, size_t n) { p = s.in(h->sim_s[k++], p, B * n); };
    auto io_ = [&](double*& p, size_t n, bool up) {
        DBuf& b = h->sim_s[k++];
        p = !p ? nullptr : up ? s.in(b, p, B * n) : s.out<double>(b, B * n);
    };
    in(dv.ry, nry); in(dv.Ru, d.nU); in(dv.d, d.nd);
    in(dv.u_step, d.nu); in(dv.y_step, d.ny); in(dv.d_step, d.nd);
    in(dv.sigma_u, d.nu); in(dv.sigma_y, d.ny); in(dv.sigma_d, d.nd); in(dv.sigma_x, nxp);
    in(dv.w_u, N * d.nu); in(dv.w_y, N * d.ny); in(dv.w_d, N * d.nd); in(dv.w_x, N * nxp);
    const int k_out = k;
    io_(dv.x0, nxp, true); io_(dv.xhat0, d.nxh, true); io_(dv.lastu0, d.nu, true); io_(dv.Ztilde, d.nZ, true);
    io_(dv.Y, N * d.ny, false); io_(dv.X, N * nxp, false); io_(dv.D, N * d.nd, false); io_(dv.Xhat, N * d.nxh, false);
    io_(dv.Yhat, N * d.ny, false); io_(dv.U, N * d.nu, false); io_(dv.Ud, N * d.nu, false);
    dv.status = io->status ? s.out<int32_t>(h->sim_s[k], B * N) : nullptr;
    if (s.rc) return s.rc;
    if (d.nd == 0) dv.d = dv.d_step = dv.sigma_d = dv.w_d = nullptr, dv.D = nullptr;
    s.rc = mpcqp_sim_device(h, &dv, h->stream);
    // back in the same order, from the same buffers (what the device call was not given -- D without a measured
    // disturbance -- stays as the caller has it)
    k = k_out;
    auto down = [&](void* host, const void* dev, size_t bytes) { s.down(dev ? host : nullptr, h->sim_s[k++], bytes); };
    down(io->x0, dv.x0, B * nxp * sz);
    down(io->xhat0, dv.xhat0, B * d.nxh * sz);
    down(io->lastu0, dv.lastu0, B * d.nu * sz);
    down(io->Ztilde, dv.Ztilde, B * d.nZ * sz);
    down(io->Y, dv.Y, B * N * d.ny * sz);
    down(io->X, dv.X, B * N * nxp * sz);
    down(io->D, dv.D, B * N * d.nd * sz);
    down(io->Xhat, dv.Xhat, B * N * d.nxh * sz);
    down(io->Yhat, dv.Yhat, B * N * d.ny * sz);
    down(io->U, dv.U, B * N * d.nu * sz);
    down(io->Ud, dv.Ud, B * N * d.nu * sz);
    down(io->status, dv.status, B * N * sizeof(int32_t));
    return s.finish();
}

static thread_local std::string g_build_err;

const char* mpcqp_last_build_error(void) { return g_build_err.c_str(); }

// One cold-started step of the first few controllers of the handle on pseudo-random states / set points, once
// with the on-demand specialisation and once with the runtime-dimension kernel: same iterates up to rounding.
static int self_test_spec_impl(mpcqp_handle h, double* worst, std::string* why, DBuf& yh, DBuf& in, DBuf& out, DBuf& sti) {
    Dims d = h->d;
    d.B = d.B < 8 ? d.B : 8;
    d.flags = (d.flags | MPCQP_FLAG_COLD_START) & ~(uint32_t)(MPCQP_FLAG_KEEP_QP | MPCQP_FLAG_WARM_DUAL);
    const size_t n = d.B, nry = (d.flags & MPCQP_FLAG_RY_CONSTANT) ? d.ny : d.nY;
    const size_t cnt[] = {n * d.nxh, n * d.nu, n * nry, n * (d.nd ? d.nd : 1), n * (d.nD ? d.nD : 1), n * d.nZ, n * d.nZ, n * d.nu, n * d.nu};
    // (Ŷ as well: the specialisation's predict! path is part of what is tested)
    { int rcy = dev_alloc(h, yh, n * d.nY * sizeof(double)); if (rcy) return rcy; }
    std::vector<double> host(cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[4], 0.0);
    uint64_t lcg = 0x9E3779B97F4A7C15ull;
    auto rnd = [&] { lcg = lcg * 6364136223846793005ull + 1442695040888963407ull; return (double)(lcg >> 11) / 9007199254740992.0 * 2.0 - 1.0; };
    for (size_t i = 0; i < cnt[0]; ++i) host[i] = rnd();
    for (size_t i = 0; i < cnt[2]; ++i) host[cnt[0] + cnt[1] + i] = 2.0 * rnd();
    size_t total_in = host.size(), total_out = cnt[5] + cnt[6] + cnt[7] + cnt[8];
    int rc = dev_alloc(h, in, total_in * sizeof(double));
    if (!rc) rc = dev_alloc(h, out, total_out * sizeof(double));
    if (!rc) rc = dev_alloc(h, sti, 4 * n * sizeof(int32_t));
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(in.p, host.data(), total_in * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(out.p, 0, total_out * sizeof(double), h->stream));
    double* pin = (double*)in.p;
    double* pout = (double*)out.p;
    int32_t* pst = (int32_t*)sti.p;
    StepIO io{};
    io.xhat0 = pin; io.lastu0 = pin + cnt[0]; io.Ry = pin + cnt[0] + cnt[1];
    if (d.nd) { io.d0 = pin + cnt[0] + cnt[1] + cnt[2]; io.Dhat0 = io.d0 + cnt[3]; }
    io.Yhat0 = (double*)yh.p;
    io.kf_predict = 0;
    std::vector<double> z(cnt[5] + cnt[6]);
    std::vector<int32_t> s(4 * n);
    // both kernels on the same inputs with the dims `dd` (iteration cap / flags of the stage); returns the largest
    // difference of the two Z~ relative to max(1, |Z~|) (infinity on a NaN)
    auto run_pair = [&](const Dims& dd, double* rel) -> int {
        HIPCHK(hipMemsetAsync(out.p, 0, total_out * sizeof(double), h->stream));
        io.Z = pout; io.u0 = pout + cnt[5] + cnt[6]; io.status = pst; io.iters = pst + n;
        HIPCHK(launch_step_unverified_spec(dd, h->m, io, h->stream));
        io.Z = pout + cnt[5]; io.u0 = pout + cnt[5] + cnt[6] + cnt[7]; io.status = pst + 2 * n; io.iters = pst + 3 * n;
        HIPCHK(launch_step_generic(dd, h->m, io, h->stream));
        HIPCHK(hipMemcpyAsync(z.data(), pout, z.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipMemcpyAsync(s.data(), pst, s.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        double scale = 1.0, diff = 0.0;
        for (size_t i = 0; i < cnt[5]; ++i) {
            scale = std::fmax(scale, std::fabs(z[cnt[5] + i]));
            diff = std::fmax(diff, std::fabs(z[i] - z[cnt[5] + i]));
            if (!(z[i] == z[i])) diff = INFINITY;
        }
        *rel = diff / scale;
        return MPCQP_OK;
    };
    // Stage 1 (deterministic): the iterates after exactly 1, 2 and 3 interior-point iterations (MPCQP_FLAG_KEEP_ITERATE).
    // Same algorithm on the same data: the two kernels differ by rounding only (1e-13 measured; the starting point has
    // D~ <= 10, so the first Newton matrices are well conditioned), while a wrong entry of Phi, of a right-hand side or of a
    // row pass moves the iterate by its own size.  Iteration 1 assembles Phi over whatever the LDS held, iterations 2, 3
    // over the previous factor: the uninitialised-row class of bugs (round 3) shows in one of them.
    double worst_it = 0.0;
    int optimal_early = 0;
    for (int k = 1; k <= 3; ++k) {
        Dims dk = d;
        dk.max_iter = k;
        dk.flags |= MPCQP_FLAG_KEEP_ITERATE;
        double rel = 0.0;
        const int rc = run_pair(dk, &rel);
        if (rc) return rc;
        bool same_status = true;
        for (size_t i = 0; i < n; ++i) {
            same_status = same_status && s[i] == s[2 * n + i];
            if (s[i] == 0) ++optimal_early;        // (converged within k iterations: the optimum is compared, below)
        }
        if ((rel > 1e-8 || !same_status) && why && why->empty())
            *why = "the iterates after " + std::to_string(k) + " interior-point iteration(s) differ by " + std::to_string(rel) +
                   (same_status ? "" : " (different statuses)");
        if (!same_status) rel = INFINITY;
        worst_it = std::fmax(worst_it, rel);
    }
    // Stage 2: the complete solves -- same statuses, the same optimum.  (The iteration counts are reported, not judged:
    // an accepted or refused polish attempt moves either count by several iterations -- round 3's rule "not more than
    // max(4, half) extra iterations" rejected a correct kernel at 14 vs 6.)
    double rel_opt = 0.0;
    rc = run_pair(d, &rel_opt);
    if (rc) return rc;
    for (size_t i = 0; i < n; ++i) {
        if (s[i] != s[2 * n + i]) {
            if (why && why->empty())
                *why = "controller " + std::to_string(i) + ": status " + std::to_string(s[i]) + " after " + std::to_string(s[n + i]) +
                       " iterations, runtime-dimension kernel: status " + std::to_string(s[2 * n + i]) + " after " +
                       std::to_string(s[3 * n + i]);
            rel_opt = INFINITY;
        }
    }
    if (rel_opt > 1e-6 && why && why->empty()) *why = "the optima differ by " + std::to_string(rel_opt);
    if (getenv("MPCQP_SELFTEST_VERBOSE")) {
        fprintf(stderr, "[mpcqp] self-test %d,%d,%d,%d,%d,%d,%x: first iterates differ by %.3e, optima by %.3e; iterations",
                d.nu, d.ny, d.nxh, d.Hp, d.Hc, d.neps, d.gmask, worst_it, rel_opt);
        for (size_t i = 0; i < n; ++i) fprintf(stderr, " %d/%d", s[n + i], s[3 * n + i]);
        fprintf(stderr, " (%d early optima)\n", optimal_early);
    }
    // one figure for the caller's tolerance (1e-6): the first iterates are held to 1e-8
    *worst = std::fmax(rel_opt, worst_it * 100.0);
    return MPCQP_OK;
}

static int self_test_spec(mpcqp_handle h, double* worst, std::string* why) {
    DBuf yh, in, out, sti;           // scratch of the comparison: released on every path
    const int rc = self_test_spec_impl(h, worst, why, yh, in, out, sti);
    (void)hipStreamSynchronize(h->stream);
    dev_release(h, yh); dev_release(h, in); dev_release(h, out); dev_release(h, sti);
    return rc;
}

int mpcqp_prepare(mpcqp_handle h) {
    if (!h) return MPCQP_ERR_NULL;
    g_build_err.clear();
    if (uses_stage_kernel(h)) {
        // nothing to build: the stage-structured kernel is in the library.  A handle it cannot take is refused here exactly
        // as its steps are (mpcqp_step*: MPCQP_ERR_UNSUPPORTED) -- the answer is what the steps WILL do
        return ms_unsupported(h) ? MPCQP_ERR_UNSUPPORTED : MPCQP_KERNEL_MS;
    }
    {   // the steps that follow run on the caller's stream, which nothing orders after the handle's: like every setter,
        // return with the handle's data complete
        ON_DEVICE(h);
        int rc = ensure_hessian(h, h->stream);
        if (!rc) rc = ensure_stepc(h, h->stream);
        if (rc) return rc;
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    int kind = prepare_step(h->d, h->m, &g_build_err);
    // an on-demand kernel that has not been checked yet (fresh build, or a cache some other process filled): compare
    // it with the runtime-dimension kernel once; needs the model and weights (BatchLinMPC prepares before its first step)
    // (a handle of the small-problem kernel has its specialisation verified too: steps that ask for Ŷ or fuse the Kalman steps
    //  run on it, and so do the dense-row handles of small batches -- mpcqp_kernels.hip: small_takes)
    const bool ondemand = kind == MPCQP_KERNEL_ONDEMAND || (kind == MPCQP_KERNEL_SMALL && !aot_or_generic_other(h->d) && spec_present(h->d));
    if (ondemand && !spec_verified(h->d) && h->have_model && h->have_weights &&
        step_lds_bytes(h->d) <= 160 * 1024) {
        ON_DEVICE(h);
        double worst = 0.0;
        std::string why;
        int rc = self_test_spec(h, &worst, &why);
        if (rc) return rc;
        const char* tol_env = getenv("MPCQP_JIT_SELFTEST_TOL");       // (tests force a rejection with a negative value)
        const double tol = tol_env ? atof(tol_env) : 1e-6;
        if (worst <= tol) {
            mark_spec_verified(h->d);
            if (kind == MPCQP_KERNEL_SMALL) kind = step_kernel_kind(h->d, h->m);      // (a small batch with dense rows moves to it)
        } else {
            reject_spec(h->d);
            g_build_err = "the on-demand specialisation disagrees with the runtime-dimension kernel (relative difference " +
                          std::to_string(worst) + (why.empty() ? "" : "; " + why) + "): rejected, the runtime-dimension kernel is used";
            fprintf(stderr, "[mpcqp] %s\n", g_build_err.c_str());
            if (kind != MPCQP_KERNEL_SMALL) kind = MPCQP_KERNEL_GENERIC;
        }
    } else if (ondemand && !spec_verified(h->d)) {
        // built / found, but not compared with the runtime-dimension kernel yet (no model or weights, or the problem does
        // not fit the LDS): steps run the runtime-dimension kernel until a later mpcqp_prepare has verified the object --
        // the return value is the kind the steps WILL run on
        g_build_err = "the on-demand specialisation exists but has not been verified on this machine yet (mpcqp_prepare "
                      "after set_model and set_weights compares it with the runtime-dimension kernel)";
        if (kind != MPCQP_KERNEL_SMALL) kind = MPCQP_KERNEL_GENERIC;
    }
    return kind;
}

int mpcqp_set_iteration_limit(mpcqp_handle h, int32_t max_iter) {
    if (!h) return MPCQP_ERR_NULL;
    if (max_iter < 0) return MPCQP_ERR_ARG;
    h->d.max_iter = max_iter > 0 ? max_iter : 80;
    return MPCQP_OK;
}

int mpcqp_lds_bytes(mpcqp_handle h) {
    if (!h) return MPCQP_ERR_NULL;
    return (int)step_lds_bytes(h->d);
}

int mpcqp_kernel_kind(mpcqp_handle h) {
    if (!h) return MPCQP_ERR_NULL;
    if (uses_stage_kernel(h)) return ms_unsupported(h) ? MPCQP_ERR_UNSUPPORTED : MPCQP_KERNEL_MS;
    return step_kernel_kind(h->d, h->m);
}

int mpcqp_predmat_form(mpcqp_handle h) {
    if (!h) return MPCQP_ERR_NULL;
    return predmat_form_is_mfma(h->d) ? 1 : 0;
}

int mpcqp_step_consts_builds(mpcqp_handle h) {
    if (!h) return MPCQP_ERR_NULL;
    return h->stepc_builds;
}

int mpcqp_row_groups(mpcqp_handle h, uint32_t* row_groups) {
    if (!h || !row_groups) return MPCQP_ERR_NULL;
    *row_groups = h->d.gmask;
    return MPCQP_OK;
}

int mpcqp_prebuild(const mpcqp_dims* in, uint32_t row_groups) {
    if (!in) return MPCQP_ERR_NULL;
    if (in->nxhat < 1 || in->nu < 1 || in->ny < 1 || in->Hp < 1 || in->Hc < 1 || in->Hc > in->Hp ||
        (in->neps != 0 && in->neps != 1) || (row_groups >> NGROUP))
        return MPCQP_ERR_ARG;
    Dims d{};
    d.nxh = in->nxhat; d.nu = in->nu; d.ny = in->ny; d.nd = in->nd; d.Hp = in->Hp; d.Hc = in->Hc; d.neps = in->neps;
    d.nDU = d.nu * d.Hc; d.nZ = d.nDU + d.neps; d.nU = d.nu * d.Hp; d.nY = d.ny * d.Hp;
    d.gmask = row_groups;
    d.default_nb = 1;
    if (in->nb)
        for (int i = 0; i < d.Hc; ++i)
            if (in->nb[i] != (i == d.Hc - 1 ? d.Hp - d.Hc + 1 : 1)) d.default_nb = 0;
    g_build_err.clear();
    const int k = prebuild_step(d, &g_build_err);
    // Kernel revision 10 (round 5) moved the row -eps <= 0 into a Y group when one exists: mpcqp_set_bounds no longer sets bit 0
    // for it (C3: 0x8d -> 0x8c).  A manifest line written before that still compiles, but no handle matches the object unless
    // it really has hard dUmin rows: say so (mpcqp_last_build_error) instead of leaving the deployment on the JIT silently.
    if (k >= 0 && d.neps && (row_groups & 1u) && !(row_groups & 2u) && (row_groups & (3u << (2 * P_Y))) && g_build_err.empty())
        g_build_err = "row_groups has bit 0 (box lower) together with an output-bound group and no box upper group: since kernel "
                      "revision 10 the slack's own row rides in the output group, so only a controller with hard dUmin bounds "
                      "and no dUmax matches this object -- a pre-revision-10 manifest line? (drop bit 0: e.g. 0x8d -> 0x8c)";
    return k < 0 ? MPCQP_ERR_DEVICE : k;
}

// ---- several devices behind one handle ---------------------------------------------------------
int mpcqp_multi_create(const mpcqp_dims* in, const int32_t* device_ids, int32_t ndev, mpcqp_multi* out) {
    if (!in || !device_ids || !out) return MPCQP_ERR_NULL;
    *out = nullptr;
    if (ndev < 1 || in->batch < ndev) return MPCQP_ERR_ARG;
    mpcqp_multi mh = new (std::nothrow) mpcqp_multi_s();
    if (!mh) return MPCQP_ERR_NOMEM;
    const int B = in->batch, base = B / ndev, rem = B % ndev;
    int o = 0;
    for (int g = 0; g < ndev; ++g) {
        mpcqp_dims dg = *in;
        dg.batch = base + (g < rem ? 1 : 0);
        dg.device = device_ids[g];
        mpcqp_handle hg = nullptr;
        const int rc = mpcqp_create(&dg, &hg);
        if (rc) { mpcqp_multi_destroy(mh); return rc; }
        hg->in_multi = true;
        mh->h.push_back(hg);
        mh->off.push_back(o);
        mh->cnt.push_back(dg.batch);
        o += dg.batch;
    }
    mh->d = mh->h[0]->d;
    mh->d.B = B;
    *out = mh;
    return MPCQP_OK;
}

int mpcqp_multi_destroy(mpcqp_multi mh) {
    if (!mh) return MPCQP_ERR_NULL;
    for (mpcqp_handle hg : mh->h) (void)mpcqp_destroy(hg);
    delete mh;
    return MPCQP_OK;
}

int mpcqp_multi_ndev(mpcqp_multi mh) { return mh ? (int)mh->h.size() : MPCQP_ERR_NULL; }

mpcqp_handle mpcqp_multi_handle(mpcqp_multi mh, int32_t g) {
    return (mh && g >= 0 && g < (int)mh->h.size()) ? mh->h[g] : nullptr;
}

int mpcqp_multi_shard(mpcqp_multi mh, int32_t g, int32_t* offset, int32_t* count) {
    if (!mh || !offset || !count) return MPCQP_ERR_NULL;
    if (g < 0 || g >= (int)mh->h.size()) return MPCQP_ERR_ARG;
    *offset = mh->off[g]; *count = mh->cnt[g];
    return MPCQP_OK;
}

int mpcqp_multi_set_model(mpcqp_multi mh, const double* Ahat, const double* Bu, const double* C,
                          const double* Bd, const double* Dd, const double* dop) {
    if (!mh) return MPCQP_ERR_NULL;
    const Dims& d = mh->d;
    for (size_t g = 0; g < mh->h.size(); ++g) {
        const int o = mh->off[g];
        const int rc = mpcqp_set_model(mh->h[g], shard_of(Ahat, o, (size_t)d.nxh * d.nxh), shard_of(Bu, o, (size_t)d.nxh * d.nu),
                                       shard_of(C, o, (size_t)d.ny * d.nxh), shard_of(Bd, o, (size_t)d.nxh * d.nd),
                                       shard_of(Dd, o, (size_t)d.ny * d.nd), shard_of(dop, o, d.nxh));
        if (rc) return rc;
    }
    return MPCQP_OK;
}

int mpcqp_multi_set_weights(mpcqp_multi mh, const double* Mdiag, const double* Ndiag, const double* Ldiag,
                            const double* Cwt) {
    if (!mh) return MPCQP_ERR_NULL;
    const Dims& d = mh->d;
    for (size_t g = 0; g < mh->h.size(); ++g) {
        const int o = mh->off[g];
        const int rc = mpcqp_set_weights(mh->h[g], shard_of(Mdiag, o, d.nY), shard_of(Ndiag, o, d.nDU),
                                         shard_of(Ldiag, o, d.nU), shard_of(Cwt, o, 1));
        if (rc) return rc;
    }
    return MPCQP_OK;
}

int mpcqp_multi_set_bounds(mpcqp_multi mh, const mpcqp_bounds* b) {
    if (!mh || !b) return MPCQP_ERR_NULL;
    const Dims& d = mh->d;
    for (size_t g = 0; g < mh->h.size(); ++g) {
        const int o = mh->off[g];
        mpcqp_bounds s{};
        s.U0min = shard_of(b->U0min, o, d.nU); s.U0max = shard_of(b->U0max, o, d.nU);
        s.DUmin = shard_of(b->DUmin, o, d.nDU); s.DUmax = shard_of(b->DUmax, o, d.nDU);
        s.Y0min = shard_of(b->Y0min, o, d.nY); s.Y0max = shard_of(b->Y0max, o, d.nY);
        s.x0min = shard_of(b->x0min, o, d.nxh); s.x0max = shard_of(b->x0max, o, d.nxh);
        s.C_umin = shard_of(b->C_umin, o, d.nU); s.C_umax = shard_of(b->C_umax, o, d.nU);
        s.C_dumin = shard_of(b->C_dumin, o, d.nDU); s.C_dumax = shard_of(b->C_dumax, o, d.nDU);
        s.C_ymin = shard_of(b->C_ymin, o, d.nY); s.C_ymax = shard_of(b->C_ymax, o, d.nY);
        s.c_x0min = shard_of(b->c_x0min, o, d.nxh); s.c_x0max = shard_of(b->c_x0max, o, d.nxh);
        const int rc = mpcqp_set_bounds(mh->h[g], &s);
        if (rc) return rc;
    }
    return MPCQP_OK;
}

int mpcqp_multi_prepare(mpcqp_multi mh) {
    if (!mh) return MPCQP_ERR_NULL;
    // every shard has the same dimensions, hence the same kernel -- unless a shard's on-demand kernel was rejected on
    // its device: the runtime-dimension kernel of ANY shard is what the caller has to know about
    int kind = -1;
    for (mpcqp_handle hg : mh->h) {
        const int k = mpcqp_prepare(hg);
        if (k < 0) return k;
        if (kind < 0 || k == MPCQP_KERNEL_GENERIC) kind = k;
    }
    return kind;
}

int mpcqp_multi_step(mpcqp_multi mh, const double* xhat0, const double* lastu0, const double* Ry,
                     const double* Ru, const double* d0, const double* Dhat0, double* Ztilde,
                     double* u0, int32_t* status, int32_t* iters, double* Yhat0) {
    if (!mh || !xhat0 || !lastu0 || !Ry || !Ztilde || !u0 || !status) return MPCQP_ERR_NULL;
    const Dims& dd = mh->d;
    if (dd.nd > 0 && (!d0 || !Dhat0)) return MPCQP_ERR_NULL;
    // phase 1: uploads, the step kernel and the gather -- each shard's results into its slice of the caller's arrays --
    // enqueued on every device's stream
    for (size_t g = 0; g < mh->h.size(); ++g) {
        mpcqp_handle h = mh->h[g];
        const Dims& d = h->d;
        const int o = mh->off[g];
        const size_t nry = (d.flags & MPCQP_FLAG_RY_CONSTANT) ? d.ny : d.nY;
        ON_DEVICE(h);
        const int rc = step_staged(h, shard_of(xhat0, o, d.nxh), shard_of(lastu0, o, d.nu), shard_of(Ry, o, nry), shard_of(Ru, o, d.nU),
                                   shard_of(d0, o, d.nd), shard_of(Dhat0, o, d.nD), shard_of(Ztilde, o, d.nZ), shard_of(u0, o, d.nu),
                                   shard_of(status, o, 1), shard_of(iters, o, 1), shard_of(Yhat0, o, d.nY));
        if (rc) return rc;
    }
    // phase 2: wait for every device
    for (mpcqp_handle h : mh->h) {
        ON_DEVICE(h);
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return MPCQP_OK;
}

int mpcqp_multi_gather_device(mpcqp_multi mh, int32_t root, const double* const* Z_shards,
                              const double* const* u0_shards, const int32_t* const* status_shards,
                              double* Z_root, double* u0_root, int32_t* status_root, void* stream) {
    if (!mh || !Z_shards || !u0_shards || !status_shards || !Z_root || !u0_root || !status_root) return MPCQP_ERR_NULL;
    if (root < 0 || root >= (int)mh->h.size()) return MPCQP_ERR_ARG;
    mpcqp_handle hr = mh->h[root];
    ON_DEVICE(hr);
    hipStream_t st = stream ? (hipStream_t)stream : hr->stream;
    const Dims& d = mh->d;
    for (size_t g = 0; g < mh->h.size(); ++g) {
        const int o = mh->off[g], src = mh->h[g]->device;
        const size_t B = mh->cnt[g];
        if (!Z_shards[g] || !u0_shards[g] || !status_shards[g]) return MPCQP_ERR_NULL;
        HIPCHK(hipMemcpyPeerAsync(shard_of(Z_root, o, d.nZ), hr->device, Z_shards[g], src, B * d.nZ * sizeof(double), st));
        HIPCHK(hipMemcpyPeerAsync(shard_of(u0_root, o, d.nu), hr->device, u0_shards[g], src, B * d.nu * sizeof(double), st));
        HIPCHK(hipMemcpyPeerAsync(shard_of(status_root, o, 1), hr->device, status_shards[g], src, B * sizeof(int32_t), st));
    }
    if (!stream) HIPCHK(hipStreamSynchronize(st));
    return MPCQP_OK;
}

int mpcqp_multi_scatter_device(mpcqp_multi mh, int32_t root, const double* xhat0_root, const double* lastu0_root,
                               const double* Ry_root, int32_t ry_rows, double* const* xhat0_shards,
                               double* const* lastu0_shards, double* const* Ry_shards, void* stream) {
    if (!mh || !xhat0_root || !lastu0_root || !Ry_root || !xhat0_shards || !lastu0_shards || !Ry_shards) return MPCQP_ERR_NULL;
    if (root < 0 || root >= (int)mh->h.size() || ry_rows <= 0) return MPCQP_ERR_ARG;
    mpcqp_handle hr = mh->h[root];
    ON_DEVICE(hr);
    hipStream_t st = stream ? (hipStream_t)stream : hr->stream;
    const Dims& d = mh->d;
    for (size_t g = 0; g < mh->h.size(); ++g) {
        const int o = mh->off[g], dst = mh->h[g]->device;
        const size_t B = mh->cnt[g];
        if (!xhat0_shards[g] || !lastu0_shards[g] || !Ry_shards[g]) return MPCQP_ERR_NULL;
        HIPCHK(hipMemcpyPeerAsync(xhat0_shards[g], dst, shard_of(xhat0_root, o, d.nxh), hr->device, B * d.nxh * sizeof(double), st));
        HIPCHK(hipMemcpyPeerAsync(lastu0_shards[g], dst, shard_of(lastu0_root, o, d.nu), hr->device, B * d.nu * sizeof(double), st));
        HIPCHK(hipMemcpyPeerAsync(Ry_shards[g], dst, shard_of(Ry_root, o, ry_rows), hr->device, B * (size_t)ry_rows * sizeof(double), st));
    }
    if (!stream) HIPCHK(hipStreamSynchronize(st));
    return MPCQP_OK;
}

static double elapsed(hipEvent_t a, hipEvent_t b, bool timed) {
    if (!timed) return -1.0;
    if (hipEventSynchronize(b) != hipSuccess) return -1.0;
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return -1.0;
    return (double)ms;
}

double mpcqp_last_step_ms(mpcqp_handle h) {
    return h ? elapsed(h->ev_s0, h->ev_s1, h->step_timed) : -1.0;
}

double mpcqp_last_condense_ms(mpcqp_handle h) {
    return h ? elapsed(h->ev_c0, h->ev_c1, h->cond_timed) : -1.0;
}

double mpcqp_last_predmat_ms(mpcqp_handle h) {
    return h ? elapsed(h->ev_c0, h->ev_cm, h->cond_timed) : -1.0;
}

}  // extern "C"
