// spec_cache.cpp -- on-demand specialisation of the step kernel: the cache of shared objects and its compiler driver.
// Dimensions outside the ahead-of-time list get their own compile-time-dims kernel: csrc/mpcqp_spec.hip is compiled with the
// installation's hipcc (the same compiler as the ahead-of-time build), cached as spec_<rev>_<dims>.so and dlopen'ed.  The
// compilation NEVER happens inside a step: it is done by prepare_step() (mpcqp_prepare / mpcqp_prebuild of the C-ABI), the step
// only looks the object up and runs the runtime-dimension kernel when there is none.  The compiler is started with posix_spawn
// on an argument vector (no shell: paths with spaces or metacharacters are data), its output goes to a log file next to the object.
//   MPCQP_JIT=0          no on-demand kernels at all
//   HIPCC                the compiler binary (one path; default /opt/rocm/bin/hipcc)
//   MPCQP_JIT_FLAGS      extra compiler arguments, space separated (experiments)
//   MPCQP_CACHE_DIR      where the objects live; default <library dir>/spec_cache when that is writable,
//                        else $XDG_CACHE_HOME/mpcqp or ~/.cache/mpcqp
// Host-only: no GPU, no HIP header (tests/spec_cache_main.cpp runs this unit under sanitizers).
#include "spec_cache.h"

#include <dirent.h>
#include <dlfcn.h>
#include <errno.h>
#include <fcntl.h>
#include <spawn.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

extern char** environ;      // (the specialisation compiler inherits the environment)

namespace mpcqp {

static bool env_flag(const char* name, bool dflt) { const char* e = getenv(name); return e ? e[0] == '1' : dflt; }
bool force_generic() { static const bool f = env_flag("MPCQP_FORCE_GENERIC", false); return f; }

struct SpecLib : SpecEntry { std::string path; };      // path: the object this entry was loaded from
using SpecKey = std::tuple<int, int, int, int, int, int, unsigned, int>;
// last field (also the last field of the object name): bit 0 default move blocking, bit 1 dense M_Hp / L_Hp in the gradient,
// bits 2.. the number of custom linear constraint rows per step
static int spec_variant(const Dims& d) { return d.default_nb | (d.dense_w ? 2 : 0) | (d.nw << 2); }
static SpecKey spec_key(const Dims& d) { return SpecKey{d.nu, d.ny, d.nxh, d.Hp, d.Hc, d.neps, d.gmask, spec_variant(d)}; }
static std::mutex g_spec_mu;                     // (lock order: g_spec_mu, then g_rej_mu)
static std::map<SpecKey, SpecLib> g_spec;        // failed loads are cached as empty entries

static std::string lib_dir() {
    Dl_info info;
    if (!dladdr((const void*)&lib_dir, &info) || !info.dli_fname) return ".";
    std::string p(info.dli_fname);
    size_t s = p.rfind('/');
    return s == std::string::npos ? "." : p.substr(0, s);
}

static bool dir_writable(const std::string& d) {
    struct stat sb;
    if (stat(d.c_str(), &sb) != 0 && mkdir(d.c_str(), 0755) != 0 && errno != EEXIST) return false;
    return access(d.c_str(), W_OK | X_OK) == 0;
}

static std::string user_cache_dir() {
    std::string base;
    if (const char* x = getenv("XDG_CACHE_HOME")) base = x;
    if (base.empty()) {
        const char* home = getenv("HOME");
        if (!home || !home[0]) return "";        // no private place to keep shared objects
        base = std::string(home) + "/.cache";
        (void)dir_writable(base);
    }
    const std::string d = base + "/mpcqp";
    (void)dir_writable(d);
    return d;
}

static const char* env_cache_dir() {         // MPCQP_CACHE_DIR, nullptr when unset or empty
    const char* e = getenv("MPCQP_CACHE_DIR");
    return e && e[0] ? e : nullptr;
}

// where NEW files go (objects built here, the .ok / .rejected markers of objects in a read-only directory)
static std::string cache_dir() {
    if (const char* e = env_cache_dir()) { (void)dir_writable(e); return e; }
    const std::string local = lib_dir() + "/spec_cache";
    if (dir_writable(local)) return local;
    return user_cache_dir();
}

// where objects are LOOKED UP: the installation's own <library dir>/spec_cache is searched even when it is read-only
// (the normal deployment: objects shipped by `python -m mpcqp.prebuild` / mpcqp_prebuild on a build host), then the
// user's cache.  MPCQP_CACHE_DIR replaces both.
static std::vector<std::string> search_dirs() {
    if (const char* e = env_cache_dir()) return {e};
    std::vector<std::string> v = {lib_dir() + "/spec_cache"};
    const std::string u = user_cache_dir();
    if (!u.empty() && u != v[0]) v.push_back(u);
    return v;
}

// Shared objects are only loaded from a directory that belongs to this user (or root) and that others cannot write.
static bool cache_dir_trusted(const std::string& d) {
    struct stat sb;
    if (d.empty() || stat(d.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode)) return false;
    if (sb.st_uid != geteuid() && sb.st_uid != 0) return false;
    const bool ok = (sb.st_mode & (S_IWGRP | S_IWOTH)) == 0;
    static bool told = false;
    if (!ok && !told) {
        told = true;
        fprintf(stderr, "[mpcqp] specialisation cache %s is writable by group / others: not used (chmod go-w, or set MPCQP_CACHE_DIR)\n", d.c_str());
    }
    return ok;
}

// ... and only files that belong to this user (or root) and that others cannot write
static bool object_trusted(const std::string& so) {
    struct stat sb;
    if (stat(so.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) return false;
    if (sb.st_uid != geteuid() && sb.st_uid != 0) return false;
    return (sb.st_mode & (S_IWGRP | S_IWOTH)) == 0;
}

static std::string hipcc_path() {
    const char* hipcc = getenv("HIPCC");
    return hipcc && hipcc[0] ? hipcc : "/opt/rocm/bin/hipcc";
}

// identity of the compiler the on-demand kernels are built with (size and mtime of the binary): part of the
// object name, so that a cache filled by another hipcc is not reused WHEN THIS MACHINE CAN BUILD ITS OWN (the same
// 32-bit value as __graft_entry__.py computes for the objects it pre-builds).  0: no compiler here.
static unsigned compiler_id() {
    struct stat sb;
    if (stat(hipcc_path().c_str(), &sb) != 0) return 0u;
    return (unsigned)(((unsigned long long)sb.st_size * 1000003ull) ^ (unsigned long long)sb.st_mtime);
}

static std::string spec_dims_suffix(const Dims& d) {
    char name[160];
    snprintf(name, sizeof name, "_%d_%d_%d_%d_%d_%d_%x_%d.so", d.nu, d.ny, d.nxh, d.Hp, d.Hc, d.neps, d.gmask, spec_variant(d));
    return name;
}
static std::string spec_rev_prefix() { return "spec_r" + std::to_string(MPCQP_KERNEL_REV) + "_c"; }

// name of the object this machine's compiler builds
static std::string spec_name(const Dims& d) {
    char cid[16];
    snprintf(cid, sizeof cid, "%08x", compiler_id());
    return spec_rev_prefix() + cid + spec_dims_suffix(d);
}

// objects rejected by this process whose file could not be renamed (read-only cache)
static std::mutex g_rej_mu;
static std::vector<std::string> g_rejected;
static bool rejected_here(const std::string& so) {
    std::lock_guard<std::mutex> lock(g_rej_mu);
    for (const std::string& r : g_rejected) if (r == so) return true;
    struct stat sb;
    const size_t sl = so.rfind('/');
    return stat((cache_dir() + "/" + so.substr(sl + 1) + ".rejected").c_str(), &sb) == 0;
}

// The object of `d` a step may load: the one this machine's compiler builds (exact name) in any search directory, else
// -- no compiler here, or a cache filled by a build host with another hipcc -- any object of the same kernel revision and
// dimensions, `spec_r<rev>_c*_<dims>.so`.  Safe because no object runs before mpcqp_prepare has compared it with the
// runtime-dimension kernel ON THIS MACHINE (marker .ok); with a local compiler the exact name wins and a foreign object
// is only used while the local one does not exist (prepare builds it).  "" if there is none.
static std::string locate_spec(const Dims& d, bool foreign_ok) {
    const std::string exact = spec_name(d), pre = spec_rev_prefix(), suf = spec_dims_suffix(d);
    const std::vector<std::string> dirs = search_dirs();
    for (const std::string& dir : dirs) {
        if (!cache_dir_trusted(dir)) continue;
        const std::string so = dir + "/" + exact;
        if (object_trusted(so) && !rejected_here(so)) return so;
    }
    if (!foreign_ok) return "";
    for (const std::string& dir : dirs) {
        if (!cache_dir_trusted(dir)) continue;
        DIR* dp = opendir(dir.c_str());
        if (!dp) continue;
        std::string best;
        while (struct dirent* e = readdir(dp)) {
            const std::string f = e->d_name;
            if (f.size() != exact.size() || f.compare(0, pre.size(), pre) != 0 ||
                f.compare(f.size() - suf.size(), suf.size(), suf) != 0)
                continue;
            const std::string so = dir + "/" + f;
            if (object_trusted(so) && !rejected_here(so) && (best.empty() || so < best)) best = so;
        }
        closedir(dp);
        if (!best.empty()) return best;
    }
    return "";
}
static std::string locate_spec(const Dims& d) { return locate_spec(d, compiler_id() == 0u || !env_flag("MPCQP_CACHE_STRICT", false)); }

// marker <object>.ok next to the object when its directory is writable, else under the same name in cache_dir()
static std::string marker_path(const std::string& so, const char* ext) {
    const size_t sl = so.rfind('/');
    const std::string dir = so.substr(0, sl);
    if (access(dir.c_str(), W_OK | X_OK) == 0) return so + ext;
    return cache_dir() + "/" + so.substr(sl + 1) + ext;
}

static bool jit_enabled() { static const bool on = env_flag("MPCQP_JIT", true); return on; }

// (custom linear constraints and dense M_Hp / L_Hp get on-demand variants of their own: -DMPCQP_SPEC_NW=nw compiles the
// custom rows in (row state in registers like every other group), -DMPCQP_SPEC_DENSE the dense products of the gradient;
// compile-time dims up to MPCQP_SPEC_NZMAX: beyond one row per lane the specialisation keeps the several-rows-per-lane
// factorisation of the runtime dims but has the matrix-core E'DE, register rows and constant trip counts)
#ifndef MPCQP_SPEC_NZMAX
#define MPCQP_SPEC_NZMAX 256      // (round 5: 128 before.  Whatever fits the LDS -- nZ~ up to ~185 -- gets its specialisation: nZ~ = 141 ... 161 run 3.6 - 4.3
                                  //  times faster than on the runtime-dimension kernel, 450 - 470 VGPRs at one wavefront per SIMD, compiled in ~50 s)
#endif
static bool spec_eligible(const Dims& d) { return d.nZ <= MPCQP_SPEC_NZMAX; }
bool spec_enabled(const Dims& d) { return jit_enabled() && spec_eligible(d); }

// run `argv` (argv[0] = binary), stdout+stderr appended to `log`; returns the exit status, -1 on failure to start
static int run_process(const std::vector<std::string>& argv, const std::string& log) {
    std::vector<char*> av;
    for (const std::string& a : argv) av.push_back(const_cast<char*>(a.c_str()));
    av.push_back(nullptr);
    posix_spawn_file_actions_t fa;
    posix_spawn_file_actions_init(&fa);
    posix_spawn_file_actions_addopen(&fa, 1, log.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);
    posix_spawn_file_actions_adddup2(&fa, 1, 2);
    pid_t pid = 0;
    const int rc = posix_spawn(&pid, av[0], &fa, nullptr, av.data(), ::environ);
    posix_spawn_file_actions_destroy(&fa);
    if (rc != 0) return -1;
    int status = 0;
    while (waitpid(pid, &status, 0) < 0) {
        if (errno != EINTR) return -1;
    }
    return WIFEXITED(status) ? WEXITSTATUS(status) : -1;
}

int spec_build(const Dims& d, std::string* path_out, std::string* err) {
    const std::string cache = cache_dir(), so = cache + "/" + spec_name(d);
    if (path_out) *path_out = so;
    if (!cache_dir_trusted(cache)) {
        if (err) *err = "specialisation cache directory '" + cache + "' is missing, not owned by this user or writable by others (set MPCQP_CACHE_DIR)";
        return -1;
    }
    {
        // an object of this shape that may be loaded exists already (this machine's own, or -- without a compiler here --
        // one a build host shipped)
        const std::string have = locate_spec(d, compiler_id() == 0u);
        if (!have.empty()) { if (path_out) *path_out = have; return 0; }
    }
    if (compiler_id() == 0u) {
        if (err) *err = "no compiler (" + hipcc_path() + ") and no prebuilt object of this shape in the specialisation cache";
        return -1;
    }
    if (access(cache.c_str(), W_OK | X_OK) != 0) {
        if (err) *err = "specialisation cache directory " + cache + " is not writable (set MPCQP_CACHE_DIR)";
        return -1;
    }
    const std::string src = lib_dir() + "/../csrc";
    char dims[160];
    snprintf(dims, sizeof dims, "-DMPCQP_SPEC_DIMS=%d,%d,%d,%d,%d,%d,%uu,%d", d.nu, d.ny, d.nxh, d.Hp, d.Hc, d.neps,
             d.gmask, d.default_nb);
    const std::string tmp = so + ".tmp" + std::to_string((long)getpid());   // (ranks of one job may build the same object)
    std::vector<std::string> argv = {hipcc_path(), "--offload-arch=gfx950", "-O3",
                                     "-std=c++17", "-shared", "-fPIC", "-w", "-I" + src, dims};
    // beyond one row per lane the LDS footprint (Phi alone is 47 KB at nZ~ = 106) leaves at most one wavefront per SIMD:
    // the kernel may as well use the whole register file (row state of several rows per lane in registers, no spills)
    if (d.nZ > WAVE) argv.push_back("-DMPCQP_STEP_WAVES=1");
    // `#pragma unroll` gives up beyond 16k unrolled instructions (LLVM's pragma-unroll-threshold): from eight tile rows on
    // (nZ~ >= ~113) a loop over the tile rows stayed rolled, its arrays went to scratch memory and every LDS and global access
    // became a flat one (DESIGN 4.1 "Beyond one row per lane": 1.5 times slower); smaller shapes compile to the same code.
    argv.push_back("-mllvm");
    argv.push_back("-pragma-unroll-threshold=1048576");
    if (d.dense_w) argv.push_back("-DMPCQP_SPEC_DENSE=1");
    if (d.nw > 0) argv.push_back("-DMPCQP_SPEC_NW=" + std::to_string(d.nw));
    if (const char* extra = getenv("MPCQP_JIT_FLAGS")) {
        std::string tok;
        for (const char* c = extra;; ++c) {
            if (*c == ' ' || *c == 0) { if (!tok.empty()) argv.push_back(tok); tok.clear(); if (!*c) break; }
            else tok += *c;
        }
    }
    argv.push_back(src + "/mpcqp_spec.hip");
    argv.push_back("-o");
    argv.push_back(tmp);
    fprintf(stderr, "[mpcqp] specialising the step kernel for nu=%d ny=%d nxhat=%d Hp=%d Hc=%d neps=%d rows=0x%x "
                    "(one-time, cached in %s)\n", d.nu, d.ny, d.nxh, d.Hp, d.Hc, d.neps, d.gmask, cache.c_str());
    const std::string log = so + ".log";
    const int rc = run_process(argv, log);
    if (rc != 0 || rename(tmp.c_str(), so.c_str()) != 0) {
        (void)unlink(tmp.c_str());
        if (err) *err = "compiling the specialisation failed (exit " + std::to_string(rc) + ", see " + log + ")";
        return -1;
    }
    (void)unlink(log.c_str());
    return 0;
}

// the cache's entry of `d`, nullptr where no object is loaded; loads a cached object, never compiles.  g_spec_mu is held.
static SpecLib* find_locked(const Dims& d) {
    if (!jit_enabled() || !spec_eligible(d)) return nullptr;
    const SpecKey key = spec_key(d);
    auto it = g_spec.find(key);
    if (it != g_spec.end()) return it->second.step ? &it->second : nullptr;
    const std::string so = locate_spec(d);
    if (so.empty()) {
        // not built (yet).  The miss is remembered (a step of a small dense-row handle asked again at every launch --
        // stat / opendir / readdir over the cache directories under g_spec_mu, and a dlopen inside a step once another
        // process had filled the cache); mpcqp_prepare forgets it before it builds or looks again (spec_forget_miss).
        g_spec.emplace(key, SpecLib{});
        return nullptr;
    }
    SpecLib sl;
    void* hdl = dlopen(so.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (hdl) {
        sl.matches = (int (*)(const Dims*))dlsym(hdl, "mpcqp_spec_matches");
        sl.matches_dims = (int (*)(const Dims*))dlsym(hdl, "mpcqp_spec_matches_dims");
        sl.step = (int (*)(const Dims*, const Model*, const StepIO*, void*))dlsym(hdl, "mpcqp_spec_launch_step");
        sl.hessian = (int (*)(const Dims*, const Model*, void*))dlsym(hdl, "mpcqp_spec_launch_hessian");
        if (!sl.matches || !sl.step || !sl.hessian || !sl.matches(&d)) sl = SpecLib{};
        else sl.path = so;
    } else {
        fprintf(stderr, "[mpcqp] dlopen(%s) failed: %s\n", so.c_str(), dlerror());
    }
    auto res = g_spec.emplace(key, sl);
    return res.first->second.step ? &res.first->second : nullptr;
}

SpecEntry spec_find(const Dims& d) {
    std::lock_guard<std::mutex> lock(g_spec_mu);
    const SpecLib* sl = find_locked(d);
    return sl ? SpecEntry(*sl) : SpecEntry{};         // (the entry points and flags only: no allocation in a step)
}
// the object `d` is loaded from ("": none), for the callers that work on its files
static std::string loaded_path(const Dims& d, bool* verified = nullptr) {
    std::lock_guard<std::mutex> lock(g_spec_mu);
    const SpecLib* sl = find_locked(d);
    if (sl && verified) *verified = sl->verified;
    return sl ? sl->path : "";
}
static void set_verified(const Dims& d, bool ok) {
    std::lock_guard<std::mutex> lock(g_spec_mu);
    auto it = g_spec.find(spec_key(d));
    if (it != g_spec.end() && it->second.step) { it->second.verified = ok; it->second.no_marker = !ok; }
}
void spec_forget_miss(const Dims& d) {
    std::lock_guard<std::mutex> lock(g_spec_mu);
    auto it = g_spec.find(spec_key(d));
    if (it != g_spec.end() && !it->second.step) g_spec.erase(it);
}

// A freshly built specialisation is checked once against the runtime-dimension kernel (mpcqp_prepare, host side)
// before it is trusted: `<object>.ok` records that it passed, a failing object is renamed `<object>.bad` and never
// loaded again (the local hipcc builds these kernels: a compiler that miscompiles them must not go unnoticed).
bool spec_present(const Dims& d) { return !force_generic() && spec_find(d).step != nullptr; }

bool spec_verified(const Dims& d) {
    bool verified = false;
    const std::string so = loaded_path(d, &verified);
    if (so.empty()) return false;
    if (verified) return true;
    struct stat sb;
    const bool ok = stat((so + ".ok").c_str(), &sb) == 0 || stat(marker_path(so, ".ok").c_str(), &sb) == 0;
    set_verified(d, ok);
    return ok;
}
void mark_spec_verified(const Dims& d) {
    const std::string so = loaded_path(d);
    if (so.empty()) return;
    // (a marker that cannot be written -- read-only cache and no user cache -- only costs the comparison again in the
    //  next process: this process remembers)
    if (FILE* f = fopen(marker_path(so, ".ok").c_str(), "w")) fclose(f);
    set_verified(d, true);
}
// the specialisation a STEP may run: loaded AND verified (mpcqp_prepare's self-test, or the marker of an earlier one);
// an object that some other process, a build pipeline (mpcqp_prebuild) or a prepare without a model put into the cache
// runs only after this machine has compared it with the runtime-dimension kernel.  The marker is looked for once per
// loaded object (and again by every mpcqp_prepare): a step does no file-system work.
SpecEntry spec_find_verified(const Dims& d) {
    const SpecEntry e = spec_find(d);
    if (!e.step || e.verified) return e;
    if (e.no_marker) return SpecEntry{};
    return spec_verified(d) ? e : SpecEntry{};
}

void reject_spec(const Dims& d) {
    const std::string so = loaded_path(d);
    if (!so.empty() && rename(so.c_str(), (so + ".bad").c_str()) != 0) {
        // read-only cache: remember the rejection in this process and, when there is a writable cache, for the next ones
        { std::lock_guard<std::mutex> lock(g_rej_mu); g_rejected.push_back(so); }
        if (FILE* f = fopen(marker_path(so, ".rejected").c_str(), "w")) fclose(f);
    }
    std::lock_guard<std::mutex> lock(g_spec_mu);
    g_spec[spec_key(d)] = SpecLib{};
}

}  // namespace mpcqp
