"""Helpers of tests/test_gpu_team.py and tests/test_isa_hazards.py: the team step kernels (k_step_team<SD, T>, csrc/
mpcqp_devwave.h) at every team size.

The size of the team is a compile-time choice of the on-demand specialisation: `-DMPCQP_TEAM=<T>` in MPCQP_JIT_FLAGS, or
auto_team() without the flag.  The process-wide specialisation cache and the object's file name do not know the JIT flags,
so every variant runs in a FRESH CHILD PROCESS (subprocess.run) with a cache directory of its own:

    python -m tests.team_util run <case> <out.npz>        one case on the GPU, every period's results into the .npz
    python -m tests.team_util prebuild <case>             compile the case's plain-shape object (mpcqp_prebuild; no GPU)

The environment of the child carries MPCQP_CACHE_DIR and MPCQP_JIT_FLAGS."""
from __future__ import annotations

import dataclasses
import glob
import os
import re
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"
VARIANTS = (0, 1, 2, 4)           # 0: no flag, the product default (auto_team)
B_TEAM = 96                       # members per case: several workgroups resident per compute unit
ARRAYS = ("Z", "u0", "status", "iters", "Yhat", "J", "audit")

PATTERNS = {"c3": {}, "all": dict(ymin=-1.2, ymax=1.0, dumin=-0.4, dumax=0.4)}


@dataclasses.dataclass
class Case:
    """One case of the invariance test.  obj: the specialisation it runs on (cases that share one share its cache
    directories); plain: (synth config string, pattern) of a shape mpcqp_prebuild can build ahead (no custom rows, no dense
    weights), else None: the object is compiled inside the child's mpcqp_prepare; auto: the team auto_team() picks;
    timeout: seconds for one child, compilation included."""
    name: str
    obj: str
    auto: int
    nZ: int
    plain: tuple | None = None
    periods: int = 2
    timeout: int = 420
    why: str = ""


CASES = {c.name: c for c in [
    Case("plain71", "plain71", 1, 71, plain=("6,2,2,35,35", "c3"), why="two row slots, five tile rows: helpers with empty or near-empty shares"),
    Case("plain106", "plain106", 2, 106, plain=("12,3,3,40,35", "all"), why="auto T = 2"),
    Case("plain141", "plain141", 4, 141, plain=("12,2,2,70,70", "all"), why="auto T = 4, three rows per lane"),
    Case("plain151", "plain151", 4, 151, plain=("12,3,3,50,50", "c3"), why="auto T = 4, three rows per lane"),
    Case("custom121", "custom121", 2, 121, why="custom-row and terminal-row shares (TJ_WROWS, TJ_XROWS)"),
    Case("custom141", "custom141", 4, 141, why="custom-row and terminal-row shares on a team of four"),
    Case("custom121nb", "custom121nb", 2, 121, why="move blocking: general Toeplitz forms on wavefront 0, matrix-core passes split"),
    Case("dense131", "dense131", 4, 131, why="dense M_Hp, N_Hc, L_Hp: the dense gradient products on a team of four"),
    Case("warmdual141", "plain141", 4, 141, plain=("12,2,2,70,70", "all"), periods=3, why="MPCQP_FLAG_WARM_DUAL closed loop"),
    Case("fused141", "plain141", 4, 141, plain=("12,2,2,70,70", "all"), periods=3, why="mpcqp_loop_device (fused Kalman steps)"),
]}


def plain_config(case):
    from mpcqp import synth
    name, pattern = CASES[case].plain
    return dataclasses.replace(synth.get_config(name), **PATTERNS[pattern])


def row_groups_of(cfg):
    """mpcqp_row_groups of a synth.Config run through parity_util.make_controller (mpcqp_set_bounds, csrc/mpcqp_host.hip): the
    child checks the handle's own answer against this one, so a prebuilt object the handle would not match is an error, not a
    silent second compilation."""
    fin = np.isfinite
    neps = 0 if np.isinf(cfg.Cwt) else 1
    g = 0
    if fin(cfg.dumin) or (neps and not fin(cfg.ymin) and not fin(cfg.ymax)):
        g |= 1 << 0
    if fin(cfg.dumax):
        g |= 1 << 1
    g |= (1 << 2 if fin(cfg.umin) else 0) | (1 << 3 if fin(cfg.umax) else 0)
    g |= (1 << 6 if fin(cfg.ymin) else 0) | (1 << 7 if fin(cfg.ymax) else 0)
    return g


# ---- the code object behind a cached specialisation ---------------------------------------------------------------------------
def device_code_objects(so, workdir):
    """The gfx950 code objects bundled in the shared object `so`, unbundled under `workdir` (llvm-objdump --offloading writes
    next to its input: a copy is unbundled, the original directory is not touched)."""
    os.makedirs(workdir, exist_ok=True)
    cp = os.path.join(workdir, os.path.basename(so))
    shutil.copyfile(so, cp)
    r = subprocess.run([OBJDUMP, "--offloading", cp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cos = sorted(glob.glob(cp + ".*amdgcn*gfx950*"))
    assert cos, f"no gfx950 code object in {so}: {r.stdout[-500:]}"
    return cos


def kernel_symbols(so, workdir):
    """Names of the kernels (symbols with a kernel descriptor `<name>.kd`) of the code objects of `so`."""
    names = []
    for co in device_code_objects(so, workdir):
        r = subprocess.run([OBJDUMP, "-t", co], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        names += [l.split()[-1][:-3] for l in r.stdout.splitlines() if l.strip().endswith(".kd")]
    return names


def team_of_symbols(names):
    """The team size of the step kernel among the kernel names of a specialisation: 1 for k_step_s<...>, T for
    k_step_team<..., T> (the mangled name of the instantiation ends in ...EEELi<T>EEEv...).  Exactly one step kernel."""
    teams = []
    for n in names:
        if re.match(r"^_ZN5mpcqp\d+k_step_teamI", n):
            m = re.search(r"EEELi(\d+)EEEv", n)
            assert m, n
            teams.append(int(m.group(1)))
        elif re.match(r"^_ZN5mpcqp\d+k_step_sI", n):
            teams.append(1)
    assert len(teams) == 1, names
    return teams[0]


def find_cached_objects(pattern):
    """On-demand objects whose file name matches the glob `pattern` in the directories the library searches
    (csrc/spec_cache.cpp search_dirs: MPCQP_CACHE_DIR alone when set, else <library dir>/spec_cache and the user's cache)."""
    if os.environ.get("MPCQP_CACHE_DIR"):
        dirs = [os.environ["MPCQP_CACHE_DIR"]]
    else:
        base = os.environ.get("XDG_CACHE_HOME") or os.path.join(os.environ.get("HOME", ""), ".cache")
        dirs = [os.path.join(ROOT, "modelpredictivecontrol.jl_amd", "lib", "spec_cache"), os.path.join(base, "mpcqp")]
    return sorted(f for d in dirs for f in glob.glob(os.path.join(d, pattern)))


def spec_objects(cache):
    return sorted(f for f in glob.glob(os.path.join(cache, "spec_r*.so")))


# ---- child processes ------------------------------------------------------------------------------------------------------
def child_env(cache, team):
    env = dict(os.environ, MPCQP_CACHE_DIR=cache)
    env.pop("MPCQP_JIT_FLAGS", None)
    if team:
        env["MPCQP_JIT_FLAGS"] = f"-DMPCQP_TEAM={team}"
    return env


def make_cache(root, obj, team):
    """The private cache directory of one (object, team size): owned by this user, not writable by others (the library
    loads from no other kind)."""
    d = os.path.join(root, f"{obj}_T{team}")
    os.makedirs(d, exist_ok=True)
    os.chmod(d, 0o700)
    return d


def prebuild_cmd(case):
    return [sys.executable, "-m", "tests.team_util", "prebuild", case]


def prebuild_plain(case, team, cache, timeout=900):
    """Compile the plain-shape object of `case` at team size `team` into `cache` (child process, no GPU); returns its path."""
    r = subprocess.run(prebuild_cmd(case), cwd=ROOT, env=child_env(cache, team), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    objs = spec_objects(cache)
    assert len(objs) == 1, objs
    return objs[0]


def prebuild_many(jobs, limit=16, timeout=1500):
    """[(case, team, cache)] compiled concurrently, at most `limit` at a time (compilation only: no GPU is opened)."""
    import time
    limit = max(1, min(limit, 16, os.cpu_count() or 1))
    pending, running, t0 = list(jobs), [], time.time()
    while pending or running:
        while pending and len(running) < limit:
            case, team, cache = pending.pop(0)
            if spec_objects(cache):                   # (a cache kept from an earlier run)
                continue
            running.append((case, team, subprocess.Popen(prebuild_cmd(case), cwd=ROOT, env=child_env(cache, team),
                                                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        still = []
        for case, team, pr in running:
            if pr.poll() is None:
                still.append((case, team, pr))
            elif pr.returncode != 0:
                out = pr.stdout.read()
                for _, _, other in running:
                    if other.poll() is None:
                        other.kill()
                raise AssertionError(f"prebuild of {case} at team {team} failed ({pr.returncode}): {out[-3000:]}")
        running = still
        if time.time() - t0 > timeout:
            for _, _, pr in running:
                pr.kill()
            raise AssertionError("prebuilding the plain-shape specialisations timed out")
        time.sleep(0.5)


class ChildDied(Exception):
    """A GPU child ended by a signal, an abort or its time limit: nothing more may be started on the GPU."""


def run_variant(case, team, cache, out, log=None):
    """One case at one team size in a fresh child process; returns the loaded .npz as a dict.  Raises ChildDied when the
    child was killed (signal, abort, time limit), AssertionError when it failed on its own."""
    c = CASES[case]
    try:
        r = subprocess.run([sys.executable, "-m", "tests.team_util", "run", case, out], cwd=ROOT, env=child_env(cache, team),
                           capture_output=True, text=True, timeout=c.timeout)
    except subprocess.TimeoutExpired as e:
        raise ChildDied(f"{case} at team {team}: no end after {c.timeout} s") from e
    tail = r.stdout[-1500:] + r.stderr[-3000:]
    if log is not None:
        log.append((case, team, r.returncode, tail))
    if r.returncode < 0 or r.returncode in (134, 139, 124, 137):
        raise ChildDied(f"{case} at team {team}: child ended with {r.returncode}\n{tail}")
    assert r.returncode == 0, f"{case} at team {team}: exit {r.returncode}\n{tail}"
    with np.load(out) as f:
        return {k: f[k] for k in f.files}


def first_difference(a, b):
    """(period, array, index, value a, value b) of the first entry in which two runs of a case differ, or None."""
    per = int(a["periods"])
    for k in range(per):
        for name in ARRAYS:
            x, y = a[f"p{k}_{name}"], b[f"p{k}_{name}"]
            if x.shape != y.shape:
                return (k, name, "shape", x.shape, y.shape)
            ne = ~((x == y) | (np.isnan(x) & np.isnan(y))) if x.dtype.kind == "f" else x != y
            if ne.any():
                idx = tuple(int(v) for v in np.argwhere(ne)[0])
                return (k, name, idx, x[idx], y[idx])
    return None


# ---- the cases (run inside the child) -----------------------------------------------------------------------------------------
def _save(out, rec, mpc_kind, row_groups, nZ):
    data = {"periods": len(rec), "kind": mpc_kind, "row_groups": row_groups, "nZ": nZ}
    for k, r in enumerate(rec):
        for name in ARRAYS:
            data[f"p{k}_{name}"] = r[name]
    np.savez(out, **data)


def _plain_closed_loop(case, **kw):
    """The plain shapes: B_TEAM different plants, states, set points (synth.make_batch) with the config's bound pattern,
    closed on their own plants for the case's number of periods."""
    from mpcqp import synth
    from tests.parity_util import make_controller, record_period
    cfg = plain_config(case)
    bt = synth.make_batch(cfg, B_TEAM, seed=17)
    mpc = make_controller(cfg, bt, **kw)
    assert mpc.hd.row_groups() == row_groups_of(cfg), (hex(mpc.hd.row_groups()), hex(row_groups_of(cfg)))
    mpc.lastu0 = bt["lastu0"].copy()
    x, rec = bt["xhat0"], []
    rg = np.random.default_rng(3)
    for k in range(CASES[case].periods):
        u = mpc.moveinput(x, bt["ry"], want_info=True)
        rec.append(record_period(mpc))
        x = np.einsum("bij,bj->bi", bt["Ahat"], x) + np.einsum("bij,bj->bi", bt["Bhu"], u) + 0.02 * rg.standard_normal(x.shape)
    return rec, mpc


def _fused_loop(case):
    """mpcqp_loop_device (preparestate! + moveinput! + updatestate! in one launch) on device-resident arrays."""
    import torch
    import mpcqp
    from mpcqp import synth
    cfg = plain_config(case)
    B = B_TEAM
    bt = synth.make_batch(cfg, B, seed=19)
    K = mpcqp.steady_kalman_gain(bt["Ahat"], bt["Chat"], np.eye(cfg.nxh), np.eye(cfg.ny))
    hd = mpcqp.Handle(B, cfg.nxh, cfg.nu, cfg.ny, 0, cfg.Hp, cfg.Hc, neps=1, flags=mpcqp.FLAG_RY_CONSTANT)
    hd.set_model(mpcqp.colmajor(bt["Ahat"]), mpcqp.colmajor(bt["Bhu"]), mpcqp.colmajor(bt["Chat"]))
    hd.set_weights(np.full((B, hd.nY), cfg.Mwt), np.full((B, hd.nDU), cfg.Nwt), np.full((B, hd.nU), cfg.Lwt), np.full(B, cfg.Cwt))
    full = lambda v, n: None if not np.isfinite(v) else np.full((B, n), float(v))
    hd.set_bounds(U0min=full(cfg.umin, hd.nU), U0max=full(cfg.umax, hd.nU), DUmin=full(cfg.dumin, hd.nDU),
                  DUmax=full(cfg.dumax, hd.nDU), Y0min=full(cfg.ymin, hd.nY), Y0max=full(cfg.ymax, hd.nY))
    assert hd.row_groups() == row_groups_of(cfg)
    hd.kf_set(mpcqp.colmajor(K), np.arange(cfg.ny))
    kind = hd.prepare()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    x, lu, ry = dev(bt["xhat0"]), dev(bt["lastu0"]), dev(bt["ry"])
    Z, u0 = dev(np.zeros((B, hd.nZ))), dev(np.zeros((B, cfg.nu)))
    st, it, Yh = dev(np.zeros(B, np.int32)), dev(np.zeros(B, np.int32)), dev(np.zeros((B, hd.nY)))
    rg, rec = np.random.default_rng(7), []
    for k in range(CASES[case].periods):
        y = dev(0.3 * rg.standard_normal((B, cfg.ny)))
        hd.loop_device(x.data_ptr(), y.data_ptr(), lu.data_ptr(), ry.data_ptr(), Z.data_ptr(), u0.data_ptr(), st.data_ptr(),
                       iters=it.data_ptr(), Yhat0=Yh.data_ptr())
        torch.cuda.synchronize()
        # (J: the fused loop has no getinfo; the updated estimate x̂0 takes its place in the record)
        rec.append({"Z": Z.cpu().numpy(), "u0": u0.cpu().numpy(), "status": st.cpu().numpy(), "iters": it.cpu().numpy(),
                    "Yhat": Yh.cpu().numpy(), "J": x.cpu().numpy(), "audit": hd.get(mpcqp.api.GET_AUDIT)})
        assert np.all(rec[-1]["status"] == 0), rec[-1]["status"]
        lu, u0 = u0, lu
    return rec, kind, hd.row_groups(), hd.nZ


def run_case(case, out):
    import mpcqp
    from mpcqp import synth
    from tests import parity_util as pu
    c = CASES[case]
    rec = []
    if case == "fused141":
        rec, kind, rows, nZ = _fused_loop(case)
    elif case.startswith("custom"):
        Hp, Hc = {"custom121": (60, 60), "custom141": (70, 70), "custom121nb": (70, [1] * 55 + [3] * 5)}[case]
        kinds = []
        pu.run_soft_custom_constraints(B=B_TEAM, kinds=kinds, Hp=Hp, Hc=Hc, terminal=True, periods=c.periods, distinct_x0=True,
                                       oracle=False, record=rec)
        kind, rows, nZ = kinds[0], -1, rec[0]["Z"].shape[1]
    elif case == "dense131":
        cfg = synth.Config("dense-team", nx=4, nu=2, ny=2, Hp=70, Hc=65, umin=-0.7, umax=0.7, ymax=0.9)
        _, kind = pu.dense_weight_case(B=B_TEAM, cfg=cfg, periods=c.periods, oracle=False, record=rec)
        rows, nZ = -1, rec[0]["Z"].shape[1]
    else:
        rec, mpc = _plain_closed_loop(case, **(dict(warm_dual=True) if case == "warmdual141" else {}))
        kind, rows, nZ = mpc.hd.kernel_kind(), mpc.hd.row_groups(), mpc.nZ
    assert nZ == c.nZ, (nZ, c.nZ)
    assert len(rec) == c.periods
    for r in rec:
        assert np.all(r["status"] == 0), r["status"]
    _save(out, rec, kind, rows, nZ)
    print(f"[team_util] {case}: kind {kind}, nZ {nZ}, iterations {[float(r['iters'].mean()) for r in rec]}")


def prebuild_case(case):
    from mpcqp import prebuild as pb
    cfg = plain_config(case)
    kind = pb.prebuild(cfg.nu, cfg.ny, cfg.nxh, cfg.Hp, cfg.Hc, neps=0 if np.isinf(cfg.Cwt) else 1, row_groups=row_groups_of(cfg))
    assert kind == 2, kind
    print(f"[team_util] prebuilt {case}")


if __name__ == "__main__":
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    if sys.argv[1] == "run":
        run_case(sys.argv[2], sys.argv[3])
    elif sys.argv[1] == "prebuild":
        prebuild_case(sys.argv[2])
    else:
        raise SystemExit(f"unknown command {sys.argv[1]!r}")
