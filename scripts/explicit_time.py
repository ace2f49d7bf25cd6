"""Timing of the batched ExplicitMPC against the step it replaces, on resident data (HIP events around the launches, median of
10 after 3 warm-ups), C3 dimensions without bounds and with Cwt = Inf:
  (a) `step`      mpcqp_step_device on that handle -- the interior-point kernel's closed-form path, which reloads H̃ and runs a
                  full Cholesky every period.  Every library has it: with --lib PATH this measures the yardstick on a build of
                  the parent commit (MPCQP_LIB);
  (b) `ex_inv`    mpcqp_explicit_step_device: the product with the stored H̃⁻¹ (the form with two substitutions on the stored
                  factor was measured once and dropped);
  (c) `law_z`     mpcqp_explicit_law_device with Z̃;
  (d) `law_u`     ... for u0 alone, with bytes per controller and the achieved TB/s.
One JSON line per measurement.  `python scripts/explicit_time.py compare PARENT_LIB [B ...]` runs parent and tree in fresh child
processes, alternating, two passes each; `big` adds a u0-only batch whose tables (832 B per controller) exceed the 256 MiB
Infinity Cache.  Usage: python scripts/explicit_time.py [compare PARENT_LIB | --lib PATH] [big] [B ...]   (default B: 65536 1024)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM, REPS = 3, 10
BIG_B = 524288


def timed(fn, torch):
    s = torch.cuda.current_stream()
    for _ in range(WARM):
        fn(s.cuda_stream)
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s); fn(s.cuda_stream); e1.record(s)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def measure(B, tag, only_law_u=False):
    import torch
    import mpcqp
    from mpcqp import synth
    cfg = synth.C3
    dev = torch.device("cuda", 0)
    if only_law_u:          # the models of a small batch, repeated: the tables are what has to exceed the cache
        bt = synth.make_batch(cfg, 4096, seed=0)
        bt = {k: (np.tile(v, (B // 4096,) + (1,) * (v.ndim - 1)) if isinstance(v, np.ndarray) else v) for k, v in bt.items()}
    else:
        bt = synth.make_batch(cfg, B, seed=0)
    mpc = mpcqp.BatchLinMPC(bt["Ahat"], bt["Bhu"], bt["Chat"], Hp=cfg.Hp, Hc=cfg.Hc, Cwt=np.inf)
    hd = mpc.hd
    hd.set_flags(hd.flags | mpcqp.FLAG_RY_CONSTANT)
    t = lambda a, dt=torch.float64: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    x, lu, ry = t(bt["xhat0"]), t(bt["lastu0"]), t(bt["ry"])
    Z, u0 = torch.zeros(B, mpc.nZ, dtype=torch.float64, device=dev), torch.zeros(B, cfg.nu, dtype=torch.float64, device=dev)
    st, it = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    p = lambda a: a.data_ptr()
    out = lambda name, ms, **kw: print(json.dumps(dict(lib=tag, B=B, what=name, ms=round(ms[0], 5), ms_min=round(ms[1], 5),
                                                       per_s=round(B / ms[0] * 1e3), **kw)), flush=True)
    if not only_law_u:
        kind = hd.prepare()
        out("step", timed(lambda s: hd.step_device(p(x), p(lu), p(ry), p(Z), p(u0), p(st), iters=p(it), stream=s), torch), kernel_kind=kind)
        Zstep = Z.cpu().numpy()
    if not hasattr(hd.lib, "mpcqp_explicit_prepare"):
        return
    n, nin = mpc.nZ, cfg.nxh + cfg.nu + cfg.ny
    kp = (1 + nin + 1) // 2
    if not only_law_u:
        hd.explicit_prepare(law=True)
        out("ex_inv", timed(lambda s: hd.explicit_step_device(p(x), p(lu), p(ry), p(Z), p(u0), p(st), stream=s), torch),
            # packed H̃⁻¹, K, Σ, Mdiag, Lsum, inputs, Z̃, u0, two status words (B = 0 and the horizon of L are not read here)
            bytes_per_controller=8 * (n * (n + 1) // 2 + cfg.nxh * mpc.nY + cfg.Hp * cfg.ny * cfg.nu + mpc.nY + n + nin + n + cfg.nu) + 8,
            max_abs_diff_vs_step=float(np.abs(Z.cpu().numpy() - Zstep).max()))
        out("law_z", timed(lambda s: hd.explicit_law_device(p(x), p(lu), p(ry), p(u0), p(st), Z=p(Z), stream=s), torch),
            bytes_per_controller=8 * (n * 2 * kp + nin + n + cfg.nu) + 8,
            max_abs_diff_vs_step=float(np.abs(Z.cpu().numpy() - Zstep).max()))
    else:
        hd.explicit_prepare(law=True)
    by = 8 * (cfg.nu * 2 * kp + nin + cfg.nu) + 8
    ms = timed(lambda s: hd.explicit_law_device(p(x), p(lu), p(ry), p(u0), p(st), stream=s), torch)
    out("law_u", ms, bytes_per_controller=by, TB_per_s=round(B * by / ms[0] * 1e-9, 3), table_MB=round(B * cfg.nu * 2 * kp * 8 / 1e6, 1))


def main():
    args = sys.argv[1:]
    if args and args[0] == "compare":
        parent, rest = os.path.abspath(args[1]), args[2:]
        me = os.path.abspath(__file__)
        # one cache of on-demand step kernels for both (the kernel sources and the compiler are the same): the caller's
        # MPCQP_CACHE_DIR, else a temporary directory -- nothing is written into the source tree
        with tempfile.TemporaryDirectory(prefix="mpcqp_spec_") as tmp:
            env = dict(os.environ, MPCQP_CACHE_DIR=os.environ.get("MPCQP_CACHE_DIR") or tmp)
            for p_ in range(2):                 # parent, tree, parent, tree: one fresh child process each, one at a time
                for lib in (parent, None):
                    cmd = [sys.executable, me] + (["--lib", lib] if lib else []) + rest
                    subprocess.run(cmd, check=True, timeout=600, env=env)
        return
    tag = "tree"
    if args and args[0] == "--lib":
        os.environ["MPCQP_LIB"] = args[1]
        tag, args = os.path.basename(args[1]), args[2:]
    big = "big" in args
    Bs = [int(a) for a in args if a.isdigit()] or [65536, 1024]
    for B in Bs:
        measure(B, tag)
    if big and tag == "tree":
        measure(BIG_B, tag, only_law_u=True)


if __name__ == "__main__":
    main()
