"""CPU tests of the on-demand specialisation cache (csrc/spec_cache.cpp): object and marker names, the compiler command line,
the trust rules, exact-name-over-foreign lookup and MPCQP_CACHE_STRICT, the remembered miss, verification markers and the
read-only installation.  A stand-alone program (tests/spec_cache_main.cpp) is compiled together with the unit under the
address and undefined-behaviour sanitizers and works on two stand-ins made here: stub objects (g++ -shared, the four entry
points of csrc/mpcqp_spec.hip, the launchers return a fixed number) and a fake compiler (a script that records its arguments
and copies a stub to the path after -o).  No GPU, no hipcc, no sanitizer in Python."""
import os
import re
import shutil
import subprocess

import pytest

import __graft_entry__ as entry
from tests import emu_util

ROOT = emu_util.ROOT
REV = int(re.search(r"#define MPCQP_KERNEL_REV (\d+)", open(os.path.join(emu_util.CSRC, "mpcqp_types.h")).read()).group(1))
DIMS = {"a": "3_2_7_12_4_1_cf_1", "b": "4_4_8_40_17_1_c8c_11"}     # (variant: default_nb | dense_w << 1 | nw << 2)
STUB = """#include "mpcqp_types.h"
using namespace mpcqp;
extern "C" {
int mpcqp_spec_matches(const Dims* d) { return MATCH && d->nu == NU && d->nw == NW; }
int mpcqp_spec_matches_dims(const Dims* d) { return mpcqp_spec_matches(d); }
int mpcqp_spec_launch_step(const Dims*, const Model*, const StepIO*, void*) { return RET; }
int mpcqp_spec_launch_hessian(const Dims*, const Model*, void*) { return RET + 1; }
}
"""


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    """The sanitizer program and the stub objects: a (returns 101), its twin (202), one whose matches() says no, b (303)."""
    d = tmp_path_factory.mktemp("spec_cache_tools")
    exe = str(d / "spec_cache_main")
    subprocess.check_call(emu_util.SANITIZER_CXX + [os.path.join(emu_util.CSRC, "spec_cache.cpp"),
                                                    os.path.join(ROOT, "tests", "spec_cache_main.cpp"), "-ldl", "-o", exe])
    (d / "stub.cpp").write_text(STUB)
    out = {"exe": exe}
    for name, nu, nw, ret, match in (("a", 3, 0, 101, 1), ("twin", 3, 0, 202, 1), ("nomatch", 3, 0, 404, 0), ("b", 4, 2, 303, 1)):
        out[name] = str(d / f"stub_{name}.so")
        subprocess.check_call(["g++", "-shared", "-fPIC", "-I" + emu_util.CSRC, f"-DNU={nu}", f"-DNW={nw}", f"-DRET={ret}",
                               f"-DMATCH={match}", str(d / "stub.cpp"), "-o", out[name]])
        os.chmod(out[name], 0o644)
    return out


def fake_compiler(tmp_path, stub, exit_code=0):
    """An executable that appends its arguments to <tmp_path>/args.txt, one per line, and copies `stub` to the path after -o."""
    path = tmp_path / f"fake_hipcc_{exit_code}"
    path.write_text(f"""#!/bin/sh
for a in "$@"; do printf '%s\\n' "$a" >> '{tmp_path}/args.txt'; done
while [ $# -gt 1 ]; do if [ "$1" = "-o" ]; then cp '{stub}' "$2"; fi; shift; done
exit {exit_code}
""")
    os.chmod(path, 0o755)
    return str(path)


def cache_dir(tmp_path, mode=0o755):
    d = tmp_path / "cache"
    d.mkdir()
    os.chmod(d, mode)          # (whatever the umask)
    return d


def env_of(hipcc, cache=None, **extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MPCQP_")}
    env.update(HIPCC=hipcc, ASAN_OPTIONS="detect_leaks=1", **extra)
    if cache is not None:
        env["MPCQP_CACHE_DIR"] = str(cache)
    return env


def run(exe, which, ops, env):
    out = subprocess.run([exe, which] + [str(o) for o in ops], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines(), out.stderr


def object_name(which, hipcc, monkeypatch):
    monkeypatch.setenv("HIPCC", hipcc)
    return f"spec_r{REV}_c{entry._compiler_id():08x}_{DIMS[which]}.so"


def put(stub, path):
    shutil.copyfile(stub, path)
    os.chmod(path, 0o644)


@pytest.mark.parametrize("which, dims_arg, extra", [
    ("a", "-DMPCQP_SPEC_DIMS=3,2,7,12,4,1,207u,1", []),
    ("b", "-DMPCQP_SPEC_DIMS=4,4,8,40,17,1,3212u,1", ["-DMPCQP_STEP_WAVES=1", "-DMPCQP_SPEC_DENSE=1", "-DMPCQP_SPEC_NW=2"]),
])
def test_object_name_and_compiler_arguments(tools, tmp_path, monkeypatch, which, dims_arg, extra):
    """Cases 1 and 2: the built file is spec_r<rev>_c<compiler id of __graft_entry__>_<dims>_<variant>.so, the compiler got the
    argument list of build_spec (literal, as it stood before the cache became a unit of its own), the log is gone."""
    cache, hipcc = cache_dir(tmp_path), fake_compiler(tmp_path, tools[which])
    lines, err = run(tools["exe"], which, ["build", "find"], env_of(hipcc, cache))
    so = str(cache / object_name(which, hipcc, monkeypatch))
    assert lines == [f"build 0|{so}|", "find " + ("101" if which == "a" else "303")], (lines, err)
    assert sorted(os.listdir(cache)) == [os.path.basename(so)]                 # no .log, no .tmp<pid>
    assert "[mpcqp] specialising the step kernel for nu=" in err and f"(one-time, cached in {cache})" in err
    src = os.path.dirname(tools["exe"]) + "/../csrc"
    args = (tmp_path / "args.txt").read_text().splitlines()
    want = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", "-w", "-I" + src, dims_arg]
    want += extra[:1] + ["-mllvm", "-pragma-unroll-threshold=1048576"] + extra[1:] + [src + "/mpcqp_spec.hip", "-o"]
    assert args[:-1] == want and re.fullmatch(re.escape(so) + r"\.tmp\d+", args[-1]), args


def test_extra_flags_split_on_single_spaces_and_failed_compilation(tools, tmp_path, monkeypatch):
    """Case 2: MPCQP_JIT_FLAGS with two spaces in a row gives exactly two more arguments; a compiler that exits 1 leaves its
    log, no temporary file and no object."""
    cache, hipcc = cache_dir(tmp_path), fake_compiler(tmp_path, tools["a"])
    run(tools["exe"], "a", ["build"], env_of(hipcc, cache, MPCQP_JIT_FLAGS="-DA=1  -DB"))
    args = (tmp_path / "args.txt").read_text().splitlines()
    assert len(args) == 13 + 2 and args[10:12] == ["-DA=1", "-DB"] and args[12].endswith("/mpcqp_spec.hip"), args
    bad_dir = tmp_path / "bad"
    bad_dir.mkdir()
    cache2, failing = cache_dir(bad_dir), fake_compiler(bad_dir, tools["a"], exit_code=1)
    lines, _ = run(tools["exe"], "a", ["build", "find"], env_of(failing, cache2))
    so = str(cache2 / object_name("a", failing, monkeypatch))
    assert lines == [f"build -1|{so}|compiling the specialisation failed (exit 1, see {so}.log)", "find none"]
    assert os.listdir(cache2) == [os.path.basename(so) + ".log"]


def test_untrusted_directory_and_object_are_not_used(tools, tmp_path, monkeypatch):
    """Case 3: a cache directory that group / others can write is not built into and nothing in it is loaded; neither is an
    object that group / others can write."""
    cache, hipcc = cache_dir(tmp_path, 0o775), fake_compiler(tmp_path, tools["a"])
    so = cache / object_name("a", hipcc, monkeypatch)
    put(tools["a"], so)
    lines, err = run(tools["exe"], "a", ["build", "find"], env_of(hipcc, cache))
    assert lines == [f"build -1|{so}|specialisation cache directory '{cache}' is missing, not owned by this user or writable "
                     "by others (set MPCQP_CACHE_DIR)", "find none"]
    assert f"[mpcqp] specialisation cache {cache} is writable by group / others: not used" in err
    assert not (tmp_path / "args.txt").exists()
    os.chmod(cache, 0o755)
    assert run(tools["exe"], "a", ["find"], env_of(hipcc, cache))[0] == ["find 101"]
    os.chmod(so, 0o664)
    assert run(tools["exe"], "a", ["find"], env_of(hipcc, cache))[0] == ["find none"]


def test_exact_name_wins_over_a_foreign_compilers_object(tools, tmp_path, monkeypatch):
    """Case 4: the object of this machine's compiler loads even with another compiler's object of the same shape next to it; the
    foreign one serves without a compiler here and -- unless MPCQP_CACHE_STRICT=1 -- while the local one does not exist."""
    cache, hipcc = cache_dir(tmp_path), fake_compiler(tmp_path, tools["a"])
    exact = cache / object_name("a", hipcc, monkeypatch)
    put(tools["twin"], cache / f"spec_r{REV}_c0badc0de_{DIMS['a']}.so")
    put(tools["a"], exact)
    assert run(tools["exe"], "a", ["find"], env_of(hipcc, cache))[0] == ["find 101"]
    os.remove(exact)
    assert run(tools["exe"], "a", ["find"], env_of(str(tmp_path / "no_such_compiler"), cache))[0] == ["find 202"]
    assert run(tools["exe"], "a", ["find"], env_of(hipcc, cache))[0] == ["find 202"]
    assert run(tools["exe"], "a", ["find"], env_of(hipcc, cache, MPCQP_CACHE_STRICT="1"))[0] == ["find none"]
    assert run(tools["exe"], "a", ["find"], env_of(str(tmp_path / "no_such_compiler"), cache, MPCQP_CACHE_STRICT="1"))[0] == ["find 202"]


def test_a_miss_is_remembered_until_it_is_forgotten(tools, tmp_path, monkeypatch):
    """Case 5: after a miss the cache directory is not looked at again (an object copied in is not seen) until
    spec_forget_miss; an object that does not match its name is an empty entry and is not tried again either."""
    cache, hipcc = cache_dir(tmp_path), fake_compiler(tmp_path, tools["a"])
    so = cache / object_name("a", hipcc, monkeypatch)
    lines, _ = run(tools["exe"], "a", ["find", "cp", tools["a"], so, "find", "present", "forget", "find", "forget", "find"], env_of(hipcc, cache))
    assert lines == ["find none", "cp", "find none", "present 0", "forget", "find 101", "forget", "find 101"]
    put(tools["nomatch"], so)                  # (with a loadable object of another compiler next to it: a second look would find that)
    put(tools["twin"], cache / f"spec_r{REV}_c0badc0de_{DIMS['a']}.so")
    lines, _ = run(tools["exe"], "a", ["find", "rm", so, "find", "forget", "find"], env_of(hipcc, cache))
    assert lines == ["find none", "rm 0", "find none", "forget", "find 202"]


def test_a_step_sees_a_marker_only_through_prepare(tools, tmp_path, monkeypatch):
    """Case 6: a loaded object without a marker is not what a step runs, and the step does not look for the marker again;
    spec_verified (mpcqp_prepare) does.  mark_spec_verified writes <object>.ok next to the object of a writable directory."""
    cache, hipcc = cache_dir(tmp_path), fake_compiler(tmp_path, tools["a"])
    so = cache / object_name("a", hipcc, monkeypatch)
    put(tools["a"], so)
    ops = ["find_verified", "find", "touch", str(so) + ".ok", "find_verified", "verified", "find_verified"]
    lines, _ = run(tools["exe"], "a", ops, env_of(hipcc, cache))
    assert lines == ["find_verified none", "find 101", "touch", "find_verified none", "verified 1", "find_verified 101"]
    os.remove(str(so) + ".ok")
    lines, _ = run(tools["exe"], "a", ["verified", "find_verified", "mark", "find_verified", "verified"], env_of(hipcc, cache))
    assert lines == ["verified 0", "find_verified none", "mark", "find_verified 101", "verified 1"]
    assert sorted(os.listdir(cache)) == [so.name, so.name + ".ok"]
    assert run(tools["exe"], "a", ["find_verified"], env_of(hipcc, cache))[0] == ["find_verified 101"]     # (the next process)


def test_read_only_installation_keeps_its_markers_in_the_users_cache(tools, tmp_path, monkeypatch):
    """Case 7: MPCQP_CACHE_DIR unset, the object in <program dir>/spec_cache with mode 0555: the .ok marker goes to
    $XDG_CACHE_HOME/mpcqp, a rejected object cannot be renamed and leaves <name>.rejected there, and is not found again in
    this process nor in the next."""
    if os.geteuid() == 0:
        pytest.skip("root writes into a directory of mode 0555: the object's own directory would take the markers and the rename")
    inst, xdg = tmp_path / "inst", tmp_path / "xdg"
    inst.mkdir(), xdg.mkdir()
    exe, hipcc = shutil.copy2(tools["exe"], inst / "spec_cache_main"), fake_compiler(tmp_path, tools["a"])
    local = inst / "spec_cache"
    local.mkdir()
    name = object_name("a", hipcc, monkeypatch)
    put(tools["a"], local / name)
    os.chmod(local, 0o555)
    env = env_of(hipcc, XDG_CACHE_HOME=str(xdg))
    try:
        lines, _ = run(exe, "a", ["find", "mark", "find_verified"], env)
        assert lines == ["find 101", "mark", "find_verified 101"]
        assert os.listdir(xdg / "mpcqp") == [name + ".ok"] and os.listdir(local) == [name]
        lines, _ = run(exe, "a", ["find_verified", "reject", "find", "forget", "find"], env)
        assert lines == ["find_verified 101", "reject", "find none", "forget", "find none"]
        assert sorted(os.listdir(xdg / "mpcqp")) == [name + ".ok", name + ".rejected"] and os.listdir(local) == [name]
        assert run(exe, "a", ["find"], env)[0] == ["find none"]
    finally:
        os.chmod(local, 0o755)


def test_rejected_object_of_a_writable_cache_is_renamed(tools, tmp_path, monkeypatch):
    """Case 8: reject_spec renames the object to <object>.bad; it is not found again."""
    cache, hipcc = cache_dir(tmp_path), fake_compiler(tmp_path, tools["a"])
    so = cache / object_name("a", hipcc, monkeypatch)
    put(tools["a"], so)
    lines, _ = run(tools["exe"], "a", ["find", "reject", "find", "forget", "find"], env_of(hipcc, cache))
    assert lines == ["find 101", "reject", "find none", "forget", "find none"]
    assert os.listdir(cache) == [so.name + ".bad"]
