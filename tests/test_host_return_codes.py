"""Which code every entry point of csrc/mpcqp_host.hip returns in which state of the handle: the integers the raw ctypes
functions answer on tiny handles (B = 2, nx̂ = 3, nu = 1, ny = 2, Hp = 4, Hc = 2, once without and once with a measured
disturbance) against the literal table EXPECTED at the end of this file.  The table pins the order of the checks inside an
entry point (which refusal wins) and which estimator sits behind the handle after every setter; it was recorded from the
library as it stood before the estimator kind became one field (`python -m tests.test_host_return_codes` prints the table
of the library at hand), and a change of the host code that moves one entry fails here.  The CPU test runs on tests/emu/libmpcqp_emu_all.so
(tests/emu/all.mk: every launcher that csrc/*_launch.h declares weak is present, so nothing answers MPCQP_ERR_UNSUPPORTED for
want of one), the `gpu` twin runs the same calls on the product library; both read the same table.  The read-back of K1's
remaining tables (MPCQP_GET_GDTAB .. MPCQP_GET_BXHAT) and mpcqp_predmat_form have a table of their own, EXPECTED_K1, written
from the header's contract and keyed by nd, since Gd and Xd answer MPCQP_ERR_ARG without a measured disturbance."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import mpcqp
from mpcqp import mhe as mhe_api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
B, NX, NU, NY, HP, HC, NYM = 2, 3, 1, 2, 4, 2, 2
STATES = ("none", "gain", "tv", "steady", "place", "mhe", "im")
GETS = {"cov": 10, "gain": 11, "im_xs": 13, "im_ys": 14, "im_yhats": 15}


def build():
    """make tests/emu/libmpcqp_emu_all.so (tests/emu/all.mk); returns its path."""
    subprocess.check_call(["make", "-s", "-j8", "-C", EMU, "-f", "all.mk", "libmpcqp_emu_all.so"])
    return os.path.join(EMU, "libmpcqp_emu_all.so")


def p(a):
    return None if a is None else a.ctypes.data


def eye(n):
    """(n,n,B): the identity in every member"""
    return np.ascontiguousarray(np.broadcast_to(np.eye(n), (B, n, n)))


def i32(*v):
    return np.array(v, dtype=np.int32)


class Rig:
    """One handle of the tiny shape and the arrays its calls need (kept alive here: the library reads them during the call)."""

    def __init__(self, lib, nd, model=True, weights=True):
        self.lib, self.nd = mhe_api._bind(lib), nd
        self.h, self.e = C.c_void_p(), C.c_void_p()
        dims = mpcqp.api.Dims(B, NX, NU, NY, nd, HP, HC, None, 0, 0, 0, 0, 0.0, 0.0, 0.0)
        assert lib.mpcqp_create(C.byref(dims), C.byref(self.h)) == 0
        rng = np.random.default_rng(7)
        # column-major members: A stable and with distinct eigenvalues, (A, C) observable
        self.A = np.ascontiguousarray(np.stack([np.diag([0.5, 0.6, 0.7]) + 0.05 * rng.standard_normal((NX, NX)) for _ in range(B)]))
        self.Bu = rng.standard_normal((B, NU, NX))
        self.Cm = rng.standard_normal((B, NX, NY))
        self.Bd = rng.standard_normal((B, max(nd, 1), NX)) if nd else None
        self.Dd = rng.standard_normal((B, max(nd, 1), NY)) if nd else None
        self.M, self.N, self.L = np.ones((B, NY * HP)), 0.1 * np.ones((B, NU * HC)), np.zeros((B, NU * HP))
        self.x, self.u, self.y = np.zeros((B, NX)), np.zeros((B, NU)), np.zeros((B, NYM))
        self.d0 = np.zeros((B, nd)) if nd else None
        self.Dh = np.zeros((B, nd * HP)) if nd else None
        self.ry, self.Z = np.zeros((B, NY * HP)), np.zeros((B, NU * HC))
        self.st, self.it = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self.K = np.zeros((B, NYM, NX))
        self.Q, self.R, self.P0 = eye(NX), eye(NYM), eye(NX)
        self.poles = np.ascontiguousarray(np.broadcast_to([0.1, 0.2, 0.3], (B, NX)))
        self.iym = i32(0, 1)
        self.big = np.zeros(4096)
        if model:
            assert self.set_model() == 0
        if weights:
            assert self.set_weights() == 0

    def close(self):
        self.lib.mpcqp_destroy(self.h)
        if self.e:
            self.lib.mpcqp_mhe_destroy(self.e)

    def set_model(self):
        return self.lib.mpcqp_set_model(self.h, p(self.A), p(self.Bu), p(self.Cm), p(self.Bd), p(self.Dd), None)

    def set_weights(self):
        return self.lib.mpcqp_set_weights(self.h, p(self.M), p(self.N), p(self.L), None)

    def estimator(self):
        """a real MovingHorizonEstimator handle of matching dimensions"""
        if not self.e:
            dims = mhe_api.MheDims(B, NX, NU, NYM, self.nd, 2, 1, 0, 0, 0, 0.0, 0.0, 0.0)
            assert self.lib.mpcqp_mhe_create(C.byref(dims), C.byref(self.e)) == 0
        return self.e

    # ---- the setters that reach the seven states, and the calls that must leave the state alone
    def enter(self, state):
        lib, h, iym = self.lib, self.h, p(self.iym)
        if state == "none":
            return lib.mpcqp_mhe_attach(h, None, None, 0)      # (detaches: MHE becomes none, anything else stays)
        if state == "gain":
            return lib.mpcqp_kf_set(h, p(self.K), iym, NYM)
        if state == "tv":
            return lib.mpcqp_kf_set_covariances(h, p(self.Q), p(self.R), p(self.P0), iym, NYM)
        if state == "tv_no_p0":
            return lib.mpcqp_kf_set_covariances(h, p(self.Q), p(self.R), None, iym, NYM)
        if state == "tv_no_p0_other_nym":
            return lib.mpcqp_kf_set_covariances(h, p(self.Q), p(eye(1)), None, iym, 1)
        if state == "steady":
            return lib.mpcqp_kf_set_steady(h, p(self.Q), p(self.R), iym, NYM)
        if state == "place":
            return lib.mpcqp_kf_set_poles(h, p(self.poles), iym, NYM)
        if state == "mhe":
            return lib.mpcqp_mhe_attach(h, self.estimator(), iym, NYM)
        if state == "im":
            return lib.mpcqp_im_set(h, 0, None, None, None, None, iym, NYM)
        if state == "im_refused":                               # two of the four matrices: MPCQP_ERR_ARG, nothing changes
            return lib.mpcqp_im_set(h, NYM, p(eye(NYM)), p(eye(NYM)), None, None, iym, NYM)
        raise KeyError(state)

    def signature(self):
        """what tells the seven states apart: the status getters and the lanes of the covariance kernel"""
        lib, h, st = self.lib, self.h, p(self.st)
        return {"kf_status": lib.mpcqp_kf_status(h, st), "im_status": lib.mpcqp_im_status(h, st),
                "sim_est_status": lib.mpcqp_sim_est_status(h, st, 1), "steady_iters": lib.mpcqp_kf_steady_iters(h, st),
                "place_sweeps": lib.mpcqp_kf_place_sweeps(h, st), "get_gain": lib.mpcqp_get(h, GETS["gain"], p(self.big)),
                "get_cov": lib.mpcqp_get(h, GETS["cov"], p(self.big)), "get_im_xs": lib.mpcqp_get(h, GETS["im_xs"], p(self.big)),
                "est_initstate": lib.mpcqp_est_initstate(h, p(self.x), p(self.u), p(self.y), p(self.d0), st),
                "lanes": lib.mpcqp_kf_lanes_per_estimator(h)}

    def probe(self):
        """every estimator entry point, in the order of the issue's list"""
        lib, h, st = self.lib, self.h, p(self.st)
        x, u, y, d0 = p(self.x), p(self.u), p(self.y), p(self.d0)
        out = {}
        out["kf_status"] = lib.mpcqp_kf_status(h, st)
        out["kf_status(out=NULL)"] = lib.mpcqp_kf_status(h, None)
        out["kf_steady_iters"] = lib.mpcqp_kf_steady_iters(h, st)
        out["kf_steady_path"] = lib.mpcqp_kf_steady_path(h, st)
        out["kf_place_sweeps"] = lib.mpcqp_kf_place_sweeps(h, st)
        out["kf_set_place_cap(5)"] = lib.mpcqp_kf_set_place_cap(h, 5)
        out["kf_set_place_cap(-1)"] = lib.mpcqp_kf_set_place_cap(h, -1)
        out["kf_lanes_per_estimator"] = lib.mpcqp_kf_lanes_per_estimator(h)
        out["kf_set_state_covariance"] = lib.mpcqp_kf_set_state_covariance(h, p(self.P0))
        out["kf_set_state_covariance(P=NULL)"] = lib.mpcqp_kf_set_state_covariance(h, None)
        out["kf_set_direct(0)"] = lib.mpcqp_kf_set_direct(h, 0)
        out["kf_set_direct(1)"] = lib.mpcqp_kf_set_direct(h, 1)
        out["kf_set_direct(2)"] = lib.mpcqp_kf_set_direct(h, 2)
        out["kf_solve_steady"] = lib.mpcqp_kf_solve_steady(h)
        out["kf_place"] = lib.mpcqp_kf_place(h)
        out["kf_correct"] = lib.mpcqp_kf_correct(h, x, y, d0)
        out["kf_correct(y0m=NULL)"] = lib.mpcqp_kf_correct(h, x, None, d0)
        out["kf_correct(xhat0=NULL)"] = lib.mpcqp_kf_correct(h, None, y, d0)
        out["kf_predict"] = lib.mpcqp_kf_predict(h, x, u, d0)
        out["kf_predict(u0=NULL)"] = lib.mpcqp_kf_predict(h, x, None, d0)
        out["kf_update"] = lib.mpcqp_kf_update(h, x, u, y, d0)
        out["kf_update(y0m=NULL)"] = lib.mpcqp_kf_update(h, x, u, None, d0)
        out["kf_update(u0=NULL)"] = lib.mpcqp_kf_update(h, x, None, y, d0)
        out["im_status"] = lib.mpcqp_im_status(h, st)
        out["im_status(out=NULL)"] = lib.mpcqp_im_status(h, None)
        out["im_correct"] = lib.mpcqp_im_correct(h, x, y, d0)
        out["im_correct(y0m=NULL)"] = lib.mpcqp_im_correct(h, x, None, d0)
        out["im_update"] = lib.mpcqp_im_update(h, x, u, d0)
        out["est_initstate"] = lib.mpcqp_est_initstate(h, x, u, y, d0, st)
        out["est_initstate(status=NULL)"] = lib.mpcqp_est_initstate(h, x, u, y, d0, None)
        for name, which in GETS.items():
            out["get(%s)" % name] = lib.mpcqp_get(h, which, p(self.big))
        out["sim_path"] = lib.mpcqp_sim_path(h)
        out["sim_est_status"] = lib.mpcqp_sim_est_status(h, st, 1)
        out["loop_device(y0m=NULL)"] = lib.mpcqp_loop_device(h, x, None, u, p(self.ry), None, d0, p(self.Dh), p(self.Z), u, st,
                                                              p(self.it), None, None)
        return out

    def probe_without_d0(self):
        """a measured disturbance, and no d0"""
        lib, h, x, u, y = self.lib, self.h, p(self.x), p(self.u), p(self.y)
        return {"kf_correct": lib.mpcqp_kf_correct(h, x, y, None), "kf_predict": lib.mpcqp_kf_predict(h, x, u, None),
                "kf_update": lib.mpcqp_kf_update(h, x, u, y, None), "im_correct": lib.mpcqp_im_correct(h, x, y, None),
                "im_update": lib.mpcqp_im_update(h, x, u, None),
                "est_initstate": lib.mpcqp_est_initstate(h, x, u, y, None, p(self.st))}

    def step(self):
        return self.lib.mpcqp_step(self.h, p(self.x), p(self.u), p(self.ry), None, p(self.d0), p(self.Dh), p(self.Z), p(self.u),
                                   p(self.st), p(self.it), None)

    def explicit_step(self):
        return self.lib.mpcqp_explicit_step(self.h, p(self.x), p(self.u), p(self.ry), None, p(self.d0), p(self.Dh), p(self.Z),
                                            p(self.u), p(self.st), None)


def states(lib, nd, without_d0=False):
    """the estimator entry points in every state, with and without a resident model (the steady and the pole setters need one)"""
    out = {}
    for model in (True, False):
        for s in STATES:
            if not model and s in ("steady", "place"):
                continue
            r = Rig(lib, nd, model=model, weights=model)
            key = "%s/%s" % (s, "model" if model else "no model")
            out[key] = {"enter": r.enter(s)}
            out[key].update(r.probe_without_d0() if without_d0 else r.probe())
            r.close()
    return out


def transitions(lib, nd):
    """all ordered pairs of states, the detach and the refused calls from each: the code of the second setter and the state after it"""
    out = {}
    for a in STATES:
        for b in STATES + ("im_refused", "tv_no_p0", "tv_no_p0_other_nym"):
            r = Rig(lib, nd)
            first = r.enter(a)
            out["%s -> %s" % (a, b)] = dict(first=first, second=r.enter(b), **r.signature())
            r.close()
    return out


def arguments(lib, nd):
    out = {}
    # the six takers of i_ym: the bounds of nym, an index outside 0 .. ny-1, a duplicate
    bad = {"nym=0": (i32(0, 1), 0), "nym=ny+1": (i32(0, 1, 0), NY + 1), "index -1": (i32(0, -1), 2), "index ny": (i32(NY, 0), 2),
           "duplicate": (i32(1, 1), 2)}
    for name, (iym, nym) in bad.items():
        r = Rig(lib, nd)
        lib_, h, q = r.lib, r.h, p(iym)
        R = eye(max(nym, 1))
        out["i_ym %s" % name] = {
            "kf_set": lib_.mpcqp_kf_set(h, p(r.big), q, nym),
            "kf_set_covariances": lib_.mpcqp_kf_set_covariances(h, p(r.Q), p(R), p(r.P0), q, nym),
            "kf_set_steady": lib_.mpcqp_kf_set_steady(h, p(r.Q), p(R), q, nym),
            "kf_set_poles": lib_.mpcqp_kf_set_poles(h, p(r.poles), q, nym),
            "im_set": lib_.mpcqp_im_set(h, 0, None, None, None, None, q, nym),
            "mhe_attach": lib_.mpcqp_mhe_attach(h, r.estimator(), q, nym)}
        out["i_ym %s" % name].update({"after: " + k: v for k, v in r.signature().items() if k in ("kf_status", "im_status", "get_gain", "est_initstate")})
        r.close()
    # every required pointer NULL in turn; P0 NULL on a handle that is not, and one that is, time-varying
    r = Rig(lib, nd)
    lib_, h, Q, R, P0, iym, po = r.lib, r.h, p(r.Q), p(r.R), p(r.P0), p(r.iym), p(r.poles)
    nonsym = eye(NX)
    nonsym[:, 0, 1] = 0.5
    unit = r.poles.copy()
    unit[1, 2] = -1.0
    nul = out["null / value"] = {}
    nul["kf_set_covariances(Q=NULL)"] = lib_.mpcqp_kf_set_covariances(h, None, R, P0, iym, NYM)
    nul["kf_set_covariances(R=NULL)"] = lib_.mpcqp_kf_set_covariances(h, Q, None, P0, iym, NYM)
    nul["kf_set_covariances(i_ym=NULL)"] = lib_.mpcqp_kf_set_covariances(h, Q, R, P0, None, NYM)
    nul["kf_set_covariances(P0=NULL) not time-varying"] = lib_.mpcqp_kf_set_covariances(h, Q, R, None, iym, NYM)
    nul["kf_set_covariances(Q not symmetric)"] = lib_.mpcqp_kf_set_covariances(h, p(nonsym), R, P0, iym, NYM)
    nul["kf_set_covariances(P0 not symmetric)"] = lib_.mpcqp_kf_set_covariances(h, Q, R, p(nonsym), iym, NYM)
    nul["kf_set_covariances"] = lib_.mpcqp_kf_set_covariances(h, Q, R, P0, iym, NYM)
    nul["kf_set_covariances(P0=NULL) time-varying"] = lib_.mpcqp_kf_set_covariances(h, Q, R, None, iym, NYM)
    nul["kf_set_covariances(P0=NULL, Q not symmetric) time-varying"] = lib_.mpcqp_kf_set_covariances(h, p(nonsym), R, None, iym, NYM)
    nul["kf_set_steady(Q=NULL)"] = lib_.mpcqp_kf_set_steady(h, None, R, iym, NYM)
    nul["kf_set_steady(R=NULL)"] = lib_.mpcqp_kf_set_steady(h, Q, None, iym, NYM)
    nul["kf_set_steady(i_ym=NULL)"] = lib_.mpcqp_kf_set_steady(h, Q, R, None, NYM)
    nul["kf_set_steady(Q not symmetric)"] = lib_.mpcqp_kf_set_steady(h, p(nonsym), R, iym, NYM)
    nul["kf_set_poles(poles=NULL)"] = lib_.mpcqp_kf_set_poles(h, None, iym, NYM)
    nul["kf_set_poles(i_ym=NULL)"] = lib_.mpcqp_kf_set_poles(h, po, None, NYM)
    nul["kf_set_poles(|pole| = 1)"] = lib_.mpcqp_kf_set_poles(h, p(unit), iym, NYM)
    nul["after: kf_status"] = lib_.mpcqp_kf_status(h, p(r.st))       # (still the time-varying filter: every refusal left it alone)
    nul["after: lanes"] = lib_.mpcqp_kf_lanes_per_estimator(h)
    nul["kf_set(Khat=NULL)"] = lib_.mpcqp_kf_set(h, None, iym, NYM)
    nul["mhe_attach(i_ym=NULL)"] = lib_.mpcqp_mhe_attach(h, r.estimator(), None, NYM)
    nul["im_set(i_ym=NULL)"] = lib_.mpcqp_im_set(h, 0, None, None, None, None, None, NYM)
    nul["im_set(nxs=0, given)"] = lib_.mpcqp_im_set(h, 0, p(r.big), p(r.big), p(r.big), p(r.big), iym, NYM)
    r.close()
    # before mpcqp_set_model: the argument error wins over MPCQP_ERR_ORDER
    r = Rig(lib, nd, model=False, weights=False)
    lib_, h, Q, R, iym, po = r.lib, r.h, p(r.Q), p(r.R), p(r.iym), p(r.poles)
    o = out["before the model"] = {}
    o["kf_set_steady"] = lib_.mpcqp_kf_set_steady(h, Q, R, iym, NYM)
    o["kf_set_steady(Q not symmetric)"] = lib_.mpcqp_kf_set_steady(h, p(nonsym), R, iym, NYM)
    o["kf_set_steady(duplicate)"] = lib_.mpcqp_kf_set_steady(h, Q, R, p(i32(1, 1)), NYM)
    o["kf_set_poles"] = lib_.mpcqp_kf_set_poles(h, po, iym, NYM)
    o["kf_set_poles(|pole| = 1)"] = lib_.mpcqp_kf_set_poles(h, p(unit), iym, NYM)
    o["kf_solve_steady"] = lib_.mpcqp_kf_solve_steady(h)
    o["kf_place"] = lib_.mpcqp_kf_place(h)
    # the step and the explicit calls before the model, before the weights, before mpcqp_explicit_prepare, and after it
    st = p(r.st)
    for stage in ("before the model", "before the weights", "before explicit_prepare", "prepared"):
        o = out.setdefault(stage, {})
        o["step"] = r.step()
        o["explicit_step"] = r.explicit_step()
        o["explicit_status"] = lib_.mpcqp_explicit_status(h, st)
        o["explicit_status(out=NULL)"] = lib_.mpcqp_explicit_status(h, None)
        if stage != "prepared":
            o["set_output_weight_blocks"] = lib_.mpcqp_set_output_weight_blocks(h, None)
            o["set_dense_weights"] = lib_.mpcqp_set_dense_weights(h, None, None, None)
            o["set_custom_bounds"] = lib_.mpcqp_set_custom_bounds(h, p(r.big), None, None, None)
            o["explicit_prepare(2)"] = lib_.mpcqp_explicit_prepare(h, 2)
        o["next"] = {"before the model": r.set_model, "before the weights": r.set_weights,
                     "before explicit_prepare": lambda: lib_.mpcqp_explicit_prepare(h, 0), "prepared": lambda: 0}[stage]()
    o = out["prepared"]
    o["im_set"] = lib_.mpcqp_im_set(h, 0, None, None, None, None, iym, NYM)       # (no InternalModel on a prepared handle)
    o["after: im_status"] = lib_.mpcqp_im_status(h, st)
    r.close()
    # custom rows: the bounds after the constraints; no InternalModel with them, and none of them on an InternalModel
    r = Rig(lib, nd)
    lib_, h, iym = r.lib, r.h, p(r.iym)
    o = out["custom rows"] = {}
    Wy, Wu = np.ones((B, NY, 1)), np.ones((B, NU, 1))
    o["set_custom_bounds before the constraints"] = lib_.mpcqp_set_custom_bounds(h, p(r.big), None, None, None)
    o["im_set"] = lib_.mpcqp_im_set(h, 0, None, None, None, None, iym, NYM)
    o["set_custom_constraints on an InternalModel"] = lib_.mpcqp_set_custom_constraints(h, 1, p(Wy), p(Wu), None, None, None)
    o["kf_set"] = lib_.mpcqp_kf_set(h, p(r.K), iym, NYM)
    o["set_custom_constraints"] = lib_.mpcqp_set_custom_constraints(h, 1, p(Wy), p(Wu), None, None, None)
    o["set_custom_bounds"] = lib_.mpcqp_set_custom_bounds(h, p(r.big), None, None, None)
    o["set_custom_bounds(C_wmin without a slack)"] = lib_.mpcqp_set_custom_bounds(h, p(r.big), None, p(r.big), None)
    o["im_set with custom rows"] = lib_.mpcqp_im_set(h, 0, None, None, None, None, iym, NYM)
    o["after: get_gain"] = lib_.mpcqp_get(h, GETS["gain"], p(r.big))
    o["step"] = r.step()
    r.close()
    # every `which` of mpcqp_get on a fresh handle
    r = Rig(lib, nd, model=False, weights=False)
    out["get on a fresh handle"] = {str(w): r.lib.mpcqp_get(r.h, w, p(r.big)) for w in range(0, 30)}
    out["get on a fresh handle"]["out=NULL"] = r.lib.mpcqp_get(r.h, 1, None)
    r.close()
    return out


K1_GETS = {"gdtab": 22, "xdtab": 23, "exhat": 24, "kxhat": 25, "bxhat": 26}


def k1_tables(lib, nd):
    """mpcqp_get of K1's remaining tables and mpcqp_predmat_form: before the model, with it, once a finite x̂ bound had the
    terminal tables built, and on a handle that only the stage-structured kernel takes (nZ̃ = 300: nothing is condensed)"""
    out = {}
    r = Rig(lib, nd, model=False, weights=False)
    gets = lambda h: {name: r.lib.mpcqp_get(h, which, p(r.big)) for name, which in K1_GETS.items()}
    out["before the model"] = gets(r.h)
    assert r.set_model() == 0 and r.set_weights() == 0
    out["model"] = gets(r.h)
    b, x0max = mpcqp.api.Bounds(), np.full((B, NX), 50.0)
    b.x0max = x0max.ctypes.data_as(C.POINTER(C.c_double))
    out["model"]["set_bounds(x0max)"] = r.lib.mpcqp_set_bounds(r.h, C.byref(b))
    out["terminal tables built"] = gets(r.h)
    out["terminal tables built"]["set_model"] = r.set_model()
    out["after another set_model"] = gets(r.h)
    out["predmat_form"] = {"h=NULL": r.lib.mpcqp_predmat_form(None), "tiny handle": r.lib.mpcqp_predmat_form(r.h)}
    r.close()
    h = C.c_void_p()
    dims = mpcqp.api.Dims(B, NX, NU, NY, nd, 300, 300, None, 0, 0, 0, 0, 0.0, 0.0, 0.0)
    assert lib.mpcqp_create(C.byref(dims), C.byref(h)) == 0
    out["stage-only handle"] = gets(h)
    lib.mpcqp_destroy(h)
    return out


def rows(section):
    """{row: {column: code}} as (columns, {row: codes}): one line of the table per row"""
    cols = tuple(next(iter(section.values())))
    assert all(tuple(r) == cols for r in section.values())
    return cols, {k: tuple(r.values()) for k, r in section.items()}


def record(lib, nd):
    out = {"states": rows(states(lib, nd)), "transitions": rows(transitions(lib, nd)), "arguments": arguments(lib, nd)}
    if nd:
        out["states without d0"] = rows(states(lib, nd, without_d0=True))
    return out


def show(t):
    """the table as the Python text of EXPECTED below"""
    out = ["{"]
    for sec in ("states", "states without d0", "transitions"):
        out += ['    "%s": (%r, {' % (sec, t[sec][0])] + ["        %r: %r," % kv for kv in t[sec][1].items()] + ["    }),"]
    out += ['    "arguments": {'] + ["        %r: %r," % kv for kv in t["arguments"].items()] + ["    },", "}"]
    return "\n".join(out)


def compare(got, want, kind, path=""):
    """every code the library answered against the table; a cell that already differed between the emulator and the product
    library when the table was recorded would be a dictionary keyed by the library kind ("emu" / "gpu"): there is none"""
    if isinstance(want, dict) and want and set(want) <= {"emu", "gpu"}:
        want = want[kind]
    if isinstance(want, dict):
        wrong = ["%s: entries %s" % (path, sorted(set(want) ^ set(got)))] if set(want) != set(got) else []
        return wrong + [w for k in want if k in got for w in compare(got[k], want[k], kind, path + " / " + str(k))]
    if isinstance(want, tuple) and isinstance(got, tuple) and len(want) == len(got):
        return [w for i, (g, v) in enumerate(zip(got, want)) for w in compare(g, v, kind, path + " [%d]" % i)]
    return [] if got == want else ["%s: %r, recorded %r" % (path, got, want)]


def check(lib, kind):
    for nd in (0, 1):
        want = {k: v for k, v in EXPECTED.items() if nd or k != "states without d0"}     # (no measured disturbance: d0 is NULL anyway)
        wrong = compare(record(lib, nd), want, kind, "nd=%d" % nd)
        assert not wrong, "\n".join(wrong)
        wrong = compare(k1_tables(lib, nd), EXPECTED_K1[nd], kind, "K1 tables, nd=%d" % nd)
        assert not wrong, "\n".join(wrong)


# K1's remaining tables (MPCQP_GET_GDTAB .. MPCQP_GET_BXHAT) and mpcqp_predmat_form, written from the contract in
# include/mpcqp.h: MPCQP_ERR_UNSUPPORTED (-4) on a stage-only handle, MPCQP_ERR_ORDER (-5) without a model and -- the terminal
# tables -- before a finite x̂ bound had them built, MPCQP_ERR_ARG (-3) for Gd / Xd when nd = 0.  Keyed by nd.
EXPECTED_K1 = {
    0: {
        'before the model': {'gdtab': -5, 'xdtab': -5, 'exhat': -5, 'kxhat': -5, 'bxhat': -5},
        'model': {'gdtab': -3, 'xdtab': -5, 'exhat': -5, 'kxhat': -5, 'bxhat': -5, 'set_bounds(x0max)': 0},
        'terminal tables built': {'gdtab': -3, 'xdtab': -3, 'exhat': 0, 'kxhat': 0, 'bxhat': 0, 'set_model': 0},
        'after another set_model': {'gdtab': -3, 'xdtab': -3, 'exhat': 0, 'kxhat': 0, 'bxhat': 0},
        'predmat_form': {'h=NULL': -1, 'tiny handle': 0},
        'stage-only handle': {'gdtab': -4, 'xdtab': -4, 'exhat': -4, 'kxhat': -4, 'bxhat': -4},
    },
    1: {
        'before the model': {'gdtab': -5, 'xdtab': -5, 'exhat': -5, 'kxhat': -5, 'bxhat': -5},
        'model': {'gdtab': 0, 'xdtab': -5, 'exhat': -5, 'kxhat': -5, 'bxhat': -5, 'set_bounds(x0max)': 0},
        'terminal tables built': {'gdtab': 0, 'xdtab': 0, 'exhat': 0, 'kxhat': 0, 'bxhat': 0, 'set_model': 0},
        'after another set_model': {'gdtab': 0, 'xdtab': 0, 'exhat': 0, 'kxhat': 0, 'bxhat': 0},
        'predmat_form': {'h=NULL': -1, 'tiny handle': 0},
        'stage-only handle': {'gdtab': -4, 'xdtab': -4, 'exhat': -4, 'kxhat': -4, 'bxhat': -4},
    },
}


# Recorded on the emulator from csrc/mpcqp_host.hip as it stood with six estimator flags in the handle.  The codes are the same
# without and with a measured disturbance; "states without d0" is recorded with one only.
EXPECTED = {
    "states": (('enter', 'kf_status', 'kf_status(out=NULL)', 'kf_steady_iters', 'kf_steady_path', 'kf_place_sweeps', 'kf_set_place_cap(5)', 'kf_set_place_cap(-1)', 'kf_lanes_per_estimator', 'kf_set_state_covariance', 'kf_set_state_covariance(P=NULL)', 'kf_set_direct(0)', 'kf_set_direct(1)', 'kf_set_direct(2)', 'kf_solve_steady', 'kf_place', 'kf_correct', 'kf_correct(y0m=NULL)', 'kf_correct(xhat0=NULL)', 'kf_predict', 'kf_predict(u0=NULL)', 'kf_update', 'kf_update(y0m=NULL)', 'kf_update(u0=NULL)', 'im_status', 'im_status(out=NULL)', 'im_correct', 'im_correct(y0m=NULL)', 'im_update', 'est_initstate', 'est_initstate(status=NULL)', 'get(cov)', 'get(gain)', 'get(im_xs)', 'get(im_ys)', 'get(im_yhats)', 'sim_path', 'sim_est_status', 'loop_device(y0m=NULL)'), {
        'none/model': (0, -5, -1, -5, -5, -5, -5, -5, 0, -5, -1, 0, 0, -3, -5, -5, -5, -5, -5, 0, -1, -5, -5, -1, -5, -1, -5, -1, -5, -5, -1, -5, -5, -5, -5, -5, 0, -5, -1),
        'gain/model': (0, -5, -1, -5, -5, -5, -5, -5, 0, -5, -1, 0, 0, -3, -5, -5, 0, 0, -1, 0, -1, 0, 0, -1, -5, -1, -5, -1, -5, 0, -1, -5, 0, -5, -5, -5, 0, -5, -1),
        'tv/model': (0, 0, -1, -5, -5, -5, -5, -5, 16, 0, -1, 0, 0, -3, -5, -5, 0, 0, -1, 0, -1, 0, 0, -1, -5, -1, -5, -1, -5, 0, -1, 0, 0, -5, -5, -5, 0, -5, -1),
        'steady/model': (0, 0, -1, 0, 0, -5, -5, -5, 16, -5, -1, 0, 0, -3, 0, -5, 0, 0, -1, 0, -1, 0, 0, -1, -5, -1, -5, -1, -5, 0, -1, 0, 0, -5, -5, -5, 0, -5, -1),
        'place/model': (0, 0, -1, -5, -5, 0, 0, -3, 64, -5, -1, 0, 0, -3, -5, 0, 0, 0, -1, 0, -1, 0, 0, -1, -5, -1, -5, -1, -5, 0, -1, -5, 0, -5, -5, -5, 0, -5, -1),
        'mhe/model': (0, -5, -1, -5, -5, -5, -5, -5, 0, -5, -1, 0, 0, -3, -5, -5, -5, -5, -5, 0, -1, -5, -5, -1, -5, -1, -5, -1, -5, 0, -1, -5, -5, -5, -5, -5, 0, -5, -1),
        'im/model': (0, -5, -1, -5, -5, -5, -5, -5, 0, -5, -1, -3, 0, -3, -5, -5, -5, -5, -5, 0, -1, -5, -5, -1, 0, -1, 0, -1, 0, 0, -1, -5, -5, 0, 0, 0, 0, -5, -1),
        'none/no model': (0, -5, -1, -5, -5, -5, -5, -5, 0, -5, -1, 0, 0, -3, -5, -5, -5, -5, -5, -5, -1, -5, -5, -1, -5, -1, -5, -1, -5, -5, -1, -5, -5, -5, -5, -5, 0, -5, -1),
        'gain/no model': (0, -5, -1, -5, -5, -5, -5, -5, 0, -5, -1, 0, 0, -3, -5, -5, -5, -5, -1, -5, -1, -5, -5, -1, -5, -1, -5, -1, -5, -5, -1, -5, 0, -5, -5, -5, 0, -5, -1),
        'tv/no model': (0, 0, -1, -5, -5, -5, -5, -5, 16, 0, -1, 0, 0, -3, -5, -5, -5, -5, -1, -5, -1, -5, -5, -1, -5, -1, -5, -1, -5, -5, -1, 0, 0, -5, -5, -5, 0, -5, -1),
        'mhe/no model': (0, -5, -1, -5, -5, -5, -5, -5, 0, -5, -1, 0, 0, -3, -5, -5, -5, -5, -5, -5, -1, -5, -5, -1, -5, -1, -5, -1, -5, -5, -1, -5, -5, -5, -5, -5, 0, -5, -1),
        'im/no model': (0, -5, -1, -5, -5, -5, -5, -5, 0, -5, -1, -3, 0, -3, -5, -5, -5, -5, -5, -5, -1, -5, -5, -1, 0, -1, -5, -1, -5, -5, -1, -5, -5, 0, 0, 0, 0, -5, -1),
    }),
    "states without d0": (('enter', 'kf_correct', 'kf_predict', 'kf_update', 'im_correct', 'im_update', 'est_initstate'), {
        'none/model': (0, -5, -1, -5, -1, -1, -1),
        'gain/model': (0, -1, -1, -1, -1, -1, -1),
        'tv/model': (0, -1, -1, -1, -1, -1, -1),
        'steady/model': (0, -1, -1, -1, -1, -1, -1),
        'place/model': (0, -1, -1, -1, -1, -1, -1),
        'mhe/model': (0, -5, -1, -5, -1, -1, -1),
        'im/model': (0, -5, -1, -5, -1, -1, -1),
        'none/no model': (0, -5, -1, -5, -1, -1, -1),
        'gain/no model': (0, -1, -1, -5, -1, -1, -1),
        'tv/no model': (0, -1, -1, -5, -1, -1, -1),
        'mhe/no model': (0, -5, -1, -5, -1, -1, -1),
        'im/no model': (0, -5, -1, -5, -1, -1, -1),
    }),
    "transitions": (('first', 'second', 'kf_status', 'im_status', 'sim_est_status', 'steady_iters', 'place_sweeps', 'get_gain', 'get_cov', 'get_im_xs', 'est_initstate', 'lanes'), {
        'none -> none': (0, 0, -5, -5, -5, -5, -5, -5, -5, -5, -5, 0),
        'none -> gain': (0, 0, -5, -5, -5, -5, -5, 0, -5, -5, 0, 0),
        'none -> tv': (0, 0, 0, -5, -5, -5, -5, 0, 0, -5, 0, 16),
        'none -> steady': (0, 0, 0, -5, -5, 0, -5, 0, 0, -5, 0, 16),
        'none -> place': (0, 0, 0, -5, -5, -5, 0, 0, -5, -5, 0, 64),
        'none -> mhe': (0, 0, -5, -5, -5, -5, -5, -5, -5, -5, 0, 0),
        'none -> im': (0, 0, -5, 0, -5, -5, -5, -5, -5, 0, 0, 0),
        'none -> im_refused': (0, -3, -5, -5, -5, -5, -5, -5, -5, -5, -5, 0),
        'none -> tv_no_p0': (0, -1, -5, -5, -5, -5, -5, -5, -5, -5, -5, 0),
        'none -> tv_no_p0_other_nym': (0, -1, -5, -5, -5, -5, -5, -5, -5, -5, -5, 0),
        'gain -> none': (0, 0, -5, -5, -5, -5, -5, 0, -5, -5, 0, 0),
        'gain -> gain': (0, 0, -5, -5, -5, -5, -5, 0, -5, -5, 0, 0),
        'gain -> tv': (0, 0, 0, -5, -5, -5, -5, 0, 0, -5, 0, 16),
        'gain -> steady': (0, 0, 0, -5, -5, 0, -5, 0, 0, -5, 0, 16),
        'gain -> place': (0, 0, 0, -5, -5, -5, 0, 0, -5, -5, 0, 64),
        'gain -> mhe': (0, 0, -5, -5, -5, -5, -5, -5, -5, -5, 0, 0),
        'gain -> im': (0, 0, -5, 0, -5, -5, -5, -5, -5, 0, 0, 0),
        'gain -> im_refused': (0, -3, -5, -5, -5, -5, -5, 0, -5, -5, 0, 0),
        'gain -> tv_no_p0': (0, -1, -5, -5, -5, -5, -5, 0, -5, -5, 0, 0),
        'gain -> tv_no_p0_other_nym': (0, -1, -5, -5, -5, -5, -5, 0, -5, -5, 0, 0),
        'tv -> none': (0, 0, 0, -5, -5, -5, -5, 0, 0, -5, 0, 16),
        'tv -> gain': (0, 0, -5, -5, -5, -5, -5, 0, -5, -5, 0, 0),
        'tv -> tv': (0, 0, 0, -5, -5, -5, -5, 0, 0, -5, 0, 16),
        'tv -> steady': (0, 0, 0, -5, -5, 0, -5, 0, 0, -5, 0, 16),
        'tv -> place': (0, 0, 0, -5, -5, -5, 0, 0, -5, -5, 0, 64),
        'tv -> mhe': (0, 0, -5, -5, -5, -5, -5, -5, -5, -5, 0, 0),
        'tv -> im': (0, 0, -5, 0, -5, -5, -5, -5, -5, 0, 0, 0),
        'tv -> im_refused': (0, -3, 0, -5, -5, -5, -5, 0, 0, -5, 0, 16),
        'tv -> tv_no_p0': (0, 0, 0, -5, -5, -5, -5, 0, 0, -5, 0, 16),
        'tv -> tv_no_p0_other_nym': (0, -2, 0, -5, -5, -5, -5, 0, 0, -5, 0, 16),
        'steady -> none': (0, 0, 0, -5, -5, 0, -5, 0, 0, -5, 0, 16),
        'steady -> gain': (0, 0, -5, -5, -5, -5, -5, 0, -5, -5, 0, 0),
        'steady -> tv': (0, 0, 0, -5, -5, -5, -5, 0, 0, -5, 0, 16),
        'steady -> steady': (0, 0, 0, -5, -5, 0, -5, 0, 0, -5, 0, 16),
        'steady -> place': (0, 0, 0, -5, -5, -5, 0, 0, -5, -5, 0, 64),
        'steady -> mhe': (0, 0, -5, -5, -5, -5, -5, -5, -5, -5, 0, 0),
        'steady -> im': (0, 0, -5, 0, -5, -5, -5, -5, -5, 0, 0, 0),
        'steady -> im_refused': (0, -3, 0, -5, -5, 0, -5, 0, 0, -5, 0, 16),
        'steady -> tv_no_p0': (0, -1, 0, -5, -5, 0, -5, 0, 0, -5, 0, 16),
        'steady -> tv_no_p0_other_nym': (0, -1, 0, -5, -5, 0, -5, 0, 0, -5, 0, 16),
        'place -> none': (0, 0, 0, -5, -5, -5, 0, 0, -5, -5, 0, 64),
        'place -> gain': (0, 0, -5, -5, -5, -5, -5, 0, -5, -5, 0, 0),
        'place -> tv': (0, 0, 0, -5, -5, -5, -5, 0, 0, -5, 0, 16),
        'place -> steady': (0, 0, 0, -5, -5, 0, -5, 0, 0, -5, 0, 16),
        'place -> place': (0, 0, 0, -5, -5, -5, 0, 0, -5, -5, 0, 64),
        'place -> mhe': (0, 0, -5, -5, -5, -5, -5, -5, -5, -5, 0, 0),
        'place -> im': (0, 0, -5, 0, -5, -5, -5, -5, -5, 0, 0, 0),
        'place -> im_refused': (0, -3, 0, -5, -5, -5, 0, 0, -5, -5, 0, 64),
        'place -> tv_no_p0': (0, -1, 0, -5, -5, -5, 0, 0, -5, -5, 0, 64),
        'place -> tv_no_p0_other_nym': (0, -1, 0, -5, -5, -5, 0, 0, -5, -5, 0, 64),
        'mhe -> none': (0, 0, -5, -5, -5, -5, -5, -5, -5, -5, -5, 0),
        'mhe -> gain': (0, 0, -5, -5, -5, -5, -5, 0, -5, -5, 0, 0),
        'mhe -> tv': (0, 0, 0, -5, -5, -5, -5, 0, 0, -5, 0, 16),
        'mhe -> steady': (0, 0, 0, -5, -5, 0, -5, 0, 0, -5, 0, 16),
        'mhe -> place': (0, 0, 0, -5, -5, -5, 0, 0, -5, -5, 0, 64),
        'mhe -> mhe': (0, 0, -5, -5, -5, -5, -5, -5, -5, -5, 0, 0),
        'mhe -> im': (0, 0, -5, 0, -5, -5, -5, -5, -5, 0, 0, 0),
        'mhe -> im_refused': (0, -3, -5, -5, -5, -5, -5, -5, -5, -5, 0, 0),
        'mhe -> tv_no_p0': (0, -1, -5, -5, -5, -5, -5, -5, -5, -5, 0, 0),
        'mhe -> tv_no_p0_other_nym': (0, -1, -5, -5, -5, -5, -5, -5, -5, -5, 0, 0),
        'im -> none': (0, 0, -5, 0, -5, -5, -5, -5, -5, 0, 0, 0),
        'im -> gain': (0, 0, -5, -5, -5, -5, -5, 0, -5, -5, 0, 0),
        'im -> tv': (0, 0, 0, -5, -5, -5, -5, 0, 0, -5, 0, 16),
        'im -> steady': (0, 0, 0, -5, -5, 0, -5, 0, 0, -5, 0, 16),
        'im -> place': (0, 0, 0, -5, -5, -5, 0, 0, -5, -5, 0, 64),
        'im -> mhe': (0, 0, -5, -5, -5, -5, -5, -5, -5, -5, 0, 0),
        'im -> im': (0, 0, -5, 0, -5, -5, -5, -5, -5, 0, 0, 0),
        'im -> im_refused': (0, -3, -5, 0, -5, -5, -5, -5, -5, 0, 0, 0),
        'im -> tv_no_p0': (0, -1, -5, 0, -5, -5, -5, -5, -5, 0, 0, 0),
        'im -> tv_no_p0_other_nym': (0, -1, -5, 0, -5, -5, -5, -5, -5, 0, 0, 0),
    }),
    "arguments": {
        'i_ym nym=0': {'kf_set': -2, 'kf_set_covariances': -2, 'kf_set_steady': -2, 'kf_set_poles': -2, 'im_set': -2, 'mhe_attach': -2, 'after: kf_status': -5, 'after: im_status': -5, 'after: get_gain': -5, 'after: est_initstate': -5},
        'i_ym nym=ny+1': {'kf_set': -2, 'kf_set_covariances': -2, 'kf_set_steady': -2, 'kf_set_poles': -2, 'im_set': -2, 'mhe_attach': -2, 'after: kf_status': -5, 'after: im_status': -5, 'after: get_gain': -5, 'after: est_initstate': -5},
        'i_ym index -1': {'kf_set': -3, 'kf_set_covariances': -3, 'kf_set_steady': -3, 'kf_set_poles': -3, 'im_set': -3, 'mhe_attach': -3, 'after: kf_status': -5, 'after: im_status': -5, 'after: get_gain': -5, 'after: est_initstate': -5},
        'i_ym index ny': {'kf_set': -3, 'kf_set_covariances': -3, 'kf_set_steady': -3, 'kf_set_poles': -3, 'im_set': -3, 'mhe_attach': -3, 'after: kf_status': -5, 'after: im_status': -5, 'after: get_gain': -5, 'after: est_initstate': -5},
        'i_ym duplicate': {'kf_set': -3, 'kf_set_covariances': -3, 'kf_set_steady': -3, 'kf_set_poles': -3, 'im_set': -3, 'mhe_attach': -3, 'after: kf_status': -5, 'after: im_status': -5, 'after: get_gain': -5, 'after: est_initstate': -5},
        'null / value': {'kf_set_covariances(Q=NULL)': -1, 'kf_set_covariances(R=NULL)': -1, 'kf_set_covariances(i_ym=NULL)': -1, 'kf_set_covariances(P0=NULL) not time-varying': -1, 'kf_set_covariances(Q not symmetric)': -3, 'kf_set_covariances(P0 not symmetric)': -3, 'kf_set_covariances': 0, 'kf_set_covariances(P0=NULL) time-varying': 0, 'kf_set_covariances(P0=NULL, Q not symmetric) time-varying': -3, 'kf_set_steady(Q=NULL)': -1, 'kf_set_steady(R=NULL)': -1, 'kf_set_steady(i_ym=NULL)': -1, 'kf_set_steady(Q not symmetric)': -3, 'kf_set_poles(poles=NULL)': -1, 'kf_set_poles(i_ym=NULL)': -1, 'kf_set_poles(|pole| = 1)': -3, 'after: kf_status': 0, 'after: lanes': 16, 'kf_set(Khat=NULL)': -1, 'mhe_attach(i_ym=NULL)': -1, 'im_set(i_ym=NULL)': -1, 'im_set(nxs=0, given)': -3},
        'before the model': {'kf_set_steady': -5, 'kf_set_steady(Q not symmetric)': -3, 'kf_set_steady(duplicate)': -3, 'kf_set_poles': -5, 'kf_set_poles(|pole| = 1)': -3, 'kf_solve_steady': -5, 'kf_place': -5, 'step': -5, 'explicit_step': -5, 'explicit_status': -5, 'explicit_status(out=NULL)': -1, 'set_output_weight_blocks': -5, 'set_dense_weights': -5, 'set_custom_bounds': -5, 'explicit_prepare(2)': -3, 'next': 0},
        'before the weights': {'step': -5, 'explicit_step': -5, 'explicit_status': -5, 'explicit_status(out=NULL)': -1, 'set_output_weight_blocks': -5, 'set_dense_weights': -5, 'set_custom_bounds': -5, 'explicit_prepare(2)': -3, 'next': 0},
        'before explicit_prepare': {'step': 0, 'explicit_step': -5, 'explicit_status': -5, 'explicit_status(out=NULL)': -1, 'set_output_weight_blocks': 0, 'set_dense_weights': 0, 'set_custom_bounds': -5, 'explicit_prepare(2)': -3, 'next': 0},
        'prepared': {'step': 0, 'explicit_step': 0, 'explicit_status': 0, 'explicit_status(out=NULL)': -1, 'next': 0, 'im_set': -4, 'after: im_status': -5},
        'custom rows': {'set_custom_bounds before the constraints': -5, 'im_set': 0, 'set_custom_constraints on an InternalModel': -4, 'kf_set': 0, 'set_custom_constraints': 0, 'set_custom_bounds': 0, 'set_custom_bounds(C_wmin without a slack)': -3, 'im_set with custom rows': -4, 'after: get_gain': 0, 'step': 0},
        'get on a fresh handle': {'0': -3, '1': -5, '2': -5, '3': -5, '4': -5, '5': -5, '6': -5, '7': -5, '8': -5, '9': -5, '10': -5, '11': -5, '12': -5, '13': -5, '14': -5, '15': -5, '16': -5, '17': -5, '18': -5, '19': -5, '20': -5, '21': -5, '22': -5, '23': -5, '24': -5, '25': -5, '26': -5, '27': -3, '28': -3, '29': -3, 'out=NULL': -1},
    },
}


def test_return_codes_on_the_emulator():
    lib = mpcqp.api.load_library(build())
    try:
        check(lib, "emu")
    finally:
        mpcqp.api._lib = None


@pytest.mark.gpu
def test_return_codes_on_the_gpu():
    check(mpcqp.api.load_library(), "gpu")


if __name__ == "__main__":      # the table of the library at hand: the emulator, or with `gpu` the product library (or MPCQP_LIB)
    lib_ = mpcqp.api.load_library(None if "gpu" in sys.argv[1:] else build())
    t0, t1 = record(lib_, 0), record(lib_, 1)
    print(show(t1))
    print("# nd = 0 differs in:", compare(t0, {k: v for k, v in t1.items() if k != "states without d0"}, "emu", "nd=0"))
