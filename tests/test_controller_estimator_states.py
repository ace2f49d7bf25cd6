"""Which estimator sits behind a BatchLinMPC after every setter, and what every estimator-dependent method does in each of
the seven states (none, Khat gain, time-varying, steady, Luenberger, MovingHorizonEstimator, InternalModel): the Python half
of the state machine whose host half tests/test_host_return_codes.py pins.  A recording proxy around `mpc.hd` (and a
recording subclass of BatchMHE where one is attached) notes the names of the methods the controller calls, in order; the
exception type with the first words of its message and the warnings with theirs are noted next to them.  Everything is
compared with the literal table EXPECTED at the end of this file, recorded on the tiny shape of test_host_return_codes
(B = 2, nx̂ = 3, nu = 1, ny = 2, Hp = 4, Hc = 2, i_ym = (0, 1), He = 2, poles (0.1, 0.2, 0.3), Q̂ = R̂ = P̂₀ = I) once
without and once with a measured disturbance, from the controller as it stood with five estimator attributes.  A cell that
changed on purpose when the estimator kind became one field is a dictionary {"tip": ..., "parent": ...}: the refused
setters that used to leave `i_ym` / `direct` behind, and the calls that used to die with an AttributeError without an
estimator.  The CPU test runs on tests/emu/libmpcqp_emu_all.so, the `gpu` twin on the product library; both read the same
table.  `python -m tests.test_controller_estimator_states [gpu] [--dump FILE] [--parent FILE]` prints the table of the code
at hand (--dump writes the raw record, --parent merges such a record in as the "parent" column)."""
import ast
import sys
import warnings

import numpy as np
import pytest

import mpcqp
from mpcqp.mhe import BatchMHE
from tests import test_host_return_codes as host_codes

B, NX, NU, NY, HP, HC, HE = 2, 3, 1, 2, 4, 2, 2
IYM = (0, 1)
STATES = ("none", "gain", "tv", "steady", "place", "mhe", "im")
FORMS = {"filter": True, "predictor": False}
PUBLIC = ("kf_timevarying", "kf_steady", "kf_luenberger", "internal")


def model(nd):
    """logical (B,·,·) matrices: Â stable with distinct eigenvalues, (Â, Ĉ) observable"""
    rng = np.random.default_rng(7)
    A = np.stack([np.diag([0.5, 0.6, 0.7]) + 0.05 * rng.standard_normal((NX, NX)) for _ in range(B)])
    Bu, Cm = rng.standard_normal((B, NX, NU)), rng.standard_normal((B, NY, NX))
    Bd = rng.standard_normal((B, NX, nd)) if nd else None
    Dd = rng.standard_normal((B, NY, nd)) if nd else None
    return A, Bu, Cm, Bd, Dd


class Recorder:
    """`obj` with the names of the methods called through this proxy appended to `log`"""

    def __init__(self, obj, log):
        self.__dict__.update(_obj=obj, _log=log)

    def __getattr__(self, name):
        a = getattr(self._obj, name)
        if not callable(a) or name.startswith("_"):
            return a
        def call(*args, **kw):
            self._log.append(name)
            return a(*args, **kw)
        return call

    def __setattr__(self, name, v):
        setattr(self._obj, name, v)


class RecordedMHE(BatchMHE):
    """a BatchMHE (setestimator asks isinstance) whose methods the controller forwards to are noted as mhe.<name>"""
    log = None


def _noted(name):
    def call(self, *args, **kw):
        self.log.append("mhe." + name)
        return getattr(BatchMHE, name)(self, *args, **kw)
    return call


for _name in ("preparestate", "updatestate", "setstate", "setmodel", "initstate", "getinfo"):
    setattr(RecordedMHE, _name, _noted(_name))


class Case:
    """One controller of the tiny shape, its recorder and the arguments of the probes."""

    def __init__(self, lib, nd):
        self.lib, self.nd, self.log = lib, nd, []
        self.model = model(nd)
        self.mpc = mpcqp.BatchLinMPC(*self.model, Hp=HP, Hc=HC, lib=lib)
        self.mpc.hd = Recorder(self.mpc.hd, self.log)
        self.d = [0.2] if nd else None

    def estimator(self, direct=True):
        A, Bu, Cm, Bd, Dd = self.model
        est = RecordedMHE(A, Bu, Cm[:, IYM], Bd, None if Dd is None else Dd[:, IYM], He=HE, direct=direct, lib=self.lib)
        est.log = self.log
        return est

    def attach(self, kind, direct=None, i_ym=IYM, **kw):
        """the six attaching calls; `kw` replaces an argument of the estimator's own dictionary or adds xhat0"""
        eye, top = np.eye, {k: kw.pop(k) for k in ("xhat0",) if k in kw}
        if kind == "gain":
            return self.mpc.setestimator(kw.get("Khat", np.full((B, NX, len(IYM)), 0.1)), i_ym, direct=direct, **top)
        if kind == "mhe":
            return self.mpc.setestimator(mhe=self.estimator(kw.get("est_direct", direct is not False)), i_ym=i_ym, direct=direct, **top)
        args = {"tv": dict(Qhat=eye(NX), Rhat=eye(len(IYM)), P0=eye(NX)), "steady": dict(Qhat=eye(NX), Rhat=eye(len(IYM))),
                "place": dict(poles=(0.1, 0.2, 0.3)), "im": dict()}[kind]
        key = {"tv": "covariances", "steady": "steady", "place": "luenberger", "im": "internal"}[kind]
        return self.mpc.setestimator(i_ym=i_ym, direct=direct, **{key: dict(args, **kw)}, **top)

    def note(self, f):
        """(outcome, calls, warnings) of f(): 'ok', or the exception type and the first words of its message"""
        del self.log[:]
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                f()
                out = "ok"
            except Exception as e:      # noqa: BLE001  (which exception it is, is what the table records)
                out = "%s: %s" % (type(e).__name__, " ".join(str(e).split()[:5]))
        return out, tuple(self.log), tuple(" ".join(str(w.message).split()[:8]) for w in caught)

    def mirror(self):
        """the estimator through the public names, direct, i_ym, x̂0 of the first member, and the handle's form as the mirror has it"""
        m = self.mpc
        kinds = [n for n in PUBLIC if getattr(m, n, False)] + (["mhe"] if getattr(m, "mhe", None) is not None else [])
        i_ym = getattr(m, "i_ym", None)
        return ("+".join(kinds) or "-", getattr(m, "direct", None), None if i_ym is None else tuple(int(i) for i in i_ym),
                self.xhat0(), getattr(m, "_hd_direct", True))

    def xhat0(self):
        try:
            return tuple(self.mpc.xhat0[0].tolist())
        except AttributeError:
            return None

    def probes(self):
        """the estimator-dependent methods, one after the other on this controller"""
        m, d, out = self.mpc, self.d, {}
        A, Bu, Cm, Bd, Dd = self.model
        ym, u, x = [0.5, -0.25], [0.1], [0.1, 0.2, 0.3]
        out["preparestate(ym)"] = self.note(lambda: m.preparestate(ym, d))
        if getattr(m, "mhe", None) is None:     # (a NaN goes to the MovingHorizonEstimator unchanged: its solve is not this table's)
            out["preparestate(NaN)"] = self.note(lambda: m.preparestate([[0.5, -0.25], [np.nan, 0.0]], d))
        out["updatestate(u, ym)"] = self.note(lambda: m.updatestate(u, ym, d))
        out["updatestate(u)"] = self.note(lambda: m.updatestate(u, None, d))
        out["setmodel"] = self.note(lambda: m.setmodel(A, Bu, Cm, Bd, Dd))
        out["setstate(x)"] = self.note(lambda: m.setstate(x)) + (self.xhat0(),)
        out["setmodel(xhop)"] = self.note(lambda: m.setmodel(A, Bu, Cm, Bd, Dd, xhop=[0.5, 0.0, -0.5])) + (self.xhat0(),)
        out["setstate(x, P)"] = self.note(lambda: m.setstate(x, np.eye(NX)))
        out["setcovariances"] = self.note(lambda: m.setcovariances(2 * np.eye(NX), 2 * np.eye(len(IYM))))
        out["initstate(u, ym)"] = self.note(lambda: m.initstate(u, ym, d))
        out["evaloutput"] = self.note(lambda: m.evaloutput(d))
        keys = []
        out["getinfo"] = self.note(lambda: (m.moveinput(None, None, d, want_info=True), keys.extend(sorted(m.getinfo())))) + (tuple(keys),)
        out["sim(2)"] = self.note(lambda: m.sim(2, d=d, plant=self.model))
        return out


def attaches(lib, nd):
    """every state x every attaching call x both forms: the setter's outcome and calls, the mirror, x̂0 with `xhat0=`"""
    out, after = {}, {}
    for a in STATES:
        for b in STATES[1:]:
            for form, direct in FORMS.items():
                c = Case(lib, nd)
                if a != "none":
                    c.attach(a, True)
                key = "%s -> %s/%s" % (a, b, form)
                out[key] = c.note(lambda: c.attach(b, direct)) + (c.mirror(),)
                if out[key][0] == "ok":
                    after[key] = c.probes()
                if direct:
                    c = Case(lib, nd)
                    if a != "none":
                        c.attach(a, True)
                    out[key] += (c.note(lambda: c.attach(b, direct, xhat0=[1.0, 2.0, 3.0]))[0], c.xhat0())
    after["none"] = Case(lib, nd).probes()       # (a controller that never had an estimator)
    return out, after


REFUSALS = {
    "two estimators": lambda c: c.mpc.setestimator(np.full((B, NX, 2), 0.1), steady=dict(Qhat=np.eye(NX), Rhat=np.eye(2))),
    "internal, direct=False": lambda c: c.attach("im", False),
    "mhe with xhat0": lambda c: c.attach("mhe", None, xhat0=[1.0, 2.0, 3.0]),
    "mhe, contradicting direct": lambda c: c.attach("mhe", False, est_direct=True),
    "Khat of the wrong shape": lambda c: c.attach("gain", False, Khat=np.zeros((B, NX, 1))),
    "tv: Q̂ not Hermitian": lambda c: c.attach("tv", False, Qhat=np.array([[1, 0.1, 0], [0, 1, 0], [0, 0, 1.0]])),
    "steady: Q̂ not Hermitian": lambda c: c.attach("steady", False, Qhat=np.array([[1, 0.1, 0], [0, 1, 0], [0, 0, 1.0]])),
    "tv: R̂ of the wrong size": lambda c: c.attach("tv", False, Rhat=np.eye(3)),
    "steady: R̂ of the wrong size": lambda c: c.attach("steady", False, Rhat=np.eye(3)),
    "complex poles": lambda c: c.attach("place", False, poles=(0.1, 0.2 + 0.1j, 0.2 - 0.1j)),
    "a pole on the unit circle": lambda c: c.attach("place", False, poles=(0.1, 0.2, -1.0)),
    "a wrong pole count": lambda c: c.attach("place", False, poles=(0.1, 0.2)),
    "stoch_ym with a zero Ds": lambda c: c.attach("im", None, stoch_ym=(0.5 * np.eye(2), np.eye(2), np.eye(2), np.zeros((2, 2)))),
}
for _b in STATES[1:]:               # i_ym out of range and repeated on every path (the predictor form where the path has one)
    for _name, _iym in (("out of range", (0, NY)), ("repeated", (1, 1))):
        REFUSALS["%s: i_ym %s" % (_b, _name)] = lambda c, b=_b, i=_iym: c.attach(b, None if b in ("mhe", "im") else False, i_ym=i)


def refusals(lib, nd):
    """every refusal from every state (entered in the filter form): outcome and calls of the refused setter, the mirror after it"""
    out = {}
    for name, f in REFUSALS.items():
        for a in STATES:
            c = Case(lib, nd)
            if a != "none":
                c.attach(a, True)
            out["%s / %s" % (name, a)] = c.note(lambda: f(c)) + (c.mirror(),)
    return out


def record(lib, nd):
    att, after = attaches(lib, nd)
    return {"attach": att, "after": after, "refusals": refusals(lib, nd)}


def fold(after):
    """the probes of 'a -> b/form' hang on the starting state a in a few cells only: 'b/form' holds the row of a = b's own first
    attach (none -> b), 'a -> b/form' only the cells that differ from it"""
    out = {"none": after["none"]}
    for key, row in after.items():
        if key == "none":
            continue
        a, tail = key.split(" -> ")
        if a == "none":
            out[tail] = row
    for key, row in after.items():
        if key == "none" or key.startswith("none -> "):
            continue
        base = out[key.split(" -> ")[1]]
        diff = {k: v for k, v in row.items() if base.get(k) != v}
        assert set(row) == set(base)
        if diff:
            out[key] = diff
    return out


def folded(lib, nd):
    r = record(lib, nd)
    return dict(r, after=fold(r["after"]))


def merge(tip, parent):
    """cells that differ become {"tip": ..., "parent": ...}"""
    if isinstance(tip, dict) and isinstance(parent, dict):
        return {k: (merge(v, parent[k]) if k in parent else v) for k, v in tip.items()}
    return tip if tip == parent else {"tip": tip, "parent": parent}


def compare(got, want, column="tip", path=""):
    if isinstance(want, dict) and set(want) == {"tip", "parent"}:
        want = want[column]
    if isinstance(want, dict):
        wrong = ["%s: entries %s" % (path, sorted(set(want) ^ set(got)))] if not isinstance(got, dict) or set(want) != set(got) else []
        return wrong + [w for k in want if isinstance(got, dict) and k in got for w in compare(got[k], want[k], column, path + " / " + str(k))]
    return [] if got == want else ["%s: %r, recorded %r" % (path, got, want)]


def show(t):
    out = ["{"]
    for sec in ("attach", "after", "refusals"):
        out += ['    "%s": {' % sec] + ["        %r: %r," % kv for kv in t[sec].items()] + ["    },"]
    return "\n".join(out + ["}"])


def check(lib, nd, column="tip"):
    wrong = compare(folded(lib, nd), EXPECTED, column, "nd=%d" % nd)
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("nd", [0, 1])
def test_estimator_states_on_the_emulator(nd):
    lib = mpcqp.api.load_library(host_codes.build())
    try:
        check(lib, nd)
    finally:
        mpcqp.api._lib = None


@pytest.mark.gpu
@pytest.mark.parametrize("nd", [0, 1])
def test_estimator_states_on_the_gpu(nd):
    check(mpcqp.api.load_library(), nd)


def main(argv):
    """the table of the code at hand: on the emulator, or with `gpu` on the product library (or MPCQP_LIB)"""
    lib = mpcqp.api.load_library(None if "gpu" in argv else host_codes.build())
    t = folded(lib, 1)
    print("# nd = 0 differs in:", compare(folded(lib, 0), t, path="nd=0"))
    if "--dump" in argv:
        open(argv[argv.index("--dump") + 1], "w").write(repr(t))
    if "--parent" in argv:
        t = merge(t, ast.literal_eval(open(argv[argv.index("--parent") + 1]).read()))
    print("EXPECTED = " + show(t))


# Recorded on the emulator.  The entries are the same without and with a measured disturbance.  "attach": 'a -> b/form' is
# (outcome, calls, warnings) of the setter of b on a controller in state a, the mirror after it -- (estimator through the public
# names, direct, i_ym, x̂0 of the first member, the handle's form) -- and, in the filter form, outcome and x̂0 of the same call
# with xhat0=(1, 2, 3).  "after": the probes on the controller that 'none -> b/form' left (from every other state they
# answer the same: fold() found no cell that differs), 'none' on a controller without an estimator.  "refusals": 'refusal /
# a' is (outcome, calls, warnings) of the refused setter on a controller in state a, and the mirror after it.
EXPECTED = {
    "attach": {
        'none -> gain/filter': ('ok', ('kf_set',), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'none -> gain/predictor': ('ok', ('kf_set_direct', 'kf_set'), (), ('-', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'none -> tv/filter': ('ok', ('kf_set_covariances',), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'none -> tv/predictor': ('ok', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_timevarying', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'none -> steady/filter': ('ok', ('kf_set_steady', 'kf_status'), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'none -> steady/predictor': ('ok', ('kf_set_direct', 'kf_set_steady', 'kf_status'), (), ('kf_steady', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'none -> place/filter': ('ok', ('kf_set_poles', 'kf_status'), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'none -> place/predictor': ('ok', ('kf_set_direct', 'kf_set_poles', 'kf_status'), (), ('kf_luenberger', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'none -> mhe/filter': ('ok', ('mhe_attach',), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True), 'ValueError: xhat0: the estimate is the', None),
        'none -> mhe/predictor': ('ok', ('mhe_attach',), (), ('mhe', False, (0, 1), (0.0, 0.0, 0.0), True)),
        'none -> im/filter': ('ok', ('im_set', 'im_status'), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'none -> im/predictor': ('ValueError: direct=False: the InternalModel is always', (), (), ('-', None, None, None, True)),
        'gain -> gain/filter': ('ok', ('kf_set',), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'gain -> gain/predictor': ('ok', ('kf_set_direct', 'kf_set'), (), ('-', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'gain -> tv/filter': ('ok', ('kf_set_covariances',), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'gain -> tv/predictor': ('ok', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_timevarying', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'gain -> steady/filter': ('ok', ('kf_set_steady', 'kf_status'), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'gain -> steady/predictor': ('ok', ('kf_set_direct', 'kf_set_steady', 'kf_status'), (), ('kf_steady', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'gain -> place/filter': ('ok', ('kf_set_poles', 'kf_status'), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'gain -> place/predictor': ('ok', ('kf_set_direct', 'kf_set_poles', 'kf_status'), (), ('kf_luenberger', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'gain -> mhe/filter': ('ok', ('mhe_attach',), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True), 'ValueError: xhat0: the estimate is the', (0.0, 0.0, 0.0)),
        'gain -> mhe/predictor': ('ok', ('mhe_attach',), (), ('mhe', False, (0, 1), (0.0, 0.0, 0.0), True)),
        'gain -> im/filter': ('ok', ('im_set', 'im_status'), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'gain -> im/predictor': ('ValueError: direct=False: the InternalModel is always', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'tv -> gain/filter': ('ok', ('kf_set',), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'tv -> gain/predictor': ('ok', ('kf_set_direct', 'kf_set'), (), ('-', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'tv -> tv/filter': ('ok', ('kf_set_covariances',), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'tv -> tv/predictor': ('ok', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_timevarying', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'tv -> steady/filter': ('ok', ('kf_set_steady', 'kf_status'), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'tv -> steady/predictor': ('ok', ('kf_set_direct', 'kf_set_steady', 'kf_status'), (), ('kf_steady', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'tv -> place/filter': ('ok', ('kf_set_poles', 'kf_status'), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'tv -> place/predictor': ('ok', ('kf_set_direct', 'kf_set_poles', 'kf_status'), (), ('kf_luenberger', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'tv -> mhe/filter': ('ok', ('mhe_attach',), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True), 'ValueError: xhat0: the estimate is the', (0.0, 0.0, 0.0)),
        'tv -> mhe/predictor': ('ok', ('mhe_attach',), (), ('mhe', False, (0, 1), (0.0, 0.0, 0.0), True)),
        'tv -> im/filter': ('ok', ('im_set', 'im_status'), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'tv -> im/predictor': ('ValueError: direct=False: the InternalModel is always', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'steady -> gain/filter': ('ok', ('kf_set',), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'steady -> gain/predictor': ('ok', ('kf_set_direct', 'kf_set'), (), ('-', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'steady -> tv/filter': ('ok', ('kf_set_covariances',), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'steady -> tv/predictor': ('ok', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_timevarying', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'steady -> steady/filter': ('ok', ('kf_set_steady', 'kf_status'), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'steady -> steady/predictor': ('ok', ('kf_set_direct', 'kf_set_steady', 'kf_status'), (), ('kf_steady', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'steady -> place/filter': ('ok', ('kf_set_poles', 'kf_status'), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'steady -> place/predictor': ('ok', ('kf_set_direct', 'kf_set_poles', 'kf_status'), (), ('kf_luenberger', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'steady -> mhe/filter': ('ok', ('mhe_attach',), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True), 'ValueError: xhat0: the estimate is the', (0.0, 0.0, 0.0)),
        'steady -> mhe/predictor': ('ok', ('mhe_attach',), (), ('mhe', False, (0, 1), (0.0, 0.0, 0.0), True)),
        'steady -> im/filter': ('ok', ('im_set', 'im_status'), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'steady -> im/predictor': ('ValueError: direct=False: the InternalModel is always', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'place -> gain/filter': ('ok', ('kf_set',), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'place -> gain/predictor': ('ok', ('kf_set_direct', 'kf_set'), (), ('-', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'place -> tv/filter': ('ok', ('kf_set_covariances',), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'place -> tv/predictor': ('ok', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_timevarying', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'place -> steady/filter': ('ok', ('kf_set_steady', 'kf_status'), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'place -> steady/predictor': ('ok', ('kf_set_direct', 'kf_set_steady', 'kf_status'), (), ('kf_steady', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'place -> place/filter': ('ok', ('kf_set_poles', 'kf_status'), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'place -> place/predictor': ('ok', ('kf_set_direct', 'kf_set_poles', 'kf_status'), (), ('kf_luenberger', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'place -> mhe/filter': ('ok', ('mhe_attach',), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True), 'ValueError: xhat0: the estimate is the', (0.0, 0.0, 0.0)),
        'place -> mhe/predictor': ('ok', ('mhe_attach',), (), ('mhe', False, (0, 1), (0.0, 0.0, 0.0), True)),
        'place -> im/filter': ('ok', ('im_set', 'im_status'), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'place -> im/predictor': ('ValueError: direct=False: the InternalModel is always', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe -> gain/filter': ('ok', ('kf_set',), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'mhe -> gain/predictor': ('ok', ('kf_set_direct', 'kf_set'), (), ('-', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'mhe -> tv/filter': ('ok', ('kf_set_covariances',), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'mhe -> tv/predictor': ('ok', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_timevarying', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'mhe -> steady/filter': ('ok', ('kf_set_steady', 'kf_status'), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'mhe -> steady/predictor': ('ok', ('kf_set_direct', 'kf_set_steady', 'kf_status'), (), ('kf_steady', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'mhe -> place/filter': ('ok', ('kf_set_poles', 'kf_status'), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'mhe -> place/predictor': ('ok', ('kf_set_direct', 'kf_set_poles', 'kf_status'), (), ('kf_luenberger', False, (0, 1), (0.0, 0.0, 0.0), False)),
        'mhe -> mhe/filter': ('ok', ('mhe_attach',), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True), 'ValueError: xhat0: the estimate is the', (0.0, 0.0, 0.0)),
        'mhe -> mhe/predictor': ('ok', ('mhe_attach',), (), ('mhe', False, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe -> im/filter': ('ok', ('im_set', 'im_status'), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'mhe -> im/predictor': ('ValueError: direct=False: the InternalModel is always', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'im -> gain/filter': ('ok', ('kf_set',), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'im -> gain/predictor': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'im -> tv/filter': ('ok', ('kf_set_covariances',), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'im -> tv/predictor': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'im -> steady/filter': ('ok', ('kf_set_steady', 'kf_status'), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'im -> steady/predictor': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'im -> place/filter': ('ok', ('kf_set_poles', 'kf_status'), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'im -> place/predictor': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'im -> mhe/filter': ('ok', ('mhe_attach',), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True), 'ValueError: xhat0: the estimate is the', (0.0, 0.0, 0.0)),
        'im -> mhe/predictor': ('ok', ('mhe_attach',), (), ('mhe', False, (0, 1), (0.0, 0.0, 0.0), True)),
        'im -> im/filter': ('ok', ('im_set', 'im_status'), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True), 'ok', (1.0, 2.0, 3.0)),
        'im -> im/predictor': ('ValueError: direct=False: the InternalModel is always', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)),
    },
    "after": {
        'none': {'preparestate(ym)': {'tip': ('ValueError: no estimator attached (setestimator)', (), ()), 'parent': ("AttributeError: 'BatchLinMPC' object has no attribute", (), ())}, 'preparestate(NaN)': {'tip': ('ValueError: no estimator attached (setestimator)', (), ()), 'parent': ("AttributeError: 'BatchLinMPC' object has no attribute", (), ())}, 'updatestate(u, ym)': {'tip': ('ValueError: no estimator attached (setestimator)', (), ()), 'parent': ('AttributeError: xhat0', (), ())}, 'updatestate(u)': {'tip': ('ValueError: no estimator attached (setestimator)', (), ()), 'parent': ('AttributeError: xhat0', (), ())}, 'setmodel': ('ok', ('set_model',), ()), 'setstate(x)': ('ValueError: no estimator attached (setestimator)', (), (), None), 'setmodel(xhop)': ('ok', ('set_model',), (), None), 'setstate(x, P)': ('ValueError: no estimator attached (setestimator)', (), ()), 'setcovariances': ('ValueError: Q̂ and R̂ can only', (), ()), 'initstate(u, ym)': ('ValueError: no estimator attached (setestimator)', (), ()), 'evaloutput': ('ValueError: no estimator attached (setestimator)', (), ()), 'getinfo': ('AttributeError: xhat0', (), (), ()), 'sim(2)': ('ValueError: no estimator attached (setestimator)', (), ())},
        'gain/filter': {'preparestate(ym)': ('ok', ('kf_correct',), ()), 'preparestate(NaN)': ('ok', ('kf_correct',), ('NaN values in the Kalman filter measurements ym:',)), 'updatestate(u, ym)': ('ok', ('kf_predict',), ()), 'updatestate(u)': ('ok', ('kf_predict',), ()), 'setmodel': ('ok', ('set_model',), ()), 'setstate(x)': ('ok', (), (), (0.1, 0.2, 0.3)), 'setmodel(xhop)': ('ok', ('set_model',), (), (-0.4, 0.2, 0.8)), 'setstate(x, P)': ('ValueError: the SteadyKalmanFilter has no covariance', (), ()), 'setcovariances': ('ValueError: Q̂ and R̂ can only', (), ()), 'initstate(u, ym)': ('ok', ('est_initstate',), ()), 'evaloutput': ('ok', (), ()), 'getinfo': ('ok', ('set_flags', 'prepare', 'step'), (), ('DeltaU', 'Dhat', 'D̂', 'J', 'Rhatu', 'Rhaty', 'R̂u', 'R̂y', 'U', 'Xhat0', 'X̂0', 'Yhat', 'Yhats', 'Ztilde', 'Z̃', 'd', 'epsilon', 'lastu', 'u', 'xhat', 'xhatend', 'x̂', 'x̂end', 'yhat', 'Ŷ', 'Ŷs', 'ŷ', 'ΔU', 'ϵ')), 'sim(2)': ('ok', ('sim_set_plant', 'sim_path', 'sim'), ())},
        'gain/predictor': {'preparestate(ym)': ('ok', (), ()), 'preparestate(NaN)': ('ok', (), ()), 'updatestate(u, ym)': ('ok', ('kf_update',), ()), 'updatestate(u)': ('ok', ('kf_update',), ('NaN values in the Kalman filter measurements ym:',)), 'setmodel': ('ok', ('set_model',), ()), 'setstate(x)': ('ok', (), (), (0.1, 0.2, 0.3)), 'setmodel(xhop)': ('ok', ('set_model',), (), (-0.4, 0.2, 0.8)), 'setstate(x, P)': ('ValueError: the SteadyKalmanFilter has no covariance', (), ()), 'setcovariances': ('ValueError: Q̂ and R̂ can only', (), ()), 'initstate(u, ym)': ('ok', ('est_initstate',), ()), 'evaloutput': ('ok', (), ()), 'getinfo': ('ok', ('set_flags', 'prepare', 'step'), (), ('DeltaU', 'Dhat', 'D̂', 'J', 'Rhatu', 'Rhaty', 'R̂u', 'R̂y', 'U', 'Xhat0', 'X̂0', 'Yhat', 'Yhats', 'Ztilde', 'Z̃', 'd', 'epsilon', 'lastu', 'u', 'xhat', 'xhatend', 'x̂', 'x̂end', 'yhat', 'Ŷ', 'Ŷs', 'ŷ', 'ΔU', 'ϵ')), 'sim(2)': ('ok', ('sim_set_plant', 'sim_path', 'sim'), ())},
        'tv/filter': {'preparestate(ym)': ('ok', ('kf_correct',), ()), 'preparestate(NaN)': ('ok', ('kf_correct',), ('NaN values in the Kalman filter measurements ym:',)), 'updatestate(u, ym)': ('ok', ('kf_predict',), ()), 'updatestate(u)': ('ok', ('kf_predict',), ()), 'setmodel': ('ok', ('set_model',), ()), 'setstate(x)': ('ok', (), (), (0.1, 0.2, 0.3)), 'setmodel(xhop)': ('ok', ('set_model',), (), (-0.4, 0.2, 0.8)), 'setstate(x, P)': ('ok', ('kf_set_state_covariance',), ()), 'setcovariances': ('ok', ('kf_set_covariances',), ()), 'initstate(u, ym)': ('ok', ('est_initstate', 'kf_set_state_covariance'), ()), 'evaloutput': ('ok', (), ()), 'getinfo': ('ok', ('set_flags', 'prepare', 'step', 'kf_covariance', 'kf_gain', 'kf_status'), (), ('DeltaU', 'Dhat', 'D̂', 'J', 'Khat', 'K̂', 'Phat', 'P̂', 'Rhatu', 'Rhaty', 'R̂u', 'R̂y', 'U', 'Xhat0', 'X̂0', 'Yhat', 'Yhats', 'Ztilde', 'Z̃', 'd', 'epsilon', 'kf_status', 'lastu', 'u', 'xhat', 'xhatend', 'x̂', 'x̂end', 'yhat', 'Ŷ', 'Ŷs', 'ŷ', 'ΔU', 'ϵ')), 'sim(2)': ('ok', ('sim_set_plant', 'sim_path', 'sim'), ())},
        'tv/predictor': {'preparestate(ym)': ('ok', (), ()), 'preparestate(NaN)': ('ok', (), ()), 'updatestate(u, ym)': ('ok', ('kf_update',), ()), 'updatestate(u)': ('ok', ('kf_update',), ('NaN values in the Kalman filter measurements ym:',)), 'setmodel': ('ok', ('set_model',), ()), 'setstate(x)': ('ok', (), (), (0.1, 0.2, 0.3)), 'setmodel(xhop)': ('ok', ('set_model',), (), (-0.4, 0.2, 0.8)), 'setstate(x, P)': ('ok', ('kf_set_state_covariance',), ()), 'setcovariances': ('ok', ('kf_set_covariances',), ()), 'initstate(u, ym)': ('ok', ('est_initstate', 'kf_set_state_covariance'), ()), 'evaloutput': ('ok', (), ()), 'getinfo': ('ok', ('set_flags', 'prepare', 'step', 'kf_covariance', 'kf_gain', 'kf_status'), (), ('DeltaU', 'Dhat', 'D̂', 'J', 'Khat', 'K̂', 'Phat', 'P̂', 'Rhatu', 'Rhaty', 'R̂u', 'R̂y', 'U', 'Xhat0', 'X̂0', 'Yhat', 'Yhats', 'Ztilde', 'Z̃', 'd', 'epsilon', 'kf_status', 'lastu', 'u', 'xhat', 'xhatend', 'x̂', 'x̂end', 'yhat', 'Ŷ', 'Ŷs', 'ŷ', 'ΔU', 'ϵ')), 'sim(2)': ('ok', ('sim_set_plant', 'sim_path', 'sim'), ())},
        'steady/filter': {'preparestate(ym)': ('ok', ('kf_correct',), ()), 'preparestate(NaN)': ('ok', ('kf_correct',), ('NaN values in the Kalman filter measurements ym:',)), 'updatestate(u, ym)': ('ok', ('kf_predict',), ()), 'updatestate(u)': ('ok', ('kf_predict',), ()), 'setmodel': ('ok', ('set_model', 'kf_solve_steady', 'kf_status'), ()), 'setstate(x)': ('ok', (), (), (0.1, 0.2, 0.3)), 'setmodel(xhop)': ('ok', ('set_model', 'kf_solve_steady', 'kf_status'), (), (-0.4, 0.2, 0.8)), 'setstate(x, P)': ('ValueError: the SteadyKalmanFilter has no covariance', (), ()), 'setcovariances': ('ok', ('kf_set_steady', 'kf_status'), ()), 'initstate(u, ym)': ('ok', ('est_initstate',), ()), 'evaloutput': ('ok', (), ()), 'getinfo': ('ok', ('set_flags', 'prepare', 'step', 'kf_covariance', 'kf_gain', 'kf_status', 'kf_steady_path'), (), ('DeltaU', 'Dhat', 'D̂', 'J', 'Khat', 'K̂', 'Phat', 'P̂', 'Rhatu', 'Rhaty', 'R̂u', 'R̂y', 'U', 'Xhat0', 'X̂0', 'Yhat', 'Yhats', 'Ztilde', 'Z̃', 'd', 'epsilon', 'kf_status', 'kf_steady_path', 'lastu', 'u', 'xhat', 'xhatend', 'x̂', 'x̂end', 'yhat', 'Ŷ', 'Ŷs', 'ŷ', 'ΔU', 'ϵ')), 'sim(2)': ('ok', ('sim_set_plant', 'sim_path', 'sim'), ())},
        'steady/predictor': {'preparestate(ym)': ('ok', (), ()), 'preparestate(NaN)': ('ok', (), ()), 'updatestate(u, ym)': ('ok', ('kf_update',), ()), 'updatestate(u)': ('ok', ('kf_update',), ('NaN values in the Kalman filter measurements ym:',)), 'setmodel': ('ok', ('set_model', 'kf_solve_steady', 'kf_status'), ()), 'setstate(x)': ('ok', (), (), (0.1, 0.2, 0.3)), 'setmodel(xhop)': ('ok', ('set_model', 'kf_solve_steady', 'kf_status'), (), (-0.4, 0.2, 0.8)), 'setstate(x, P)': ('ValueError: the SteadyKalmanFilter has no covariance', (), ()), 'setcovariances': ('ok', ('kf_set_steady', 'kf_status'), ()), 'initstate(u, ym)': ('ok', ('est_initstate',), ()), 'evaloutput': ('ok', (), ()), 'getinfo': ('ok', ('set_flags', 'prepare', 'step', 'kf_covariance', 'kf_gain', 'kf_status', 'kf_steady_path'), (), ('DeltaU', 'Dhat', 'D̂', 'J', 'Khat', 'K̂', 'Phat', 'P̂', 'Rhatu', 'Rhaty', 'R̂u', 'R̂y', 'U', 'Xhat0', 'X̂0', 'Yhat', 'Yhats', 'Ztilde', 'Z̃', 'd', 'epsilon', 'kf_status', 'kf_steady_path', 'lastu', 'u', 'xhat', 'xhatend', 'x̂', 'x̂end', 'yhat', 'Ŷ', 'Ŷs', 'ŷ', 'ΔU', 'ϵ')), 'sim(2)': ('ok', ('sim_set_plant', 'sim_path', 'sim'), ())},
        'place/filter': {'preparestate(ym)': ('ok', ('kf_correct',), ()), 'preparestate(NaN)': ('ok', ('kf_correct',), ('NaN values in the Kalman filter measurements ym:',)), 'updatestate(u, ym)': ('ok', ('kf_predict',), ()), 'updatestate(u)': ('ok', ('kf_predict',), ()), 'setmodel': ('ok', ('set_model', 'kf_place', 'kf_status'), ()), 'setstate(x)': ('ok', (), (), (0.1, 0.2, 0.3)), 'setmodel(xhop)': ('ok', ('set_model', 'kf_place', 'kf_status'), (), (-0.4, 0.2, 0.8)), 'setstate(x, P)': ('ValueError: Luenberger does not compute an', (), ()), 'setcovariances': ('ValueError: Q̂ and R̂ can only', (), ()), 'initstate(u, ym)': ('ok', ('est_initstate',), ()), 'evaloutput': ('ok', (), ()), 'getinfo': ('ok', ('set_flags', 'prepare', 'step', 'kf_gain', 'kf_status', 'kf_place_sweeps'), (), ('DeltaU', 'Dhat', 'D̂', 'J', 'Khat', 'K̂', 'Rhatu', 'Rhaty', 'R̂u', 'R̂y', 'U', 'Xhat0', 'X̂0', 'Yhat', 'Yhats', 'Ztilde', 'Z̃', 'd', 'epsilon', 'kf_status', 'lastu', 'place_sweeps', 'u', 'xhat', 'xhatend', 'x̂', 'x̂end', 'yhat', 'Ŷ', 'Ŷs', 'ŷ', 'ΔU', 'ϵ')), 'sim(2)': ('ok', ('sim_set_plant', 'sim_path', 'sim'), ())},
        'place/predictor': {'preparestate(ym)': ('ok', (), ()), 'preparestate(NaN)': ('ok', (), ()), 'updatestate(u, ym)': ('ok', ('kf_update',), ()), 'updatestate(u)': ('ok', ('kf_update',), ('NaN values in the Kalman filter measurements ym:',)), 'setmodel': ('ok', ('set_model', 'kf_place', 'kf_status'), ()), 'setstate(x)': ('ok', (), (), (0.1, 0.2, 0.3)), 'setmodel(xhop)': ('ok', ('set_model', 'kf_place', 'kf_status'), (), (-0.4, 0.2, 0.8)), 'setstate(x, P)': ('ValueError: Luenberger does not compute an', (), ()), 'setcovariances': ('ValueError: Q̂ and R̂ can only', (), ()), 'initstate(u, ym)': ('ok', ('est_initstate',), ()), 'evaloutput': ('ok', (), ()), 'getinfo': ('ok', ('set_flags', 'prepare', 'step', 'kf_gain', 'kf_status', 'kf_place_sweeps'), (), ('DeltaU', 'Dhat', 'D̂', 'J', 'Khat', 'K̂', 'Rhatu', 'Rhaty', 'R̂u', 'R̂y', 'U', 'Xhat0', 'X̂0', 'Yhat', 'Yhats', 'Ztilde', 'Z̃', 'd', 'epsilon', 'kf_status', 'lastu', 'place_sweeps', 'u', 'xhat', 'xhatend', 'x̂', 'x̂end', 'yhat', 'Ŷ', 'Ŷs', 'ŷ', 'ΔU', 'ϵ')), 'sim(2)': ('ok', ('sim_set_plant', 'sim_path', 'sim'), ())},
        'mhe/filter': {'preparestate(ym)': ('ok', ('mhe.preparestate',), ()), 'updatestate(u, ym)': ('ok', ('mhe.updatestate',), ()), 'updatestate(u)': ('ValueError: updatestate: the MovingHorizonEstimator needs ym', (), ()), 'setmodel': ('ok', ('set_model', 'mhe.setmodel'), ()), 'setstate(x)': ('ok', ('mhe.setstate',), (), (0.1, 0.2, 0.3)), 'setmodel(xhop)': ('ok', ('set_model', 'mhe.setmodel'), (), (0.1, 0.2, 0.3)), 'setstate(x, P)': ('MpcqpError: MovingHorizonEstimator does not compute an', ('mhe.setstate',), ()), 'setcovariances': ('ValueError: Q̂ and R̂ can only', (), ()), 'initstate(u, ym)': ('ok', ('est_initstate', 'mhe.initstate'), ()), 'evaloutput': ('ok', (), ()), 'getinfo': ('ok', ('set_flags', 'prepare', 'step', 'mhe.getinfo'), (), ('DeltaU', 'Dhat', 'D̂', 'J', 'Rhatu', 'Rhaty', 'R̂u', 'R̂y', 'U', 'Xhat0', 'X̂0', 'Yhat', 'Yhats', 'Ztilde', 'Z̃', 'd', 'epsilon', 'estim', 'lastu', 'u', 'xhat', 'xhatend', 'x̂', 'x̂end', 'yhat', 'Ŷ', 'Ŷs', 'ŷ', 'ΔU', 'ϵ')), 'sim(2)': ('ok', ('sim_set_plant', 'sim_path', 'sim', 'sim_est_status'), ())},
        'mhe/predictor': {'preparestate(ym)': ('ok', ('mhe.preparestate',), ()), 'updatestate(u, ym)': ('ok', ('mhe.updatestate',), ()), 'updatestate(u)': ('ValueError: updatestate: the MovingHorizonEstimator needs ym', (), ()), 'setmodel': ('ok', ('set_model', 'mhe.setmodel'), ()), 'setstate(x)': ('ok', ('mhe.setstate',), (), (0.1, 0.2, 0.3)), 'setmodel(xhop)': ('ok', ('set_model', 'mhe.setmodel'), (), (0.1, 0.2, 0.3)), 'setstate(x, P)': ('MpcqpError: MovingHorizonEstimator does not compute an', ('mhe.setstate',), ()), 'setcovariances': ('ValueError: Q̂ and R̂ can only', (), ()), 'initstate(u, ym)': ('ok', ('est_initstate', 'mhe.initstate'), ()), 'evaloutput': ('ok', (), ()), 'getinfo': ('ok', ('set_flags', 'prepare', 'step', 'mhe.getinfo'), (), ('DeltaU', 'Dhat', 'D̂', 'J', 'Rhatu', 'Rhaty', 'R̂u', 'R̂y', 'U', 'Xhat0', 'X̂0', 'Yhat', 'Yhats', 'Ztilde', 'Z̃', 'd', 'epsilon', 'estim', 'lastu', 'u', 'xhat', 'xhatend', 'x̂', 'x̂end', 'yhat', 'Ŷ', 'Ŷs', 'ŷ', 'ΔU', 'ϵ')), 'sim(2)': ('ok', ('sim_set_plant', 'sim_path', 'sim', 'sim_est_status'), ())},
        'im/filter': {'preparestate(ym)': ('ok', ('im_correct',), ()), 'preparestate(NaN)': ('ok', ('im_correct',), ('NaN values in the internal model measurements ym:',)), 'updatestate(u, ym)': ('ok', ('im_update',), ()), 'updatestate(u)': ('ok', ('im_update',), ()), 'setmodel': ('ok', ('set_model',), ()), 'setstate(x)': ('ok', (), (), (0.1, 0.2, 0.3)), 'setmodel(xhop)': ('ok', ('set_model',), (), (-0.4, 0.2, 0.8)), 'setstate(x, P)': ('ValueError: the SteadyKalmanFilter has no covariance', (), ()), 'setcovariances': ('ValueError: Q̂ and R̂ can only', (), ()), 'initstate(u, ym)': ('ok', ('est_initstate',), ()), 'evaloutput': ('ok', ('get',), ()), 'getinfo': ('ok', ('set_flags', 'prepare', 'step', 'get', 'im_status', 'get', 'get'), (), ('DeltaU', 'Dhat', 'D̂', 'J', 'Rhatu', 'Rhaty', 'R̂u', 'R̂y', 'U', 'Xhat0', 'X̂0', 'Yhat', 'Yhats', 'Ztilde', 'Z̃', 'd', 'epsilon', 'im_status', 'lastu', 'u', 'xhat', 'xhatend', 'x̂', 'x̂end', 'x̂s', 'yhat', 'Ŷ', 'Ŷs', 'ŷ', 'ŷs', 'ΔU', 'ϵ')), 'sim(2)': ('ok', ('sim_set_plant', 'sim_path', 'sim'), ())},
    },
    "refusals": {
        'two estimators / none': ('ValueError: give one of Khat (SteadyKalmanFilter),', (), (), ('-', None, None, None, True)),
        'two estimators / gain': ('ValueError: give one of Khat (SteadyKalmanFilter),', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'two estimators / tv': ('ValueError: give one of Khat (SteadyKalmanFilter),', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'two estimators / steady': ('ValueError: give one of Khat (SteadyKalmanFilter),', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'two estimators / place': ('ValueError: give one of Khat (SteadyKalmanFilter),', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'two estimators / mhe': ('ValueError: give one of Khat (SteadyKalmanFilter),', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'two estimators / im': ('ValueError: give one of Khat (SteadyKalmanFilter),', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'internal, direct=False / none': ('ValueError: direct=False: the InternalModel is always', (), (), ('-', None, None, None, True)),
        'internal, direct=False / gain': ('ValueError: direct=False: the InternalModel is always', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'internal, direct=False / tv': ('ValueError: direct=False: the InternalModel is always', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'internal, direct=False / steady': ('ValueError: direct=False: the InternalModel is always', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'internal, direct=False / place': ('ValueError: direct=False: the InternalModel is always', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'internal, direct=False / mhe': ('ValueError: direct=False: the InternalModel is always', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'internal, direct=False / im': ('ValueError: direct=False: the InternalModel is always', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe with xhat0 / none': ('ValueError: xhat0: the estimate is the', (), (), ('-', None, None, None, True)),
        'mhe with xhat0 / gain': ('ValueError: xhat0: the estimate is the', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe with xhat0 / tv': ('ValueError: xhat0: the estimate is the', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe with xhat0 / steady': ('ValueError: xhat0: the estimate is the', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe with xhat0 / place': ('ValueError: xhat0: the estimate is the', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe with xhat0 / mhe': ('ValueError: xhat0: the estimate is the', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe with xhat0 / im': {'tip': ('ValueError: xhat0: the estimate is the', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('ValueError: xhat0: the estimate is the', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'mhe, contradicting direct / none': ("ValueError: direct=False contradicts the estimator's direct=True:", (), (), ('-', None, None, None, True)),
        'mhe, contradicting direct / gain': ("ValueError: direct=False contradicts the estimator's direct=True:", (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe, contradicting direct / tv': ("ValueError: direct=False contradicts the estimator's direct=True:", (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe, contradicting direct / steady': ("ValueError: direct=False contradicts the estimator's direct=True:", (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe, contradicting direct / place': ("ValueError: direct=False contradicts the estimator's direct=True:", (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe, contradicting direct / mhe': ("ValueError: direct=False contradicts the estimator's direct=True:", (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe, contradicting direct / im': {'tip': ("ValueError: direct=False contradicts the estimator's direct=True:", (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ("ValueError: direct=False contradicts the estimator's direct=True:", (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'Khat of the wrong shape / none': {'tip': ('ValueError: Khat size must be (B,', (), (), ('-', None, None, None, True)), 'parent': ('ValueError: Khat size must be (B,', (), (), ('-', None, (0, 1), None, True))},
        'Khat of the wrong shape / gain': ('ValueError: Khat size must be (B,', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'Khat of the wrong shape / tv': {'tip': ('ValueError: Khat size must be (B,', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('ValueError: Khat size must be (B,', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'Khat of the wrong shape / steady': {'tip': ('ValueError: Khat size must be (B,', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('ValueError: Khat size must be (B,', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'Khat of the wrong shape / place': {'tip': ('ValueError: Khat size must be (B,', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('ValueError: Khat size must be (B,', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'Khat of the wrong shape / mhe': {'tip': ('ValueError: Khat size must be (B,', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('ValueError: Khat size must be (B,', (), (), ('-', True, (0, 1), None, True))},
        'Khat of the wrong shape / im': {'tip': ('ValueError: Khat size must be (B,', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('ValueError: Khat size must be (B,', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'tv: Q̂ not Hermitian / none': {'tip': ('ValueError: Q̂ must be Hermitian', (), (), ('-', None, None, None, True)), 'parent': ('ValueError: Q̂ must be Hermitian', (), (), ('-', None, (0, 1), None, True))},
        'tv: Q̂ not Hermitian / gain': ('ValueError: Q̂ must be Hermitian', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'tv: Q̂ not Hermitian / tv': ('ValueError: Q̂ must be Hermitian', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'tv: Q̂ not Hermitian / steady': ('ValueError: Q̂ must be Hermitian', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'tv: Q̂ not Hermitian / place': ('ValueError: Q̂ must be Hermitian', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'tv: Q̂ not Hermitian / mhe': ('ValueError: Q̂ must be Hermitian', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'tv: Q̂ not Hermitian / im': {'tip': ('ValueError: Q̂ must be Hermitian', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('ValueError: Q̂ must be Hermitian', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'steady: Q̂ not Hermitian / none': {'tip': ('ValueError: Q̂ must be Hermitian', (), (), ('-', None, None, None, True)), 'parent': ('ValueError: Q̂ must be Hermitian', (), (), ('-', None, (0, 1), None, True))},
        'steady: Q̂ not Hermitian / gain': ('ValueError: Q̂ must be Hermitian', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'steady: Q̂ not Hermitian / tv': ('ValueError: Q̂ must be Hermitian', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'steady: Q̂ not Hermitian / steady': ('ValueError: Q̂ must be Hermitian', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'steady: Q̂ not Hermitian / place': ('ValueError: Q̂ must be Hermitian', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'steady: Q̂ not Hermitian / mhe': ('ValueError: Q̂ must be Hermitian', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'steady: Q̂ not Hermitian / im': {'tip': ('ValueError: Q̂ must be Hermitian', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('ValueError: Q̂ must be Hermitian', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'tv: R̂ of the wrong size / none': {'tip': ('ValueError: R̂ size must be (2,', (), (), ('-', None, None, None, True)), 'parent': ('ValueError: R̂ size must be (2,', (), (), ('-', None, (0, 1), None, True))},
        'tv: R̂ of the wrong size / gain': ('ValueError: R̂ size must be (2,', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'tv: R̂ of the wrong size / tv': ('ValueError: R̂ size must be (2,', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'tv: R̂ of the wrong size / steady': ('ValueError: R̂ size must be (2,', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'tv: R̂ of the wrong size / place': ('ValueError: R̂ size must be (2,', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'tv: R̂ of the wrong size / mhe': ('ValueError: R̂ size must be (2,', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'tv: R̂ of the wrong size / im': {'tip': ('ValueError: R̂ size must be (2,', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('ValueError: R̂ size must be (2,', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'steady: R̂ of the wrong size / none': {'tip': ('ValueError: R̂ size must be (2,', (), (), ('-', None, None, None, True)), 'parent': ('ValueError: R̂ size must be (2,', (), (), ('-', None, (0, 1), None, True))},
        'steady: R̂ of the wrong size / gain': ('ValueError: R̂ size must be (2,', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'steady: R̂ of the wrong size / tv': ('ValueError: R̂ size must be (2,', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'steady: R̂ of the wrong size / steady': ('ValueError: R̂ size must be (2,', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'steady: R̂ of the wrong size / place': ('ValueError: R̂ size must be (2,', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'steady: R̂ of the wrong size / mhe': ('ValueError: R̂ size must be (2,', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'steady: R̂ of the wrong size / im': {'tip': ('ValueError: R̂ size must be (2,', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('ValueError: R̂ size must be (2,', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'complex poles / none': ('NotImplementedError: complex observer poles are not', (), (), ('-', None, None, None, True)),
        'complex poles / gain': ('NotImplementedError: complex observer poles are not', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'complex poles / tv': ('NotImplementedError: complex observer poles are not', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'complex poles / steady': ('NotImplementedError: complex observer poles are not', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'complex poles / place': ('NotImplementedError: complex observer poles are not', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'complex poles / mhe': ('NotImplementedError: complex observer poles are not', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'complex poles / im': {'tip': ('NotImplementedError: complex observer poles are not', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('NotImplementedError: complex observer poles are not', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'a pole on the unit circle / none': ('ValueError: Observer poles should be inside', (), (), ('-', None, None, None, True)),
        'a pole on the unit circle / gain': ('ValueError: Observer poles should be inside', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'a pole on the unit circle / tv': ('ValueError: Observer poles should be inside', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'a pole on the unit circle / steady': ('ValueError: Observer poles should be inside', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'a pole on the unit circle / place': ('ValueError: Observer poles should be inside', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'a pole on the unit circle / mhe': ('ValueError: Observer poles should be inside', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'a pole on the unit circle / im': {'tip': ('ValueError: Observer poles should be inside', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('ValueError: Observer poles should be inside', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'a wrong pole count / none': ('ValueError: poles length (2) ≠ nx̂', (), (), ('-', None, None, None, True)),
        'a wrong pole count / gain': ('ValueError: poles length (2) ≠ nx̂', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'a wrong pole count / tv': ('ValueError: poles length (2) ≠ nx̂', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'a wrong pole count / steady': ('ValueError: poles length (2) ≠ nx̂', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'a wrong pole count / place': ('ValueError: poles length (2) ≠ nx̂', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'a wrong pole count / mhe': ('ValueError: poles length (2) ≠ nx̂', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'a wrong pole count / im': {'tip': ('ValueError: poles length (2) ≠ nx̂', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('ValueError: poles length (2) ≠ nx̂', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'stoch_ym with a zero Ds / none': ('ValueError: Stochastic model requires a nonzero', (), (), ('-', None, None, None, True)),
        'stoch_ym with a zero Ds / gain': ('ValueError: Stochastic model requires a nonzero', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'stoch_ym with a zero Ds / tv': ('ValueError: Stochastic model requires a nonzero', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'stoch_ym with a zero Ds / steady': ('ValueError: Stochastic model requires a nonzero', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'stoch_ym with a zero Ds / place': ('ValueError: Stochastic model requires a nonzero', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'stoch_ym with a zero Ds / mhe': ('ValueError: Stochastic model requires a nonzero', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'stoch_ym with a zero Ds / im': ('ValueError: Stochastic model requires a nonzero', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'gain: i_ym out of range / none': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('-', None, None, None, False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('-', False, (0, 2), None, False))},
        'gain: i_ym out of range / gain': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('-', False, (0, 2), (0.0, 0.0, 0.0), False))},
        'gain: i_ym out of range / tv': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('-', False, (0, 2), (0.0, 0.0, 0.0), False))},
        'gain: i_ym out of range / steady': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('-', False, (0, 2), (0.0, 0.0, 0.0), False))},
        'gain: i_ym out of range / place': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('-', False, (0, 2), (0.0, 0.0, 0.0), False))},
        'gain: i_ym out of range / mhe': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('-', False, (0, 2), None, False))},
        'gain: i_ym out of range / im': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('-', True, (0, 2), (0.0, 0.0, 0.0), True))},
        'gain: i_ym repeated / none': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('-', None, None, None, False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('-', False, (1, 1), None, False))},
        'gain: i_ym repeated / gain': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('-', False, (1, 1), (0.0, 0.0, 0.0), False))},
        'gain: i_ym repeated / tv': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('-', False, (1, 1), (0.0, 0.0, 0.0), False))},
        'gain: i_ym repeated / steady': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('-', False, (1, 1), (0.0, 0.0, 0.0), False))},
        'gain: i_ym repeated / place': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('-', False, (1, 1), (0.0, 0.0, 0.0), False))},
        'gain: i_ym repeated / mhe': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set'), (), ('-', False, (1, 1), None, False))},
        'gain: i_ym repeated / im': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('-', True, (1, 1), (0.0, 0.0, 0.0), True))},
        'tv: i_ym out of range / none': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('-', None, None, None, False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('-', False, (0, 2), None, False))},
        'tv: i_ym out of range / gain': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('-', False, (0, 2), (0.0, 0.0, 0.0), False))},
        'tv: i_ym out of range / tv': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_timevarying', False, (0, 2), (0.0, 0.0, 0.0), False))},
        'tv: i_ym out of range / steady': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_steady', False, (0, 2), (0.0, 0.0, 0.0), False))},
        'tv: i_ym out of range / place': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_luenberger', False, (0, 2), (0.0, 0.0, 0.0), False))},
        'tv: i_ym out of range / mhe': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('mhe', False, (0, 2), (0.0, 0.0, 0.0), False))},
        'tv: i_ym out of range / im': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('-', True, (0, 2), (0.0, 0.0, 0.0), True))},
        'tv: i_ym repeated / none': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('-', None, None, None, False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('-', False, (1, 1), None, False))},
        'tv: i_ym repeated / gain': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('-', False, (1, 1), (0.0, 0.0, 0.0), False))},
        'tv: i_ym repeated / tv': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_timevarying', False, (1, 1), (0.0, 0.0, 0.0), False))},
        'tv: i_ym repeated / steady': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_steady', False, (1, 1), (0.0, 0.0, 0.0), False))},
        'tv: i_ym repeated / place': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('kf_luenberger', False, (1, 1), (0.0, 0.0, 0.0), False))},
        'tv: i_ym repeated / mhe': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_covariances'), (), ('mhe', False, (1, 1), (0.0, 0.0, 0.0), False))},
        'tv: i_ym repeated / im': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('-', True, (1, 1), (0.0, 0.0, 0.0), True))},
        'steady: i_ym out of range / none': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('-', None, None, None, False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('-', False, (0, 2), None, False))},
        'steady: i_ym out of range / gain': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('-', False, (0, 2), (0.0, 0.0, 0.0), False))},
        'steady: i_ym out of range / tv': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('kf_timevarying', False, (0, 2), (0.0, 0.0, 0.0), False))},
        'steady: i_ym out of range / steady': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('kf_steady', False, (0, 2), (0.0, 0.0, 0.0), False))},
        'steady: i_ym out of range / place': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('kf_luenberger', False, (0, 2), (0.0, 0.0, 0.0), False))},
        'steady: i_ym out of range / mhe': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('mhe', False, (0, 2), (0.0, 0.0, 0.0), False))},
        'steady: i_ym out of range / im': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('-', True, (0, 2), (0.0, 0.0, 0.0), True))},
        'steady: i_ym repeated / none': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('-', None, None, None, False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('-', False, (1, 1), None, False))},
        'steady: i_ym repeated / gain': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('-', False, (1, 1), (0.0, 0.0, 0.0), False))},
        'steady: i_ym repeated / tv': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('kf_timevarying', False, (1, 1), (0.0, 0.0, 0.0), False))},
        'steady: i_ym repeated / steady': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('kf_steady', False, (1, 1), (0.0, 0.0, 0.0), False))},
        'steady: i_ym repeated / place': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('kf_luenberger', False, (1, 1), (0.0, 0.0, 0.0), False))},
        'steady: i_ym repeated / mhe': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), False)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct', 'kf_set_steady'), (), ('mhe', False, (1, 1), (0.0, 0.0, 0.0), False))},
        'steady: i_ym repeated / im': {'tip': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('MpcqpError: mpcqp error -3: illegal argument', ('kf_set_direct',), (), ('-', True, (1, 1), (0.0, 0.0, 0.0), True))},
        'place: i_ym out of range / none': ('ValueError: i_ym: unique indices of measured', (), (), ('-', None, None, None, True)),
        'place: i_ym out of range / gain': ('ValueError: i_ym: unique indices of measured', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'place: i_ym out of range / tv': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'place: i_ym out of range / steady': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'place: i_ym out of range / place': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'place: i_ym out of range / mhe': ('ValueError: i_ym: unique indices of measured', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'place: i_ym out of range / im': {'tip': ('ValueError: i_ym: unique indices of measured', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('ValueError: i_ym: unique indices of measured', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'place: i_ym repeated / none': ('ValueError: i_ym: unique indices of measured', (), (), ('-', None, None, None, True)),
        'place: i_ym repeated / gain': ('ValueError: i_ym: unique indices of measured', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'place: i_ym repeated / tv': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'place: i_ym repeated / steady': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'place: i_ym repeated / place': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'place: i_ym repeated / mhe': ('ValueError: i_ym: unique indices of measured', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'place: i_ym repeated / im': {'tip': ('ValueError: i_ym: unique indices of measured', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('ValueError: i_ym: unique indices of measured', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'mhe: i_ym out of range / none': ('ValueError: i_ym: unique indices of measured', (), (), ('-', None, None, None, True)),
        'mhe: i_ym out of range / gain': ('ValueError: i_ym: unique indices of measured', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe: i_ym out of range / tv': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe: i_ym out of range / steady': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe: i_ym out of range / place': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe: i_ym out of range / mhe': ('ValueError: i_ym: unique indices of measured', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe: i_ym out of range / im': {'tip': ('ValueError: i_ym: unique indices of measured', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('ValueError: i_ym: unique indices of measured', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'mhe: i_ym repeated / none': ('ValueError: i_ym: unique indices of measured', (), (), ('-', None, None, None, True)),
        'mhe: i_ym repeated / gain': ('ValueError: i_ym: unique indices of measured', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe: i_ym repeated / tv': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe: i_ym repeated / steady': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe: i_ym repeated / place': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe: i_ym repeated / mhe': ('ValueError: i_ym: unique indices of measured', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'mhe: i_ym repeated / im': {'tip': ('ValueError: i_ym: unique indices of measured', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)), 'parent': ('ValueError: i_ym: unique indices of measured', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True))},
        'im: i_ym out of range / none': ('ValueError: i_ym: unique indices of measured', (), (), ('-', None, None, None, True)),
        'im: i_ym out of range / gain': ('ValueError: i_ym: unique indices of measured', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'im: i_ym out of range / tv': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'im: i_ym out of range / steady': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'im: i_ym out of range / place': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'im: i_ym out of range / mhe': ('ValueError: i_ym: unique indices of measured', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'im: i_ym out of range / im': ('ValueError: i_ym: unique indices of measured', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'im: i_ym repeated / none': ('ValueError: i_ym: unique indices of measured', (), (), ('-', None, None, None, True)),
        'im: i_ym repeated / gain': ('ValueError: i_ym: unique indices of measured', (), (), ('-', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'im: i_ym repeated / tv': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_timevarying', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'im: i_ym repeated / steady': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_steady', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'im: i_ym repeated / place': ('ValueError: i_ym: unique indices of measured', (), (), ('kf_luenberger', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'im: i_ym repeated / mhe': ('ValueError: i_ym: unique indices of measured', (), (), ('mhe', True, (0, 1), (0.0, 0.0, 0.0), True)),
        'im: i_ym repeated / im': ('ValueError: i_ym: unique indices of measured', (), (), ('internal', True, (0, 1), (0.0, 0.0, 0.0), True)),
    },
}


if __name__ == "__main__":
    main(sys.argv[1:])
