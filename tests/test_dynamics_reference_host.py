"""CPU side of the dynamics-path tests: the host-compiled device arithmetic (tests/hostcheck/hostcheck.cpp) and the fp64 NumPy oracle
through the longdouble reference of tests/dynamics_reference.py, the oracle's figures that set the bars of
tests/test_gpu_dynamics_paths.py, the conditions on the cases of tests/dynamics_cases.py, and planted faults that ``judge`` must
see.  No GPU.

The oracle's largest figure per quantity over all cases of tests/dynamics_cases.py, in units of 2^-53 (``ORACLE_MAX`` below; the bar
of a case is max(16, 4 x its own figure)):

  1 s chain   x_hat pos 7.7  vel 9.4   Phi pos cols 15.3  vel cols 10.1   r_orbit 10.2
  hop         x_hat pos 0.9  vel 0.9   Phi pos cols 1.0   vel cols 2.7    r_orbit 2.6
  attitude    f 1.3   qgrad 2.3   Hl 3.3   Hd 3.0   Hu 3.3
  assembly    bands 4.6 (BA_reg 4.6)   rhs 4.7   last_hessian 2.4   initial mean 2.4
  landmark    step_fwd 1.1 (Gauss-Jordan without row exchanges per 6x6 block in NumPy; the oracle's banded LU of the 9n system:
              4.2), retract 3.8

The host-compiled device arithmetic stands within the same bars on c2 and on every new case (printed by
test_device_arithmetic_through_the_reference)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dynamics_cases as C
import dynamics_reference as R
from conftest import ROOT, golden_inputs
from oracle import ba_oracle as O

SRC = os.path.join(ROOT, "tests", "hostcheck", "hostcheck.cpp")
LIB = os.path.join(ROOT, "tests", "hostcheck", "libhostcheck.so")
P = ctypes.POINTER(ctypes.c_double)
PI = ctypes.POINTER(ctypes.c_int64)
ORACLE_MAX = dict(xhat_p=7.7, xhat_v=9.4, Phi_p=15.3, Phi_v=10.1, r_orbit=10.2, f=1.3, qgrad=2.3, Hl=3.3, Hd=3.0, Hu=3.3, bands=4.6,
                  rhs=4.7, last_hessian=2.4, sum_init=2.4, step_fwd=1.1, retract=3.8)
_LV = {}


def _p(a):
    return a.ctypes.data_as(P)


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


@pytest.fixture(scope="module")
def hc():
    hdr = os.path.join(ROOT, "vinsat_amd", "csrc", "vba_math.h")
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    if not hasattr(lib, "hc_step6"):         # a library built from an older source with a newer time stamp
        subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
        lib = ctypes.CDLL(LIB)
    return lib


def levels(c, init=False, hop=False, reg=False):
    key = (c.name, init, hop, reg)
    if key not in _LV:
        it, lam = (C.IT_INIT, C.LAM_INIT) if init else (C.IT, C.LAM)
        _LV[key] = R.oracle_levels(c.args(), it, lam, init, hop=hop, prior=c.prior() if reg else None)
    return _LV[key]


def _c2_case(c2, k):
    inp = golden_inputs(c2)
    st = _c(c2[f"states_in_{k}"][0])
    return C.Case(f"c2[{k}]", st, inp["xyz"], inp["uv"], inp["conf"], np.asarray(inp["ii"], dtype=np.int64), inp["K"], inp["cumrot"],
                  np.asarray(inp["time_idx"], dtype=np.int64), st)


def device_arrays(hc, c, lv, init=False, hop=False, reg=False):
    """What a fetch would hand out if the kernels were the host-compiled device arithmetic: the factor from hc_orbit(_hop) /
    hc_attitude at the case's states, the system from hc_assemble(_reg) on that factor and the oracle's per-pose sums, the
    landmark-only step from hc_step6 / hc_retract."""
    st, n = _c(c.states), c.n
    dbg = lv.oracle["dbg"]
    wmax = float(dbg["wmax"])
    iu = np.triu_indices(6)
    Hraw, braw = _c((dbg["H"] * wmax)[:, iu[0], iu[1]]), _c(dbg["b"] * wmax)
    sym = np.zeros((6, 6), dtype=np.int64)
    sym[iu] = np.arange(21)
    sym = np.maximum(sym, sym.T)
    d = dict(H=Hraw[:, sym] / wmax, b=braw / wmax)
    lam32 = lv.oracle["lam32"]
    z = lambda *s: np.zeros(s)
    bands, rhs = z(n, 3, 9, 9), z(n, 9)
    if init:
        d.update(Phi=z(n, 6, 6), r_pred=z(n - 1, 7), qgrad=z(n, 3), Hq=z(n, 3, 3, 3))
        hc.hc_assemble(n, _p(Hraw), _p(braw), ctypes.c_double(1 / wmax), ctypes.c_double(0.0), _p(z(n, 36)), _p(z(n, 6)), _p(z(n, 3)),
                       _p(z(n, 9)), _p(z(n, 9)), _p(z(n, 9)), _p(bands), _p(rhs))
        dpose, out = z(n, 9), z(n, 10)
        hc.hc_step6(n, _p(Hraw), _p(braw), ctypes.c_double(1 / wmax), ctypes.c_double(lam32), _p(dpose))
        hc.hc_retract(n, _p(st), _p(dpose), _p(out))
        d.update(dpose=dpose, out=out)
    else:
        steps = O.step_counts(c.t)
        xhat, Phi = z(n, 6), z(n, 6, 6)
        if hop:
            x6 = _c(np.concatenate([st[:, :3], st[:, 7:]], 1))
            hc.hc_orbit_hop(n, _p(x6), steps.ctypes.data_as(PI), _p(xhat), _p(Phi))
        else:
            hc.hc_orbit(n, _p(st), steps.ctypes.data_as(PI), _p(xhat), _p(Phi))
        x = np.concatenate([st[:, :3], st[:, 7:]], 1)
        rorb = z(n, 6)
        rorb[:-1] = (xhat[:-1] - x[1:]) * R.D6           # (the kernels: x_hat - x_next, the velocity rows times 100)
        f, qgrad = z(n), z(n, 3)
        Hd, Hu, Hl = z(n, 3, 3), z(n, 3, 3), z(n, 3, 3)
        hc.hc_attitude(n, _p(st), _p(_c(c.cumrot)), _p(f), _p(qgrad), _p(Hd), _p(Hu), _p(Hl))
        sigma = ctypes.c_double(float(lv.oracle["sigma"]))
        if reg:
            sp, Hs = c.prior()
            px = _c(np.concatenate([sp[:, :3], sp[:, 7:]], 1))
            hc.hc_assemble_reg(n, _p(Hraw), _p(braw), ctypes.c_double(1 / wmax), sigma, _p(Phi), _p(rorb), _p(qgrad), _p(Hd), _p(Hu),
                               _p(Hl), _p(_c(Hs)), _p(px), _p(st), _p(bands), _p(rhs))
        else:
            hc.hc_assemble(n, _p(Hraw), _p(braw), ctypes.c_double(1 / wmax), sigma, _p(Phi), _p(rorb), _p(qgrad), _p(Hd), _p(Hu), _p(Hl),
                           _p(bands), _p(rhs))
        d.update(Phi=Phi, r_pred=np.concatenate([rorb[:-1], f[:-1, None]], 1), qgrad=qgrad, Hq=np.stack([Hl, Hd, Hu], 1))
    hess = bands[-1, 1] + lam32 * np.eye(9)
    d.update(bands=bands, rhs=rhs, hess=hess, lam32=lam32, sigma=float(lv.oracle["sigma"]), est=dbg["est"])
    return d


def judge_arrays(c, d, lv, init=False, hop=False, reg=False):
    prior = c.prior() if reg else None
    if init:
        figs, exact = R.step_layer(d["dpose"], d["out"], d["H"], d["b"], d["lam32"], c.states)
    else:
        figs, exact = R.factor_layer(c.states, c.t, c.cumrot, d["Phi"], d["r_pred"], d["qgrad"], d["Hq"], hop)
    g, e2 = R.assembly_layer(d["bands"], d["rhs"], d["hess"], d["lam32"], d["H"], d["b"], d["sigma"], d["Phi"], d["r_pred"], d["qgrad"],
                             d["Hq"], init, prior, c.states)
    figs.update(g)
    if "sum_init" in d:
        pr = (R.prior_ld(c.states, prior)[0] if not init else np.zeros((c.n, 6))) if reg else None
        pden = R.prior_ld(c.states, prior, absolute=True)[0] if reg and not init else None
        ref, den = R.residual_sums_ld(c.uv, d["est"], None, d["r_pred"], d["sigma"], c.n, init, pr, prior_den=pden)
        figs["sum_init"] = R.sums_figure(d["sum_init"], ref, den)
    return R.judge(lv, figs, exact + e2)


# ------------------------------------------------------------------------------------------------ the device arithmetic, the oracle
HOST_CASES = [(2, "mixed"), (5, "mixed"), (17, "steps64"), (33, "long31"), (129, "mixed")]


@pytest.mark.parametrize("what", ["full", "hop", "reg", "init"])
def test_device_arithmetic_through_the_reference(hc, c2, what):
    init, hop, reg = what == "init", what == "hop", what == "reg"
    cases = [C.case(n, kind) for n, kind in HOST_CASES]
    if what in ("full", "init"):
        cases.append(_c2_case(c2, 9 if init else 10))
    bad = []
    for c in cases:
        if c.name.startswith("c2"):
            it, lam = int(c2["iters"][9 if init else 10]), float(c2["lamda_in"][9 if init else 10])
            lv = R.oracle_levels(c.args(), it, lam, init, need_accept=False)
        else:
            lv = levels(c, init, hop, reg)
        v = judge_arrays(c, device_arrays(hc, c, lv, init, hop, reg), lv, init, hop, reg)
        print(f"FIGURES {c.name} {what}: host-compiled device arithmetic (oracle): "
              + " ".join(f"{k} {v.units[k]:.2f} ({lv.units[k]:.2f})" for k in v.units))
        bad += [f"{c.name} {what}: {f}" for f in v.failures]
    assert not bad, "\n".join(bad)


def test_oracle_figures():
    """The table of the module docstring: the oracle through the reference on every case and call kind.  ``oracle_levels`` asserts the
    conditions (no figure above 1024 units, exact zeros where nothing is summed, the first trial accepted); the recorded maxima
    hold to a factor of 1.5 (another NumPy may sum a product in another order)."""
    worst = {}
    for n, kind in C.factor_cases():
        c = C.case(n, kind)
        kinds = [(False, False, False), (False, True, False), (False, False, True)] + ([(True, False, False)] if kind == "mixed" else [])
        for init, hop, reg in kinds:
            for k, v in levels(c, init, hop, reg).units.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("FIGURES oracle maxima: " + " ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert set(worst) == set(ORACLE_MAX)
    for k, v in worst.items():
        assert v <= 1.5 * ORACLE_MAX[k], (k, v, ORACLE_MAX[k])


# ------------------------------------------------------------------------------------------------ conditions on the cases
def test_every_block_boundary_lies_inside_a_window():
    ns = sorted({n for n, _ in C.factor_cases()})
    for B in C.BOUNDARIES:
        assert B - 1 in ns and B in ns and B + 1 in ns, B        # the boundary behind the last pose, on it, and with a live pose behind it
    assert max(C.RAGGED) == 129 and min(C.RAGGED) == 2 and 33 in C.RAGGED and 128 in C.RAGGED
    for n, kind in C.factor_cases():
        c = C.case(n, kind)
        g = np.diff(c.t)
        assert c.n == n and g.min() >= 1 and np.bincount(c.ii, minlength=n).min() >= 3 and np.bincount(c.ii).max() <= 6
        if kind == "mixed":
            assert g.max() <= 60 and (n < 3 or np.any(g[1:] != g[:-1]))
        if kind == "steps64":
            assert g[0] == 64 and (n == 2 or g[1] == 1) and g.max() == 64
        if kind.startswith("long"):
            k = int(kind[4:])
            assert g[k] == 65 and np.count_nonzero(g > 64) == 1 and k in (31, 32) and n > k + 1


def test_every_pose_weighs_a_hundred_bars_in_the_residual_sum():
    """sqrt(sigma) sum |r_pred_i| of every edge over the whole sum of the initial mean against 100 x K x 2^-53 of ``sum_init``: a
    dropped pose cannot hide in the bar."""
    for n, kind in C.factor_cases():
        c = C.case(n, kind)
        for reg in (False, True):
            lv = levels(c, reg=reg)
            sh = R.pred_shares(lv.oracle["fac"]["r_pred"], lv.oracle["sigma"], lv.oracle["sum_total"])
            assert sh.min() > 100 * lv.K("sum_init") * R.U, (c.name, reg, float(sh.min()), int(np.argmin(sh)))


# ------------------------------------------------------------------------------------------------ planted faults
def _clean(c, init=False, reg=False):
    """The oracle's own arrays as a fetch would hand them out."""
    lv = levels(c, init=init, reg=reg)
    o = lv.oracle
    dbg = o["dbg"]
    d = dict(H=dbg["H"].copy(), b=dbg["b"].copy(), bands=dbg["bands"].copy(), rhs=dbg["rhs"].copy(), hess=o["hess"].copy(),
             lam32=o["lam32"], sigma=float(o["sigma"]), est=dbg["est"], sum_init=dbg["init_residual"])
    d.update({k: o["fac"][k].copy() for k in ("Phi", "r_pred", "qgrad", "Hq")})
    if init:
        d.update(dpose=dbg["trials"][0]["dpose"].copy(), out=o["out"].copy())
    return d, lv


def _assemble_from(c, d, fac, reg=False, keep_last=False):
    """The oracle's assembly from a factor ``fac`` (dict Phi, r_pred, qgrad, Hq) -- what a kernel that read the wrong input forms."""
    n = c.n
    D = R.D6
    E = np.zeros((n - 1, 6, 9))
    DPhi = D[None, :, None] * fac["Phi"][:-1]
    E[:, :, 0:3], E[:, :, 6:9] = DPhi[:, :, 0:3], DPhi[:, :, 3:6]
    F = np.zeros((6, 9))
    F[0:3, 0:3] = -np.eye(3)
    F[3:6, 6:9] = -O.VEL_COEFF * np.eye(3)
    Hq = fac["Hq"]
    bands, rhs = O.assemble(d["H"], d["b"], 1.0, d["sigma"], E, F, fac["r_pred"][:, :6], fac["qgrad"], Hq[:, 1], Hq[:-1, 2], Hq[1:, 0], False)
    if reg:
        rp, Jp = O.prior_factor(c.states, *c.prior(), vel_coeff=1.0)
        bands[:, 1] += np.einsum("irc,ird->icd", Jp, Jp)
        rhs -= np.einsum("irc,ir->ic", Jp, rp)
    return bands, rhs


FAULTS = ("phi-columns-swapped", "halo-phi-from-the-neighbour", "last-propagation-kept", "velocity-coefficient-missing", "sigma-missing",
          "Hu-Hl-exchanged", "prior-missing", "lamda-not-float32", "pose-dropped-from-the-sum", "band-entry-1e-9")


def _fault(name):
    """(case, arrays, kwargs of judge_arrays, the figures that must fail)."""
    c = C.case(33, "mixed")
    reg, init = name == "prior-missing", name == "lamda-not-float32"
    d, lv = _clean(c, init=init, reg=reg)
    kw = dict(init=init, reg=reg)
    if name == "phi-columns-swapped":           # half == 1 writes tangent 4 where 5 belongs
        d["Phi"][5][:, [4, 5]] = d["Phi"][5][:, [5, 4]]
        return c, d, lv, kw, {"Phi_v"}
    if name == "halo-phi-from-the-neighbour":   # pose 16, the first of its block: Phi_{i-1} staged from pose 16 instead of 15
        fac = {k: d[k].copy() for k in ("Phi", "r_pred", "qgrad", "Hq")}
        fac["Phi"][15] = d["Phi"][16]
        b2, r2 = _assemble_from(c, d, fac)
        d["bands"][16], d["rhs"][16] = b2[16], r2[16]
        return c, d, lv, kw, {"bands"}
    if name == "last-propagation-kept":
        st = c.states
        x = np.concatenate([st[:, :3], st[:, 7:]], 1)
        xh, Phi = O.propagate_orbit(x[-1:], np.array([1]))
        E = np.zeros((6, 9))
        E[:, 0:3], E[:, 6:9] = (R.D6[:, None] * Phi[0])[:, 0:3], (R.D6[:, None] * Phi[0])[:, 3:6]
        d["bands"][-1, 1] += d["sigma"] * E.T @ E
        return c, d, lv, kw, {"bands"}
    if name == "velocity-coefficient-missing":
        d["r_pred"][7, 3:6] /= 100.0
        return c, d, lv, kw, {"r_orbit", "xhat_v"}
    if name == "sigma-missing":
        d["bands"][9, 1, 3:6, 3:6] += (1.0 - d["sigma"]) * d["Hq"][9, 1]
        return c, d, lv, kw, {"bands"}
    if name == "Hu-Hl-exchanged":
        d["Hq"][12, [0, 2]] = d["Hq"][12, [2, 0]]
        return c, d, lv, kw, {"Hu", "Hl"}
    if name == "prior-missing":
        fac = {k: d[k] for k in ("Phi", "r_pred", "qgrad", "Hq")}
        b2, r2 = _assemble_from(c, d, fac, reg=False)
        d["bands"][12], d["rhs"][12] = b2[12], r2[12]
        return c, d, lv, kw, {"bands", "rhs"}
    if name == "lamda-not-float32":
        A = d["H"] + C.LAM_INIT * np.eye(6)
        d["dpose"][:, :6] = np.linalg.solve(A, d["b"][:, :, None])[:, :, 0]
        d["out"] = O.retract(c.states, d["dpose"])
        return c, d, lv, kw, {"step_fwd"}
    if name == "pose-dropped-from-the-sum":
        m = c.m
        d["sum_init"] = d["sum_init"] - np.sqrt(d["sigma"]) * np.abs(d["r_pred"][17]).sum() / (2 * m + 7 * (c.n - 1))
        return c, d, lv, kw, {"sum_init"}
    if name == "band-entry-1e-9":
        d["bands"][20, 2, 7, 1] *= 1.0 + 1e-9
        return c, d, lv, kw, {"bands"}
    raise KeyError(name)


@pytest.mark.parametrize("what", ["full", "reg", "init"])
def test_clean_arrays_pass(what):
    c = C.case(33, "mixed")
    d, lv = _clean(c, init=what == "init", reg=what == "reg")
    v = judge_arrays(c, d, lv, init=what == "init", reg=what == "reg")
    assert v.ok, v.failures


def test_a_step_solved_with_the_float32_damping_passes():
    """The clean counterpart of the ``lamda-not-float32`` fault: the same per-pose solve with float32(lamda)."""
    c = C.case(33, "mixed")
    d, lv = _clean(c, init=True)
    d["dpose"][:, :6] = np.linalg.solve(d["H"] + d["lam32"] * np.eye(6), d["b"][:, :, None])[:, :, 0]
    d["out"] = O.retract(c.states, d["dpose"])
    v = judge_arrays(c, d, lv, init=True)
    assert v.ok, v.failures


@pytest.mark.parametrize("name", FAULTS)
def test_planted_fault(name):
    c, d, lv, kw, must = _fault(name)
    v = judge_arrays(c, d, lv, **kw)
    failing = {k for k in v.units if not v.units[k] <= v.bars[k]}
    print(f"FIGURES fault {name}: " + " ".join(f"{k} {v.units[k]:.3g} (K {v.bars[k]:.3g})" for k in sorted(failing)))
    assert must <= failing, (name, must, failing, v.failures)
    # the failure names the pose the fault was planted at
    assert not v.ok
