"""The part of a BA call between the accumulation and the solve, on every path and on the block edges of its index arithmetic:
the orbit-dynamics factor with its transition matrix, the attitude Newton term, the block-tridiagonal assembly, the landmark-only
step and the block partials behind the accept test (vinsat_amd/csrc/vba_dyn.hip, vba_dyn_body.h, vba_asm.h, vba_asm_fast.h).

One BA call per case at the case's states (tests/dynamics_cases.py: pose counts on the boundaries of 4, 16, 32, 128 and 256 poses
per block, mixed gaps, a 64-step gap beside a 1-step gap, a long edge at the last / first pose of a dynamics block), then
``vba_debug_fetch``.  tests/dynamics_reference.py judges in two layers, componentwise, per pose: the factor against the longdouble
factor at the input states, and bands / rhs / last_hessian / the landmark-only step / the means of the accept test against the
longdouble restatement formed from the device's OWN H, b, Phi, r_pred, qgrad, Hq, rows and prior.  A figure passes at K x 2^-53,
K = max(16, 4 x the fp64 NumPy oracle's figure on the same case); tests/test_dynamics_reference_host.py holds the oracle's
figures, the conditions on the cases and the planted faults.

Where each test lands (enqueue_front, launch_dynamics, launch_assemble):

  test_factor[latency]      mode 1: dynamics_block riding in the grid of k_obs_accumulate (dyn_in_acc)
  test_factor[profiled]     mode 1 through ``step_profiled``: k_dynamics as its own launch (``ride`` is off under ``prof``)
  test_factor[bandwidth]    mode 0: k_dynamics_pair on the second stream
  test_factor[hop]          mode 1 with the hop integrator (one RK4 step of the whole gap below 100 s; a 65 s edge stays on the lanes)
                            In every one of them ``bands`` / ``rhs`` are formed by the assembly launched for the fetch: default mask
                            (bit 3 on): k_assemble_rows<4, false> (mode 1) / k_assemble_rows<16, false> (mode 0).
  test_assembly             fusion mask 1 (bits 1, 2, 3 off: the solve forms no blocks, the per-entry form) and 9 (bit 3: the
                            uniform-pass form); mode 1: k_assemble<false, 4, REG> / k_assemble_rows<4, REG>, mode 0:
                            k_assemble<false, 16, REG> / k_assemble_rows<16, REG>; REG = BA_reg with a per-pose prior
  test_landmark_only        mode 1, mask 14 (bit 0 off: the trial kernel does not form the step): k_assemble<true, 4, false>;
                            mode 0: k_init_step (launch_assemble sends every fused landmark-only call of a bandwidth-mode handle
                            there: k_assemble<true, 16, false> is instantiated but has no caller)
  test_residual_sums        two calls on one handle (both parities of part_pred / part_prior), the long-edge variants included (the
                            slots behind nblk_pred), both kernel sets, plain and BA_reg; the trial mean of the first call against
                            the rows and the factor the second call reports at the trial states
  test_ragged_batch         windows of 129, 2, 33, 128 poses on a handle with n_max = 129, both kernel sets, plain and BA_reg: every
                            window by the same bars and bit-equal to the same window alone on a handle of its own size

Measured on the MI355X: the largest figure per quantity in units of 2^-53, in brackets the oracle's figure on the case that gave it
(the bar is max(16, 4 x the bracket)); docs/NOTEBOOK.md has the same table with every column.

  path                               x_hat pos / vel            Phi pos / vel cols           r_orbit        f / qgrad / Hl / Hd / Hu
  latency = profiled = bandwidth     7.65 (7.65) / 9.31 (9.31)  15.23 (15.23) / 10.09 (10.09)  10.14 (10.14)  1.17 / 1.73 / 2.43 / 2.98 / 2.64
  hop                                0.84 (0.81) / 0.86 (0.86)  1.00 (1.00) / 2.69 (2.69)      1.96 (1.65)    (1.17 / 1.64 / 3.28 / 2.50 / 2.45)

  path                               bands        rhs          last_hessian  initial mean
  factor tests (rows form)           3.97 (3.91)  4.41 (4.41)  2.82 (1.38)   1.94 (1.18)      hop: 4.33 (4.40)  4.13 (4.13)  2.82  2.11 (1.19)
  test_assembly, all four kernels    3.93 (3.45)  2.76 (2.77)  2.82 (1.38)   1.66 (0.07)
  ... with REG                       3.85 (3.95)  3.57 (3.57)  2.82 (1.50)   1.86 (1.44)
  ragged batch                       3.91 (3.89)  3.57 (3.57)  2.02 (2.02)   0.89 (0.30)
  landmark-only k_assemble<FUSE, 4>  step_fwd 1.17 (0.82)  retract 3.98 (3.49)  diagonal blocks / rhs / last_hessian 2.00 / 2.00 / 1.96
  landmark-only k_init_step          step_fwd 1.16 (0.84)  retract 3.56 (3.49)  the same; initial mean 1.76 (0.96)
  residual sums, two calls           initial mean 1.66 .. 1.97, trial mean of call 1 against the rows of call 2: 0.01 .. 0.32

Nothing comes near a bar and no kernel changed.  The three forms of the dynamics kernel left the same bits in the initial mean on
every case; every window of the ragged batch carried the bits of the same window alone (the bandwidth-mode handles with the solve
pinned to one window per wavefront: the default partition follows n_max).
"""
import numpy as np
import pytest

import dynamics_cases as C
import dynamics_reference as R

pytestmark = pytest.mark.gpu

_LEVELS = {}
FIGURES = {}                    # (path, quantity) -> [device units, oracle units on that case, where]


def levels(c, it=C.IT, lam=C.LAM, init=False, hop=False, reg=False, states=None, tag="", accept=True):
    key = (c.name, it, init, hop, reg, tag)
    if key not in _LEVELS:
        _LEVELS[key] = R.oracle_levels(c.args(states), it, lam, init, hop=hop, prior=c.prior() if reg else None, need_accept=accept)
    return _LEVELS[key]


def engine(n_max, m_max, windows=1, mode=1, hop=False, fusion=None):
    from vinsat_amd.engine import BAEngine
    e = BAEngine(n_max, m_max, windows=windows, mode=mode)
    if hop:
        e.set_integrator(True)
    if fusion is not None:
        e.set_fusion(fusion)
    return e


def upload(e, c, k=0, reg=False, lam=C.LAM):
    e.upload_observations(c.xyz, c.uv, c.conf, c.ii, c.n, window=k)
    e.upload_window(c.K, c.cumrot, c.t, window=k)
    if reg:
        e.upload_prior(*c.prior(), window=k)
    e.set_states(c.states, lam, window=k)


WHAT = ("Phi", "r_pred", "qgrad", "Hq", "H", "b", "bands", "rhs", "scalars", "dpose", "est", "weight")


def fetch(e, k=0):
    d = {w: e.debug(w, window=k) for w in WHAT}
    d["out"], d["lam"], d["hess"], d["ntr"], d["flags"] = e.get_states(window=k)
    return d


def _note(path, v, lv):
    for k in v.units:
        cur = FIGURES.setdefault((path, k), [0.0, 0.0, None])
        if v.units[k] >= cur[0]:
            FIGURES[(path, k)] = [v.units[k], lv.units.get(k, float("nan")), v.where[k]]


def check_full(c, d, lv, path, where, hop=False, reg=False, states=None, lam=C.LAM, one_trial=True):
    """A full-phase call: both layers and the initial mean.  [] or what is out of bounds, each line with case, path, window, pose, entry."""
    st = c.states if states is None else states
    prior = c.prior() if reg else None
    bad = []
    if d["flags"] & ~1 or (one_trial and (d["flags"] != 0 or d["ntr"] != 1)):
        bad.append(f"{where}: flags {d['flags']}, {d['ntr']} trials (the case asks for one accepted trial)")
    sigma, lam32 = d["scalars"][5], d["scalars"][4]
    if lam32 != float(np.float32(lam)):
        bad.append(f"{where}: damping {lam32!r} is not float32({lam})")
    figs, exact = R.factor_layer(st, c.t, c.cumrot, d["Phi"], d["r_pred"], d["qgrad"], d["Hq"], hop)
    g, e2 = R.assembly_layer(d["bands"], d["rhs"], d["hess"], lam32, d["H"], d["b"], sigma, d["Phi"], d["r_pred"], d["qgrad"], d["Hq"],
                             False, prior, st)
    figs.update(g)
    pr = R.prior_ld(st, prior)[0] if reg else None
    pden = R.prior_ld(st, prior, absolute=True)[0] if reg else None
    ref, den = R.residual_sums_ld(c.uv, d["est"], None, d["r_pred"], sigma, c.n, False, pr, prior_den=pden)
    figs["sum_init"] = R.sums_figure(d["scalars"][2], ref, den)
    v = R.judge(lv, figs, exact + e2)
    _note(path, v, lv)
    print(f"FIGURES {where}: " + " ".join(f"{k}={v.units[k]:.2f}/{lv.units[k]:.2f}" for k in v.units))
    return bad + [f"{where}: {f}" for f in v.failures]


def report(path, bad):
    rows = {k[1]: v for k, v in FIGURES.items() if k[0] == path}
    if rows:
        print(f"\nLARGEST {path}: " + "  ".join(f"{q} {v[0]:.2f} ({v[1]:.2f}) at {v[2]}" for q, v in rows.items()))
    assert not bad, "\n".join(bad[:40])


# ------------------------------------------------------------------------------------------------ the dynamics factor
GROUPS = {
    "blocks-of-4": [(n, "mixed") for n in C.POSES_4],
    "blocks-of-16-32": [(n, "mixed") for n in C.POSES_32],
    "pair-blocks": [(n, "mixed") for n in C.POSES_128],
    "init-step-blocks": [(n, "mixed") for n in C.POSES_256],
    "64-beside-1": [(n, "steps64") for n in C.STEPS64_POSES],
    "long-edge": [nk for nk in C.factor_cases() if nk[1].startswith("long")],
}
_SUMS = {}                      # (case, path) -> bits of the initial mean


def run_factor(c, path):
    hop = path == "hop"
    e = engine(c.n, c.m, mode=0 if path == "bandwidth" else 1, hop=hop)
    upload(e, c)
    if path == "profiled":
        e.step_profiled(C.IT, False)
    else:
        e.step(C.IT, False)
    d = fetch(e)
    e.close()
    return d


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("path", ["latency", "profiled", "bandwidth", "hop"])
def test_factor(path, group):
    bad = []
    for n, kind in GROUPS[group]:
        c = C.case(n, kind)
        hop = path == "hop"
        d = run_factor(c, path)
        bad += check_full(c, d, levels(c, hop=hop), path, f"{c.name} {path} w=0", hop=hop)
        _SUMS[(c.name, path)] = float(d["scalars"][2])
        if kind.startswith("long") and not hop:
            # the long edge is k_long_factor's: its slots are not zero, and its neighbours answered to the bars above
            k = int(kind[4:])
            if not (np.abs(d["Phi"][k]).max() > 0 and np.abs(d["r_pred"][k, :6]).max() > 0):
                bad.append(f"{c.name} {path}: the long edge {k} has no factor")
    report(path, bad)


@pytest.mark.parametrize("group", list(GROUPS))
def test_dynamics_forms_leave_the_bits_of_one_sum(group):
    """dynamics_block in the accumulation's grid, k_dynamics as its own launch and k_dynamics_pair promise the same block partials of
    |r_pred| at the input states: the initial mean of a call carries the same bits on all three paths.  (The trial mean does not
    have to: it follows the step, and the two kernel sets solve by different partitions.)"""
    bad = []
    for n, kind in GROUPS[group]:
        c = C.case(n, kind)
        got = {}
        for path in ("latency", "profiled", "bandwidth"):
            if (c.name, path) not in _SUMS:
                d = run_factor(c, path)
                _SUMS[(c.name, path)] = float(d["scalars"][2])
            got[path] = _SUMS[(c.name, path)]
        for path in ("profiled", "bandwidth"):
            if got[path] != got["latency"]:
                bad.append(f"{c.name}: initial mean {got[path]!r} on the {path} path, {got['latency']!r} in latency mode")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ the assembly
ASM_CASES = [(n, "mixed") for n in (2, 3, 4, 5, 9, 16, 17, 33, 65)] + [(129, "steps64"), (65, "long31")]


@pytest.mark.parametrize("reg", [False, True], ids=["BA", "BA_reg"])
@pytest.mark.parametrize("mask", [1, 9], ids=["per-entry", "uniform-pass"])
@pytest.mark.parametrize("mode", [1, 0], ids=["4-poses", "16-poses"])
def test_assembly(mode, mask, reg):
    path = f"assembly {'4' if mode else '16'} {'rows' if mask & 8 else 'entry'}{' reg' if reg else ''}"
    bad = []
    for n, kind in ASM_CASES:
        c = C.case(n, kind)
        e = engine(c.n, c.m, mode=mode, fusion=mask)
        upload(e, c, reg=reg)
        if reg:
            e.set_prior(True)
        e.step(C.IT, False)
        d = fetch(e)
        e.close()
        bad += check_full(c, d, levels(c, reg=reg), path, f"{c.name} {path} w=0", reg=reg)
    report(path, bad)


# ------------------------------------------------------------------------------------------------ the landmark-only phase
@pytest.mark.parametrize("mode,mask", [(1, 14), (0, None)], ids=["k_assemble-FUSE-4", "k_init_step"])
@pytest.mark.parametrize("group", ["blocks-of-4", "blocks-of-16-32", "pair-blocks", "init-step-blocks"])
def test_landmark_only(group, mode, mask):
    path = "landmark-only " + ("FUSE 4" if mode else "k_init_step")
    bad = []
    for n, kind in GROUPS[group]:
        c = C.case(n, kind)
        lv = levels(c, it=C.IT_INIT, lam=C.LAM_INIT, init=True)
        e = engine(c.n, c.m, mode=mode, fusion=mask)
        upload(e, c, lam=C.LAM_INIT)
        before = e.solver_fallbacks()
        e.step(C.IT_INIT, True)
        d = fetch(e)
        fell = e.solver_fallbacks() != before
        e.close()
        where = f"{c.name} {path} w=0"
        if d["flags"] != 0 or d["ntr"] != 1 or fell:
            bad.append(f"{where}: flags {d['flags']}, {d['ntr']} trials, fallback {fell}: not the fused first trial")
        lam32 = d["scalars"][4]
        if lam32 != float(np.float32(C.LAM_INIT)):
            bad.append(f"{where}: damping {lam32!r} is not float32({C.LAM_INIT})")
        figs, exact = R.step_layer(d["dpose"], d["out"], d["H"], d["b"], lam32, c.states)
        z = np.zeros
        g, e2 = R.assembly_layer(d["bands"], d["rhs"], d["hess"], lam32, d["H"], d["b"], 0.0, z((c.n, 6, 6)), z((c.n - 1, 7)), z((c.n, 3)),
                                 z((c.n, 3, 3, 3)), True)
        figs.update(g)
        if np.any(d["bands"][:, 0] != 0) or np.any(d["bands"][:, 2] != 0):
            bad.append(f"{where}: an off-diagonal block of a landmark-only call is not zero")
        ref, den = R.residual_sums_ld(c.uv, d["est"], None, None, 0.0, c.n, True)
        figs["sum_init"] = R.sums_figure(d["scalars"][2], ref, den)
        v = R.judge(lv, figs, exact + e2)
        _note(path, v, lv)
        print(f"FIGURES {where}: " + " ".join(f"{k}={v.units[k]:.2f}/{lv.units[k]:.2f}" for k in v.units))
        bad += [f"{where}: {f}" for f in v.failures]
    report(path, bad)


# ------------------------------------------------------------------------------------------------ the residual sums
SUM_CASES = [(5, "mixed"), (33, "long31"), (34, "long32"), (129, "long31"), (257, "mixed")]


def check_trial_mean(c, d1, d2, lv, path, where, reg):
    """The trial mean of the first call (``d1``) against the rows and the factor the second call (``d2``) reports at the trial
    states, with the first call's weights (est comes from the fetch's projection kernel, the sum from the trial kernel: the rows'
    denominator is |uv| + |est|)."""
    prior = c.prior() if reg else None
    st2 = d1["out"]
    pr = R.prior_ld(st2, prior)[0] if reg else None
    pden = R.prior_ld(st2, prior, absolute=True)[0] if reg else None
    ref, den = R.residual_sums_ld(c.uv, d2["est"], d1["weight"], d2["r_pred"], d1["scalars"][5], c.n, False, pr, trial=True, prior_den=pden)
    v = R.judge(lv, {"sum_trial": R.sums_figure(d1["scalars"][3], ref, den)}, bars={"sum_trial": "sum_init"})
    _note(path, v, lv)
    print(f"FIGURES {where}: sum_trial={v.units['sum_trial']:.2f}")
    return [f"{where}: {f}" for f in v.failures]


@pytest.mark.parametrize("reg", [False, True], ids=["BA", "BA_reg"])
@pytest.mark.parametrize("mode", [1, 0], ids=["latency", "bandwidth"])
def test_residual_sums(mode, reg):
    path = f"sums {'latency' if mode else 'bandwidth'}{' reg' if reg else ''}"
    bad = []
    for n, kind in SUM_CASES:
        c = C.case(n, kind)
        e = engine(c.n, c.m, mode=mode)
        upload(e, c, reg=reg)
        if reg:
            e.set_prior(True)
        e.step(C.IT, False)
        d1 = fetch(e)
        e.step(C.IT, False)             # from the trial states the first call left, the other parity of the block partials
        d2 = fetch(e)
        e.close()
        lv = levels(c, reg=reg)
        bad += check_full(c, d1, lv, path, f"{c.name} {path} w=0 call 1", reg=reg)
        lv2 = levels(c, reg=reg, states=d1["out"], lam=d1["lam"], tag=f"behind {path}", accept=False)
        bad += check_full(c, d2, lv2, path, f"{c.name} {path} w=0 call 2", reg=reg, states=d1["out"], lam=d1["lam"], one_trial=False)
        bad += check_trial_mean(c, d1, d2, lv, path, f"{c.name} {path} w=0 trial of call 1", reg)
    report(path, bad)


# ------------------------------------------------------------------------------------------------ the ragged batch
@pytest.mark.parametrize("reg", [False, True], ids=["BA", "BA_reg"])
@pytest.mark.parametrize("mode", [1, 0], ids=["latency", "bandwidth"])
def test_ragged_batch(mode, reg):
    path = f"ragged {'latency' if mode else 'bandwidth'}{' reg' if reg else ''}"
    wins = C.ragged()
    e = engine(max(c.n for c in wins), max(c.m for c in wins), windows=len(wins), mode=mode)
    if mode == 0:
        e.set_solver(-2)                # one window per wavefront on both handles: the default partition follows n_max
    for k, c in enumerate(wins):
        upload(e, c, k, reg=reg)
    if reg:
        e.set_prior(True)
    e.step(C.IT, False)
    together = [fetch(e, k) for k in range(len(wins))]
    e.close()
    bad = []
    for k, c in enumerate(wins):
        bad += check_full(c, together[k], levels(c, reg=reg), path, f"{c.name} {path} w={k}", reg=reg)
        e = engine(c.n, c.m, windows=1, mode=mode)
        if mode == 0:
            e.set_solver(-2)
        upload(e, c, reg=reg)
        if reg:
            e.set_prior(True)
        e.step(C.IT, False)
        alone = fetch(e)
        e.close()
        for q in ("Phi", "r_pred", "qgrad", "Hq", "H", "b", "bands", "rhs", "dpose", "out", "hess"):
            a, b = together[k][q], alone[q]
            if q == "Phi":
                a, b = a[:-1], b[:-1]           # (the last pose has no edge: its slot is not written)
            if not np.array_equal(a, b):
                i = int(np.argmax((a != b).reshape(a.shape[0], -1).any(1))) if a.ndim > 1 and a.shape[0] == b.shape[0] else -1
                bad.append(f"{c.name} {path} w={k}: {q} differs from the window alone, first at pose {i}")
        # (the initial mean; the trial mean is summed over block partials whose count follows n_max: the trial kernel's business)
        if together[k]["scalars"][2] != alone["scalars"][2]:
            bad.append(f"{c.name} {path} w={k}: the initial mean {together[k]['scalars'][2]!r} differs from the window alone {alone['scalars'][2]!r}")
    report(path, bad)
