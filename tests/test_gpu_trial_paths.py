"""Every form of the trial kernel (``k_trial``, vinsat_amd/csrc/vba_trial.hip) by what it leaves behind: the trial states it forms, the
block sums of the accept test slot by slot, the trial mean, and the next call's keys, histogram and bin buckets.

One ``vba_step`` per case and form whose first trial is accepted with flags 0, then ``vba_debug_fetch`` (``VBA_DBG_PART_TRIAL``,
``VBA_DBG_NEXT_*``, ``VBA_DBG_PART_NEXT`` beside the older selectors), then a second call at those states for ``VBA_DBG_EST`` there.
tests/trial_cases.py has the windows (the seams of 15 edges and of 256 edges per pose-chain block, 256 leading rows in one
observation block, poses without rows, tiles that begin inside a pose, 1 .. 9 tiles, a long edge, BA_reg), tests/trial_reference.py
the longdouble slot sums and the restated bin functions, tests/test_trial_reference_host.py the oracle's figures, the conditions on
the cases and the planted faults.  A sum or a state passes at K x 2^-53, K = max(16, 4 x the fp64 NumPy oracle's figure on the same
case and quantity); keys, histogram, buckets and the TILES comparison have no tolerance.  No case is left out of any check.

Where each test lands (``launch_trial_emit``; E = EMIT: 2 default, 1 ``set_warm_select(False)``, 0 ``set_key_carry(False)``):

  test_form[F1-E2 / E1 / E0]     latency mode, default mask, landmark-only call: k_trial<E, 1> (6x6 solve per pose, retraction, last_hessian)
  test_form[F2-E2 / E1 / E0]     ... full-phase call: k_trial<E, 2> (recovery of the partitioned solve; the 2-pose handle has no
                                 partition and lands in k_trial<E, 3>: the fetch says so and the test expects it)
  test_form[F3p-E2 / E1 / E0]    ... ``set_pivoting(True)``, landmark-only call: k_trial<E, 3> (16-lane geometry, states from memory)
  test_form[F3s-E2]              ... ``set_solver(0)``, full-phase call: k_trial<2, 3> behind the sequential solver
  test_form[F0-E2 / E1 / E0]     latency mode, fusion mask 14 (bit 0 off), full-phase call: k_trial<E, 0> (plain geometry, one grid)
  test_form[F0i-E2]              ... landmark-only call (the step is k_assemble<true>'s)
  test_form[T2 / T4 / T8]        ... ``set_trial_tiles``: k_trial<2, 0, 0, 2 / 4 / 8>
  test_form[P-E2 / E1 / E0]      bandwidth mode, full-phase call: k_trial<E, 0, 2> and k_trial<E, 0, 1> as two launches
  test_form[Pi-E2]               ... landmark-only call
  test_tiles_leave_the_same_bits TILES 1 / 2 / 4 / 8 on every window: states, scalars, keys, histogram, part_trial, part_next bit for bit,
                                 buckets as multisets per bin
  test_small_buckets             ``set_bucket_cap(8)`` on F1 and T4: full bins hold a sub-multiset, the histogram the full count
  test_ragged_batch              46, 2, 32 (1025 rows) and 17 poses on one handle (n_max 46, m_max 1025), F2 / F1 / bandwidth: every
                                 window by the same bars; states, step, keys, histogram, part_next and the observation slots bit-equal to
                                 the window alone.  The pose-chain slots follow the handle: the 16-lane geometry gives the last pose's
                                 prior term to block min(j / 15, nblk_dyn - 1) and the plain one has ceil(n_max / 256) slots, so they
                                 (and the mean summed over them) are judged by the bars only.

Not reached: k_trial<E, 1> on a window that has fallen back to the pivoted kernels (flag 16).  Such a call never ends with one trial
and flags 0 -- the fallback is a repeat -- and no window of the suite's landmark-only cases trips the 6x6 pivot check;
tests/test_gpu_solve_paths.py::test_packed_walk_pivoted_fallback reaches a fallback of the full-phase packed walk only.

Measured on the MI355X: the largest figure per form and quantity over all cases in units of 2^-53, in brackets the oracle's figure on
the case that gave it (the bar is max(16, 4 x the bracket): 16, and 16.04 for the retraction of mixed[30]); docs/NOTEBOOK.md has the same table.

  form                  retract       step_fwd      last_hessian  part_obs      part_next     part_dyn      part_long     mean
  F1-E2                 3.98 (3.49)   1.38 (2.07)   1.96 (0.00)   2.30 (1.60)   1.50 (1.50)   0.00 (0.00)   -             1.49 (0.22)
  F2-E2                 3.92 (2.91)   -             -             1.89 (0.99)   1.77 (0.82)   1.74 (0.45)   0.93 (0.97)   0.40 (0.29)
  F3p-E2                4.28 (3.62)   -             1.96 (0.00)   2.09 (0.84)   1.75 (1.50)   0.00 (0.00)   -             2.22 (0.07)
  F0-E2                 3.92 (2.91)   -             -             1.89 (0.99)   1.77 (0.82)   2.96 (0.86)   0.93 (0.97)   0.40 (0.29)
  P-E2                  3.98 (3.32)   -             -             1.48 (0.43)   2.04 (1.30)   0.51 (0.86)   1.70 (0.97)   0.40 (0.29)
  F1-E1                 3.98 (3.49)   1.38 (2.07)   1.96 (0.00)   2.30 (1.60)   1.50 (1.50)   0.00 (0.00)   -             1.49 (0.22)
  F2-E1                 3.92 (2.91)   -             -             1.89 (0.99)   1.77 (0.82)   1.74 (0.45)   0.93 (0.97)   0.40 (0.29)
  F3p-E1                4.28 (3.62)   -             1.96 (0.00)   2.09 (0.84)   1.75 (1.50)   0.00 (0.00)   -             2.22 (0.07)
  F0-E1                 3.92 (2.91)   -             -             1.89 (0.99)   1.77 (0.82)   2.96 (0.86)   0.93 (0.97)   0.40 (0.29)
  P-E1                  3.98 (3.32)   -             -             1.48 (0.43)   2.04 (1.30)   0.51 (0.86)   1.70 (0.97)   0.40 (0.29)
  F1-E0                 3.98 (3.49)   1.38 (2.07)   1.96 (0.00)   2.30 (1.60)   -             0.00 (0.00)   -             1.49 (0.22)
  F2-E0                 3.92 (2.91)   -             -             1.89 (0.99)   -             1.74 (0.45)   0.93 (0.97)   0.40 (0.29)
  F3p-E0                4.28 (3.62)   -             1.96 (0.00)   2.09 (0.84)   -             0.00 (0.00)   -             2.22 (0.07)
  F0-E0                 3.92 (2.91)   -             -             1.89 (0.99)   -             2.96 (0.86)   0.93 (0.97)   0.40 (0.29)
  P-E0                  3.98 (3.32)   -             -             1.48 (0.43)   -             0.51 (0.86)   1.70 (0.97)   0.40 (0.29)
  F3s-E2                4.30 (3.32)   -             -             1.91 (2.03)   1.69 (1.26)   1.28 (0.50)   0.15 (0.97)   0.40 (0.29)
  F0i-E2                3.98 (3.49)   -             1.96 (0.00)   2.30 (1.60)   1.50 (1.50)   0.00 (0.00)   -             1.49 (0.22)
  Pi-E2                 3.64 (3.67)   -             1.96 (0.00)   1.87 (1.16)   1.40 (1.27)   0.00 (0.00)   -             1.97 (0.04)
  T2                    3.92 (2.91)   -             -             1.89 (0.99)   1.77 (0.82)   2.96 (0.86)   0.93 (0.97)   0.40 (0.29)
  T4                    3.92 (2.91)   -             -             1.89 (0.99)   1.77 (0.82)   2.96 (0.86)   0.93 (0.97)   0.40 (0.29)
  T8                    3.92 (2.91)   -             -             1.89 (0.99)   1.77 (0.82)   2.96 (0.86)   0.93 (0.97)   0.40 (0.29)
  F1-E2 cap 8           3.27 (3.06)   1.12 (0.62)   1.94 (0.51)   2.30 (1.60)   1.46 (1.42)   0.00 (0.00)   -             0.82 (0.74)
  T4 cap 8              3.14 (2.53)   -             -             1.53 (0.56)   1.77 (0.82)   0.15 (0.01)   -             0.15 (0.01)
  ragged F2-E2          2.79 (3.00)   -             -             1.53 (0.56)   1.10 (0.67)   0.97 (0.65)   -             0.40 (0.29)
  ragged F1-E2          2.95 (2.86)   0.72 (0.74)   1.40 (0.36)   0.99 (0.79)   1.50 (1.50)   0.00 (0.00)   -             1.49 (0.22)
  ragged P-E2           3.63 (2.38)   -             -             1.91 (2.03)   1.67 (0.67)   0.40 (0.29)   -             0.40 (0.29)
  ragged F2-E2 reg      2.97 (2.56)   -             -             1.03 (0.21)   1.43 (1.34)   0.43 (0.50)   -             0.16 (0.27)
  ragged F1-E2 reg      2.95 (2.86)   0.72 (0.74)   1.40 (0.36)   0.99 (0.79)   1.50 (1.50)   0.00 (0.00)   -             0.97 (0.37)
  ragged P-E2 reg       3.80 (2.56)   -             -             1.45 (1.00)   1.21 (1.33)   0.32 (0.02)   -             0.32 (0.02)

Nothing comes near a bar and no kernel changed.  Keys, histograms and buckets were exact in every form and on every case; TILES 2 / 4 / 8
left the bits of TILES 1; an EMIT 1 / EMIT 0 form left the sums and states of its EMIT 2 twin (the rows above repeat).
"""
import numpy as np
import pytest

import dynamics_reference as R
import trial_cases as C
import trial_reference as T

pytestmark = pytest.mark.gpu

# name -> mode, fusion mask, landmark-only, pivoting, solver, tiles, key carry, warm select | what the fetch must report: FUSED, EMIT, split
FORMS = {}


def _form(name, mode=1, fusion=None, init=False, pivot=False, solver=None, tiles=None, carry=True, warm=True, fused=0, split=0):
    FORMS[name] = dict(mode=mode, fusion=fusion, init=init, pivot=pivot, solver=solver, tiles=tiles, carry=carry, warm=warm,
                       fused=fused, emit=0 if not carry else (2 if warm else 1), split=split, lanes16=fused != 0)


for _e, _kw in (("E2", {}), ("E1", dict(warm=False)), ("E0", dict(carry=False))):
    _form(f"F1-{_e}", init=True, fused=1, **_kw)
    _form(f"F2-{_e}", fused=2, **_kw)
    _form(f"F3p-{_e}", init=True, pivot=True, fused=3, **_kw)
    _form(f"F0-{_e}", fusion=14, **_kw)
    _form(f"P-{_e}", mode=0, split=1, **_kw)
_form("F3s-E2", solver=0, fused=3)
_form("F0i-E2", fusion=14, init=True)
_form("Pi-E2", mode=0, split=1, init=True)
for _t in (2, 4, 8):
    _form(f"T{_t}", fusion=14, tiles=_t)
FORMS["F0-E2"]["tiles"] = 1

_LEVELS = {}
_RUNS = {}
FIGURES = {}


def levels(s, init, lanes16):
    key = (s.name, s.n_max, s.m_max, init, lanes16)
    if key not in _LEVELS:
        _LEVELS[key] = T.oracle_levels(s.case, C.IT_INIT if init else C.IT, C.LAM_INIT if init else C.LAM, init, s.n_max, s.m_max, lanes16,
                                       reg=s.reg)
    return _LEVELS[key]


def engine(n_max, m_max, f, windows=1, cap=None):
    from vinsat_amd.engine import BAEngine
    e = BAEngine(n_max, m_max, windows=windows, mode=f["mode"])
    if f["fusion"] is not None:
        e.set_fusion(f["fusion"])
    if f["pivot"]:
        e.set_pivoting(True)
    if f["solver"] is not None:
        e.set_solver(f["solver"])
    if f["tiles"] is not None:
        e.set_trial_tiles(f["tiles"])
    if not f["carry"]:
        e.set_key_carry(False)
    if not f["warm"]:
        e.set_warm_select(False)
    if cap is not None:
        e.set_bucket_cap(cap)
    return e


def upload(e, c, reg, lam, k=0):
    e.upload_observations(c.xyz, c.uv, c.conf, c.ii, c.n, window=k)
    e.upload_window(c.K, c.cumrot, c.t, window=k)
    if reg:
        e.upload_prior(*c.prior(), window=k)
    e.set_states(c.states, lam, window=k)


def fetch(e, f, k=0):
    d = {w: e.debug(w, window=k) for w in ("scalars", "dpose", "weight", "H", "b")}
    d["out"], d["lam"], d["hess"], d["ntr"], d["flags"] = e.get_states(window=k)
    d["geo"] = e.debug_trial(window=k)
    d["chunk"] = e.mode()[1]
    d["next"] = e.debug_next(window=k) if f["emit"] else None
    return d


def run(s, name, cap=None):
    """One call of form ``name`` on window ``s`` (a handle of its own), everything fetched, and est at the trial states from a second call."""
    key = (s.name, name, cap)
    if key not in _RUNS:
        f = FORMS[name]
        it, lam = (C.IT_INIT, C.LAM_INIT) if f["init"] else (C.IT, C.LAM)
        e = engine(s.n_max, s.m_max, f, cap=cap)
        upload(e, s.case, s.reg, lam)
        if s.reg:
            e.set_prior(True)
        e.step(it, f["init"])
        d = fetch(e, f)
        e.step(it, f["init"])
        d["est2"] = e.debug("est")
        e.close()
        _RUNS[key] = d
    return _RUNS[key]


def _note(path, v, lv):
    for k in v.units:
        cur = FIGURES.setdefault((path, k), [0.0, 0.0, None])
        if v.units[k] >= cur[0]:
            FIGURES[(path, k)] = [v.units[k], lv.units.get(k, float("nan")), v.where[k]]


def check(s, c, d, f, lv, path, where, n_max=None, m_max=None, cap=None):
    """Every check of one window: [] or what is wrong, each line with case, form, window."""
    n_max, m_max = s.n_max if n_max is None else n_max, s.m_max if m_max is None else m_max
    init, reg = f["init"], s.reg
    bad, exact, figs = [], [], {}
    if d["flags"] != 0 or d["ntr"] != 1:
        bad.append(f"{where}: flags {d['flags']}, {d['ntr']} trials (the case asks for one accepted trial)")
    geo = d["geo"]
    no, nd = T.geometry(n_max, m_max, f["lanes16"])
    sigma, lam32 = d["scalars"][5], d["scalars"][4]
    prior = c.prior() if (reg and not init) else None
    ch = T.chain_terms(d["out"], c.t, c.cumrot, sigma, init, False, prior)
    nl = 0 if init else int(geo["nblk_long"])
    # (a handle too short for the partitioned solve walks its chain: its full-phase calls read the trial states from memory)
    fused = 3 if (f["fused"] == 2 and d["chunk"] <= 0) else f["fused"]
    want = dict(nblk_obs=no, nblk_dyn=nd, fused=fused, emit=f["emit"], split=f["split"])
    if f["tiles"] is not None:
        want["tiles"] = f["tiles"]
    for k, v in want.items():
        if geo[k] != v:
            bad.append(f"{where}: the fetch reports {k} = {geo[k]}, this form is {v}: another kernel ran")
    if nl < int(ch["long"].sum()):
        bad.append(f"{where}: {int(ch['long'].sum())} long edges, {nl} slots")
    # states
    figs["retract"] = T.retract_figure(c.states, d["dpose"], d["out"], exact)
    if f["fused"] == 1:
        g, e2 = R.step_layer(d["dpose"], d["out"], d["H"], d["b"], lam32, c.states)
        figs["step_fwd"] = g["step_fwd"]
        exact += e2
    if init:
        figs["last_hessian"] = T.hessian_figure(d["hess"], d["H"][-1], lam32, exact)
    # sums
    ref = T.slot_sums(c.uv, d["est2"], d["weight"], c.ii, ch, n_max, m_max, f["lanes16"], nl)
    figs.update(T.slot_figures(ref, geo["part_trial"], d["next"]["part_next"] if d["next"] else None, nl, exact))
    mean, den = T.trial_mean(ref, c.n, c.m, init, reg)
    figs["mean"] = R.sums_figure(d["scalars"][3], mean, den)
    if not d["scalars"][3] < d["scalars"][2]:
        bad.append(f"{where}: the trial mean {d['scalars'][3]!r} is not below the initial mean {d['scalars'][2]!r}")
    # what is carried
    if d["next"]:
        nx = d["next"]
        bad += [f"{where}: {x}" for x in T.check_keys(nx["keys"], c.uv, d["est2"])]
        if nx["kind"] != f["emit"]:
            bad.append(f"{where}: histogram of kind {nx['kind']}, EMIT {f['emit']}")
        bad += [f"{where}: {x}" for x in T.check_hist(nx["keys"], nx["kind"], nx["warm_lo"], nx["shift"], nx["hist"], d["scalars"][0],
                                                       nx["sel_rank"])]
        if ("buckets" in nx) != (f["emit"] == 2 and f["mode"] == 1):
            bad.append(f"{where}: bin buckets {'fetched' if 'buckets' in nx else 'missing'}")
        if "buckets" in nx:
            if cap is not None and nx["cap"] != cap:
                bad.append(f"{where}: bucket cap {nx['cap']}, set to {cap}")
            bad += [f"{where}: {x}" for x in T.check_buckets(nx["keys"], nx["warm_lo"], nx["shift"], nx["hist"], nx["buckets"], nx["cap"])]
    v = R.judge(lv, figs, exact)
    _note(path, v, lv)
    print(f"FIGURES {where}: " + " ".join(f"{k}={v.units[k]:.2f}/{lv.units.get(k, float('nan')):.2f}" for k in v.units))
    return bad + [f"{where}: {x}" for x in v.failures]


def report(path, bad):
    rows = {k[1]: v for k, v in FIGURES.items() if k[0] == path}
    if rows:
        print(f"\nLARGEST {path}: " + "  ".join(f"{q} {v[0]:.2f} ({v[1]:.2f}) at {v[2]}" for q, v in rows.items()))
    assert not bad, "\n".join(bad[:40])


# ------------------------------------------------------------------------------------------------ form by form
@pytest.mark.parametrize("group", list(C.GROUPS))
@pytest.mark.parametrize("name", list(FORMS))
def test_form(name, group):
    f = FORMS[name]
    bad = []
    for s in C.group(group):
        d = run(s, name)
        bad += check(s, s.case, d, f, levels(s, f["init"], f["lanes16"]), name, f"{s.name} {name}")
    report(name, bad)


# ------------------------------------------------------------------------------------------------ TILES
BITS = ("out", "dpose", "scalars", "hess")


def same_bits(a, b, what, where, buckets=True):
    """[] or where two runs differ: states, scalars, keys, histogram, part_trial, part_next bit for bit, buckets as multisets per bin."""
    bad = [f"{where}: {q} differs from {what}" for q in BITS if not np.array_equal(a[q], b[q])]
    if not np.array_equal(a["geo"]["part_trial"], b["geo"]["part_trial"]):
        k = int(np.argmax(a["geo"]["part_trial"] != b["geo"]["part_trial"]))
        bad.append(f"{where}: part_trial slot {k} differs from {what}")
    for q in ("keys", "hist", "part_next", "warm_lo", "shift"):
        if not np.array_equal(a["next"][q], b["next"][q]):
            bad.append(f"{where}: {q} differs from {what}")
    if buckets:
        ha, ba, bb = a["next"]["hist"].astype(np.int64), a["next"]["buckets"], b["next"]["buckets"]
        cap = a["next"]["cap"]
        for bn in range(1, 2047):
            k = min(int(ha[bn]), cap)
            if k <= cap and int(ha[bn]) <= cap and not np.array_equal(np.sort(ba[bn, :k]), np.sort(bb[bn, :k])):
                bad.append(f"{where}: bucket {bn} holds another multiset than {what}")
    return bad


@pytest.mark.parametrize("group", list(C.GROUPS))
def test_tiles_leave_the_same_bits(group):
    bad = []
    for s in C.group(group):
        one = run(s, "F0-E2")
        for t in (2, 4, 8):
            bad += same_bits(run(s, f"T{t}"), one, "TILES 1", f"{s.name} TILES {t}")
    assert not bad, "\n".join(bad[:40])


# ------------------------------------------------------------------------------------------------ small buckets
@pytest.mark.parametrize("name", ["F1-E2", "T4"])
def test_small_buckets(name):
    f = FORMS[name]
    bad, full = [], 0
    for s in C.group("tiles"):
        d = run(s, name, cap=8)
        full += int((d["next"]["hist"][1:2047] > 8).sum())
        bad += check(s, s.case, d, f, levels(s, f["init"], f["lanes16"]), f"{name} cap 8", f"{s.name} {name} cap 8", cap=8)
    assert full > 0, "no bin holds more than 8 keys: the cases do not reach a full bucket"
    report(f"{name} cap 8", bad)


# ------------------------------------------------------------------------------------------------ the ragged batch
@pytest.mark.parametrize("name", ["F2-E2", "F1-E2", "P-E2"])
@pytest.mark.parametrize("reg", [False, True], ids=["BA", "BA_reg"])
def test_ragged_batch(reg, name):
    f = FORMS[name]
    wins, n_max, m_max = C.ragged()
    it, lam = (C.IT_INIT, C.LAM_INIT) if f["init"] else (C.IT, C.LAM)

    def go(cs, n_max, m_max, chunk=None):
        e = engine(n_max, m_max, f, windows=len(cs))
        if f["mode"] == 0:
            e.set_solver(-2)            # one window per wavefront on both handles: the default partition follows n_max
        elif chunk is not None and n_max >= 8:
            # ... and so does the chunk size of the latency-mode handles: the batch's on the window alone, with the cyclic reduction
            # of the default behind it (a handle of fewer than 8 poses walks its chain: the 2-pose window is one chunk either way)
            e.set_solver(chunk, -1)
        for k, c in enumerate(cs):
            upload(e, c, reg, lam, k)
        if reg:
            e.set_prior(True)
        e.step(it, f["init"])
        ds = [fetch(e, f, k) for k in range(len(cs))]
        e.step(it, f["init"])
        for k, d in enumerate(ds):
            d["est2"] = e.debug("est", window=k)
        e.close()
        return ds

    together = go(wins, n_max, m_max)
    path = f"ragged {name}{' reg' if reg else ''}"
    bad = []
    for k, c in enumerate(wins):
        s = C.Spec(c, n_max, m_max, reg)
        bad += check(s, c, together[k], f, levels(s, f["init"], f["lanes16"]), path, f"{c.name} {path} w={k}")
        alone = go([c], c.n, c.m, together[k]["chunk"] if not f["init"] else None)[0]
        where = f"{c.name} {path} w={k}"
        for q in ("out", "dpose", "hess"):
            if not np.array_equal(together[k][q], alone[q]):
                bad.append(f"{where}: {q} differs from the window alone")
        ta, tb = together[k]["next"], alone["next"]
        for q in ("keys", "hist", "warm_lo"):
            if not np.array_equal(ta[q], tb[q]):
                bad.append(f"{where}: {q} differs from the window alone")
        nt = -(-c.m // 256)
        if not np.array_equal(ta["part_next"][:nt], tb["part_next"][:nt]):
            bad.append(f"{where}: part_next differs from the window alone")
        if not np.array_equal(together[k]["geo"]["part_trial"][:nt], alone["geo"]["part_trial"][:nt]):
            bad.append(f"{where}: an observation slot of part_trial differs from the window alone")
    report(path, bad)
