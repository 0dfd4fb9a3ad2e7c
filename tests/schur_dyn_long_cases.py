"""Problems and CPU references of the free-landmark mode with the dynamics factor ACROSS LONG GAPS (``SchurBA(..., long_gaps=True)``,
``vba_schur_enable_dynamics_long``, vinsat_amd/csrc/vba_schur_dyn_long.hip), shared by tests/test_schur_dyn_long_host.py and
tests/test_gpu_schur_dyn_long.py (plain module, no tests).  Built once per process; users leave them unchanged.

A problem is built as ``schur_dyn_cases.case`` builds: ``synth.make_tracked_landmarks`` at the case's own pose times, the position and
velocity columns of ``states_gt`` replaced by the EXACT chain of tests/exact_orbit.py from pose 0, then perturbed by 2 km, 2e-3 in
attitude, 2 m/s in velocity and 20 m on the landmarks.  ``SIGMA_DYN``, ``LAMS`` and ``BARS`` are those of tests/schur_dyn_cases.py.

  L12    12 / 150, one panel, gaps [1, 5, 65, 1, 64, 935, 1, 3, 510, 1, 2]: a 65 beside a 64 (the threshold), the gaps of the two-pass
         window (935 s, 510 s), a long edge that is the last before short ones
  L29    29 / 300, 9 n = 261 is two panels, gaps resize([5, 1, 66, 1, 5, 5, 1024, 5, 1, 129], 28): the saturation boundary of the plan
         (1024 s is the longest gap with L ~ sqrt(0.76 s) chunks), 129 s with four chunks
  factor-only windows of ``len(gaps) + 3`` poses, [5] + gaps + [4], with the gap tuples of
  ``test_gpu_long_gaps.test_gap_lengths_around_every_rule_of_the_partition``

Trial cases hold gaps <= 1024 s on purpose: there the parallel-in-time chain is within rounding of the serial walk, so the
bar of 1e-10 on ``c0`` is the oracle's to meet.

The exact-chain bar of a long edge is that of ``test_gpu_long_gaps._check_factor_exact``, measured on the MI355X for the same
``long_states``: device error <= EXACT_FACTOR x (error of ``O.propagate_orbit``) + EXACT_SLACK, per edge and component.
"""
import functools
from types import SimpleNamespace

import numpy as np

import exact_orbit as X
import schur_dyn_cases as C
import schur_dyn_oracle as D
from oracle import ba_oracle as O
from vinsat_amd import synth

SIGMA_DYN, LAMS, BARS = C.SIGMA_DYN, C.LAMS, C.BARS
LONG_GAP = 64                   # an edge of more steps is long (kSchurDynLongGap)
EXACT_SLACK = 2.0 ** -46
EXACT_FACTOR = 16.0
D6 = np.array([1.0, 1.0, 1.0, 100.0, 100.0, 100.0])

_GAPS = {
    "L12": np.array([1, 5, 65, 1, 64, 935, 1, 3, 510, 1, 2]),
    "L29": np.resize(np.array([5, 1, 66, 1, 5, 5, 1024, 5, 1, 129]), 28),
}
_LANDMARKS = {"L12": 150, "L29": 300}
NAMES = tuple(_GAPS)
FACTOR_GAPS = ((64, 65, 66), (100, 7, 1024, 3), (1025, 2, 2000), (3000,), (729, 730, 731))
FAULTS = ("reversed_product", "r_against_start", "no_long_cost")


def long_plan(s):
    """``long_plan`` of vinsat_amd/csrc/vba_math.h, restated: (L, P, sub, nsubL, G)."""
    L = 1
    while 45 * L * L < 34 * s:
        L += 1
    if 64 * L < s:
        L = (s + 63) // 64
    P = (s + L - 1) // L
    per_chunk = min(128 // P, 4)
    sub = max((L + per_chunk - 1) // per_chunk, 8)
    nsubL = (L + sub - 1) // sub
    last = s - (P - 1) * L
    return L, P, sub, nsubL, (P - 1) * nsubL + (last + sub - 1) // sub


def _build(gaps, n_landmarks, seed):
    gaps = np.asarray(gaps, dtype=np.int64)
    n = gaps.size + 1
    times = 10 + np.concatenate([[0], np.cumsum(gaps)])
    d = synth.make_tracked_landmarks(n_landmarks=n_landmarks, seed=seed, times=times)
    gt = d["states_gt"]
    x0 = np.concatenate([gt[0, :3], gt[0, 7:10]])
    xs = X.propagate(np.repeat(x0[None], n, 0), times - times[0], stm=False).astype(np.float64)
    gt = gt.copy()
    gt[:, :3], gt[:, 7:10] = xs[:, :3], xs[:, 3:]
    d["states_gt"] = gt
    rng = np.random.default_rng(seed + 100)
    st = gt.copy()
    st[:, :3] += rng.normal(0, 2.0, (n, 3))
    dq = np.concatenate([rng.normal(0, 2e-3, (n, 3)), np.ones((n, 1))], 1)
    st[:, 3:7] = O.qmul(st[:, 3:7], dq / np.linalg.norm(dq, axis=1, keepdims=True))
    st[:, 7:10] += rng.normal(0, 2e-3, (n, 3))
    d["states0"] = st
    d["w"] = np.full(d["uv"].shape[0], 0.95)
    d["Xs"] = d["X0"] + rng.normal(0, 0.02, d["X0"].shape)
    d["time_idx"] = times.astype(np.int32)
    d["sigma_dyn"] = SIGMA_DYN
    d["long"] = np.nonzero(gaps > LONG_GAP)[0]
    return d


@functools.lru_cache(maxsize=None)
def case(name, seed=1):
    return _build(_GAPS[name], _LANDMARKS[name], seed)


@functools.lru_cache(maxsize=None)
def factor_window(gaps, seed=1):
    """``len(gaps) + 3`` poses: a 5 s edge, the gaps, a 4 s edge (short edges beside the long ones keep their arithmetic)."""
    return _build([5] + list(gaps) + [4], 20 * (len(gaps) + 3), seed)


args, rel = C.args, C.rel


@functools.lru_cache(maxsize=None)
def exact_long_edges(key):
    """Per long edge of the problem (``key``: a case name or a tuple of gaps) at ``states0``: (edges, steps, exact x_hat and Phi in long
    double, the fp64 serial walk's errors against them as ``exact_orbit.edge_errors`` gives them)."""
    d = case(key) if isinstance(key, str) else factor_window(key)
    st, steps = d["states0"], np.diff(d["time_idx"]).astype(np.int64)
    e = d["long"]
    x = np.concatenate([st[:, :3], st[:, 7:]], -1)
    xe, Pe = X.propagate(x[e], steps[e])
    xo, Po = O.propagate_orbit(x[e], steps[e])
    return e, steps[e], xe, Pe, X.edge_errors(xo, Po, xe, Pe)


def _faulty_blocks(d, states, fault):
    """``schur_dyn_oracle.dynamics_blocks`` with a mistake planted in the LONG edges only."""
    t, sd = d["time_idx"], d["sigma_dyn"]
    n = states.shape[0]
    r, E, F = O.orbit_factor(states, np.asarray(t), jacobian=True)
    r, E = r.copy(), E.copy()
    steps = np.diff(t).astype(np.int64)
    x = np.concatenate([states[:, :3], states[:, 7:]], -1)
    for e in d["long"]:
        if fault == "reversed_product":         # Phi = Phi_2 Phi_1 of the two halves of the edge, multiplied the other way round
            h1 = int(steps[e]) // 2
            xm, P1 = O.propagate_orbit(x[e:e + 1], np.array([h1]))
            _, P2 = O.propagate_orbit(xm, np.array([int(steps[e]) - h1]))
            A = D6[:, None] * (P1[0] @ P2[0])
            E[e][:, 0:3], E[e][:, 6:9] = A[:, :3], A[:, 3:]
        if fault == "r_against_start":          # the residual against the edge's own start pose
            r[e] = r[e] + D6 * (x[e + 1] - x[e])
    idx = D.unknown_index(n)
    H, g = np.zeros((9 * n, 9 * n)), np.zeros(9 * n)
    for e in range(n - 1):
        a, b = idx[e], idx[e + 1]
        H[np.ix_(a, a)] += sd * E[e].T @ E[e]
        H[np.ix_(b, b)] += sd * F.T @ F
        Xb = sd * F.T @ E[e]
        H[np.ix_(b, a)] += Xb
        H[np.ix_(a, b)] += Xb.T
        g[a] -= sd * E[e].T @ r[e]
        g[b] -= sd * F.T @ r[e]
    return H, g


def _cost(d, states, Xl, fault=None):
    t, sd = d["time_idx"], d["sigma_dyn"]
    c = D.cost(states, Xl, *args(d), t, sd)
    if fault == "no_long_cost":
        r = O.orbit_factor(states, np.asarray(t), jacobian=False)
        c -= float(sd * (r[d["long"]] ** 2).sum())
    return c


@functools.lru_cache(maxsize=None)
def reference(name, lam, sigma_dyn=None, full=False, fault=None):
    """One LM trial of ``case(name)`` by the oracle's Schur route (``schur_dyn_cases.reference`` on these cases); ``fault``: one of
    FAULTS planted in the long edges."""
    d = dict(case(name))
    if sigma_dyn is not None:
        d["sigma_dyn"] = sigma_dyn
    sd = d["sigma_dyn"]
    st, Xs, t = d["states0"], d["Xs"], d["time_idx"]
    n = st.shape[0]
    r = SimpleNamespace()
    r.c0 = _cost(d, st, Xs, fault)
    ne = D.normal_equations(st, Xs, *args(d), lam, t, sd)
    if fault in ("reversed_product", "r_against_start"):
        B9, Cl, E9, v9, wl = ne
        H0, g0, _, _ = D.dynamics_blocks(st, t, sd)
        H1, g1 = _faulty_blocks(d, st, fault)
        ne = (B9 - H0 + H1, Cl, E9, v9 - g0 + g1, wl)
    dc9, dl, r.Sm, r.Lc = D.step_schur(*ne)
    s1, X1 = D.apply_step(st, Xs, dc9, dl)
    r.c1 = _cost(d, s1, X1, fault)
    r.ok = r.c1 < r.c0
    r.st, r.X = (s1, X1) if r.ok else (st, Xs)
    r.s1, r.X1 = s1, X1
    r.dc, r.dv, r.dl = dc9[:6 * n].reshape(n, 6), dc9[6 * n:].reshape(n, 3), dl.reshape(-1, 3)
    if full:
        f9, fl = D.step_full(*ne)
        r.floor = dict(dc=rel(dc9[:6 * n], f9[:6 * n]), dv=rel(dc9[6 * n:], f9[6 * n:]), dl=rel(dl, fl))
    return r


# ------------------------------------------------------------------------------------------------ downstream consumers on L12
@functools.lru_cache(maxsize=None)
def cov_reference(name, lam):
    """``schur_dyn_cov_cases.reference`` on a case of this module: the four families of the state covariance by the full inverse, the
    floor against the Schur route, the bar ``schur_dyn_cov_cases.bar`` reads."""
    import schur_dyn_cov_cases as V
    d = case(name)
    n = d["states0"].shape[0]
    s = V.structure(d)
    B9, Cm, E9, _, _ = D.normal_equations(d["states0"], d["Xs"], *args(d), lam, d["time_idx"], d["sigma_dyn"])
    n9 = B9.shape[0]
    bi, bj = s["blk_i"].astype(np.int64), s["blk_j"].astype(np.int64)
    Hinv = np.linalg.inv(np.block([[B9, E9], [E9.T, Cm]]))
    r = SimpleNamespace(blk_i=bi, blk_j=bj, lam=lam, n=n)
    for k, v in V.families(Hinv[:n9, :n9], V._diag_blocks(Hinv[n9:, n9:], 3), n, bi, bj).items():
        setattr(r, k, v)
    Cinv = np.linalg.inv(V._diag_blocks(Cm, 3))
    G = np.einsum("alc,lcd->ald", E9.reshape(n9, -1, 3), Cinv).reshape(n9, -1)
    S9 = B9 - G @ E9.T
    W = np.linalg.inv(np.linalg.cholesky(S9))
    Sinv = W.T @ W
    lm2 = Cinv + np.einsum("alc,ald->lcd", G.reshape(n9, -1, 3), (Sinv @ G).reshape(n9, -1, 3))
    r.floor = V.scaled(V.families(Sinv, lm2, n, bi, bj), r)
    return r


@functools.lru_cache(maxsize=None)
def att_case(name):
    """The case with the gap rotations of the truth and ``schur_att_cases.SIGMA_ATT`` (as ``schur_att_cases.case`` adds them)."""
    import schur_att_cases as AC
    import schur_att_oracle as A
    d = dict(case(name))
    q = d["states_gt"][:, 3:7]
    c = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (q.shape[0], 1))
    c[:-1] = O.qmul(A.conj(q[:-1]), q[1:])
    d["cumrot"], d["sigma_att"] = c, AC.SIGMA_ATT
    return d


@functools.lru_cache(maxsize=None)
def att_reference(name, lam, full=False):
    """``schur_att_cases.reference`` on a case of this module: one trial with the attitude factor on top."""
    import schur_att_oracle as A
    d = att_case(name)
    st, Xs = d["states0"], d["Xs"]
    f = (d["time_idx"], d["sigma_dyn"], d["cumrot"], d["sigma_att"])
    n = st.shape[0]
    r = SimpleNamespace()
    r.c0 = A.cost(st, Xs, *args(d), *f)
    ne = A.normal_equations(st, Xs, *args(d), lam, *f)
    dc9, dl, r.Sm, r.Lc = A.step_schur(*ne)
    s1, X1 = A.apply_step(st, Xs, dc9, dl)
    r.c1 = A.cost(s1, X1, *args(d), *f)
    r.ok = r.c1 < r.c0
    r.st, r.X = (s1, X1) if r.ok else (st, Xs)
    r.dc, r.dv, r.dl = dc9[:6 * n].reshape(n, 6), dc9[6 * n:].reshape(n, 3), dl.reshape(-1, 3)
    if full:
        f9, fl = A.step_full(*ne)
        r.floor = dict(dc=rel(dc9[:6 * n], f9[:6 * n]), dv=rel(dc9[6 * n:], f9[6 * n:]), dl=rel(dl, fl))
    return r
