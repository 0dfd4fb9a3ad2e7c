"""Windows whose row segments sit on the edges of the accumulation kernel's lane arithmetic (k_obs_accumulate,
vinsat_amd/csrc/vba_accumulate.hip), and windows with depth-clamped rows.  No GPU needed (the library's host code is: build first).

Every builder returns a ``Case``: the upload arrays (rows shuffled), the states the call is made at, the per-pose row counts.  Rows
come from ``synth.make_sequence`` / ``od_pipe.prepare_window``; a pose's rows are the first ``count`` of its own (repeated in turn
if it has fewer).

``edges(G, m_mod)``   70 poses (two blocks at 4 lanes per pose, the second partly filled; 18 blocks at 64), row counts cycling through
                      0, 1, 2, G-1, G, G+1, 2G-1, 2G, 2G+1, kAccDepth G - 1, kAccDepth G + 1, 4G+1, 201; the last pose gets an odd count
                      (its last pair straddles the window's last row); ``m % 32 == m_mod`` by lengthening one 201-row pose (0: the
                      padded row count equals m); at least one segment starts at an odd sorted index (asserted).
``clamped(G)``        the same layout with ~10 % of the rows moved to camera-frame depths -40, 0.05, 0.0999 (clamped) and 0.1001 km
                      (live) at the case's states, |x|, |y| <= 0.03 km, uv = the clamped projection + 2 px of noise; 5 % of all rows
                      of confidence 0; one pose with only such rows; one pose with only clamped rows.  At equal confidence a moved
                      row (f / 0.1 km in translation, 2 f 40 km / 0.1 km in rotation at -40 km) carries all of its pose's trace(H),
                      so the moved rows of a pose get the confidence that gives them a share of trace(H) cycling through 20 .. 80 %
                      at the case's call (weights of the longdouble reference) -- a median of 2e-4 of the others', 1e-6 for a pose
                      whose moved rows stand at -40 km up to ~1 for one with a single 0.05 km row among 200; asserted on the
                      reference: 10 .. 90 % in every pose with both kinds of row.
States: the window's truth plus a tenth of the driver's initial perturbation (10 km, 0.02 rad).  From the full perturbation the pose
chain of the first full-phase call drags the poses ~100 km, the rows planted 0.05 km in front of them fly off and the oracle
rejects all 8 trials of that call; from a tenth it accepts the first trial of every call of random_windows.SCHEDULE and 80 .. 170
rows stay clamped throughout (tests/test_accumulate_reference_host.py asserts the acceptance).
``walk()``            8 windows of 130, 129, 97, 65, 64, 33, 32 and 2 poses with ~3 rows per pose (the 97-pose one clamped-style),
                      cycled over 1024 windows of a handle with n_max = 130: at 8 / 16 lanes per pose launch_obs_accumulate then walks
                      groups = 4 groups of poses per block without any environment knob."""
from dataclasses import dataclass, field

import numpy as np

import accumulate_reference as A

ACC_DEPTH = 2                   # kAccDepth (VBA_ACC_DEPTH)
N_EDGES = 70
DEPTHS = (-40.0, 0.05, 0.0999, 0.1001)
IT = 12                         # the call the cases are made for: full phase, alpha = 1
CONF_MOVED = 1e-4
GUESS_SCALE = 0.1               # at the full initial guess (100 km, 0.2 rad) the oracle rejects every trial of call 10 of clamped(8)
_SRC = {}
_CASES = {}


@dataclass
class Case:
    name: str
    states: np.ndarray          # [n, 10]
    xyz: np.ndarray             # [m, 3] rows as uploaded (shuffled)
    uv: np.ndarray              # [m, 2]
    conf: np.ndarray            # [m]
    ii: np.ndarray              # [m] int64
    K: np.ndarray               # [n, 4]
    cumrot: np.ndarray          # [n, 4]
    t: np.ndarray               # [n] int64
    counts: np.ndarray          # [n] rows per pose
    moved: np.ndarray           # [m] bool: rows planted near the camera
    extras: dict = field(default_factory=dict)

    @property
    def n(self):
        return self.states.shape[0]

    @property
    def m(self):
        return self.ii.size

    def oracle_args(self):
        """The window arguments of ``oracle.ba_oracle.ba_iteration`` behind (it, states)."""
        return (self.cumrot, self.uv, self.xyz, self.ii, self.t, self.K, self.conf)


def _source(n, rows, seed):
    from vinsat_amd import od_pipe, quat, synth
    key = (n, rows, seed)
    if key not in _SRC:
        det, orb = synth.make_sequence(synth.WindowConfig(f"acc{n}", n, rows, 5), seed=seed)
        win = od_pipe.prepare_window(det, orb)
        assert win.time_idx.size == n, (n, win.time_idx.size)
        # states: the truth plus GUESS_SCALE of the perturbation of od_pipe.initial_guess (10 km, 0.02 rad, 1 % |v|)
        gt, g = np.concatenate([win.poses_gt, win.velocities], -1), od_pipe.initial_guess(win, seed=seed)
        st = gt + GUESS_SCALE * (g - gt)
        st[:, 3:7] = quat.qexp(quat.qlog(gt[:, 3:7]) + GUESS_SCALE * (quat.qlog(g[:, 3:7]) - quat.qlog(gt[:, 3:7])))
        _SRC[key] = (win, st)
    return _SRC[key]


def edge_counts(G, m_mod=None, n=N_EDGES):
    cyc = [0, 1, 2, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, ACC_DEPTH * G - 1, ACC_DEPTH * G + 1, 4 * G + 1, 201]
    cnt = np.array([cyc[i % len(cyc)] for i in range(n)], dtype=np.int64)
    cnt[-1] |= 1
    if m_mod is not None:
        long_ones = np.nonzero(cnt == 201)[0]
        cnt[long_ones[-1]] += (m_mod - int(cnt.sum())) % 32
        assert int(cnt.sum()) % 32 == m_mod
    return cnt


def _layout(name, win, states, counts, seed):
    """The first counts[i] rows of pose i (repeated in turn if the source has fewer), shuffled."""
    rng = np.random.default_rng(seed)
    take = []
    for i, c in enumerate(counts):
        own = np.nonzero(win.ii == i)[0]
        assert c == 0 or own.size > 0
        take.append(np.resize(own, int(c)) if c else own[:0])
    take = np.concatenate(take)
    take = take[rng.permutation(take.size)]
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    case = Case(name, states.copy(), win.landmarks_xyz[take].copy(), win.landmarks_uv[take].copy(),
                rng.uniform(0.3, 1.2, size=take.size), win.ii[take].astype(np.int64), win.intrinsics.copy(), win.cumrot_last.copy(),
                win.time_idx.astype(np.int64).copy(), np.asarray(counts, dtype=np.int64), np.zeros(take.size, dtype=bool))
    case.extras["odd_starts"] = int(np.count_nonzero((starts % 2 == 1) & (np.asarray(counts) > 0)))
    return case


def edges(G, m_mod=None):
    key = ("edges", G, m_mod)
    if key not in _CASES:
        win, st0 = _source(N_EDGES, 240, 7)
        counts = edge_counts(G, m_mod)
        case = _layout(f"edges({G}, m%32={m_mod})", win, st0, counts, 100 + G)
        assert case.extras["odd_starts"] > 0 and counts[-1] % 2 == 1 and case.n == N_EDGES
        assert m_mod is None or case.m % 32 == m_mod
        _CASES[key] = case
    return _CASES[key]


def trace_shares(case, it=IT):
    """Per pose the share of trace(H) that the moved rows carry, from the longdouble reference at the case's states (NaN for a pose
    without rows of non-zero weight)."""
    rows = A.rows_ld(case.states, case.xyz, case.K, case.ii)
    est = rows.est.astype(np.float64)
    r = case.uv - est
    a = np.abs(r).reshape(-1)
    c = np.sort(a)[(a.size - 1) // 2]
    raw = A.weights_ld(r, np.ones(case.m), c, 1.0, it)
    tr = (raw * np.asarray(case.conf).astype(A.LD) * (rows.Jg ** 2).sum((1, 2))).astype(np.float64)
    tot = np.bincount(case.ii, weights=tr, minlength=case.n)
    mov = np.bincount(case.ii, weights=tr * case.moved, minlength=case.n)
    with np.errstate(invalid="ignore", divide="ignore"):
        return mov / tot


def plant_clamped(case, seed, it=IT, only_clamped=None, only_zero=None, fraction=0.10):
    """Moves ``fraction`` of the rows (and every row of pose ``only_clamped``) close to the camera, gives 5 % of the rows (and every
    row of pose ``only_zero``) confidence 0 and the moved rows of every pose the confidence that sets their share of trace(H)."""
    rng = np.random.default_rng(seed)
    m = case.m
    moved = rng.random(m) < fraction
    if only_zero is not None:
        moved[case.ii == only_zero] = False
    if only_clamped is not None:
        moved[case.ii == only_clamped] = True
    idx = np.nonzero(moved)[0]
    depth = np.array([DEPTHS[k % 4] for k in range(idx.size)])
    if only_clamped is not None:
        sel = case.ii[idx] == only_clamped
        depth[sel] = np.array([DEPTHS[k % 3] for k in range(int(sel.sum()))])
    pc = np.stack([rng.uniform(-0.03, 0.03, idx.size), rng.uniform(-0.03, 0.03, idx.size), depth], -1)
    Rm = A.rotation_ld(case.states[:, 3:7]).astype(np.float64)[case.ii[idx]]
    case.xyz[idx] = case.states[case.ii[idx], :3] + np.einsum("kij,kj->ki", Rm, pc)
    case.moved = moved
    rows = A.rows_ld(case.states, case.xyz, case.K, case.ii)
    z = rows.pc[idx, 2].astype(np.float64)
    assert np.abs(z - depth).max() < 1e-9, "a planted depth moved across the clamp when the point was rounded"
    case.uv[idx] = rows.est[idx].astype(np.float64) + rng.normal(0.0, 2.0, size=(idx.size, 2))
    case.extras["clamped"] = moved & ~rows.live
    case.extras["depth"] = np.full(m, np.nan)
    case.extras["depth"][idx] = depth
    # confidences: the moved rows of a pose share one value, set from the share of trace(H) it is to give them
    case.conf[moved] = CONF_MOVED
    zero = rng.random(m) < 0.05
    if only_clamped is not None:
        zero[case.ii == only_clamped] = False
    if only_zero is not None:
        zero[case.ii == only_zero] = True
    case.conf[zero] = 0.0
    shares = trace_shares(case, it)
    k = 0
    for i in range(case.n):
        s = shares[i]
        if np.isfinite(s) and 0.0 < s < 1.0:
            target = (0.2, 0.35, 0.5, 0.65, 0.8)[k % 5]
            k += 1
            case.conf[moved & (case.ii == i)] *= (target / (1 - target)) / (s / (1 - s))
    case.extras["conf_ratio"] = case.conf[moved & ~zero] / np.median(case.conf[~moved & ~zero])
    return case


def clamped(G, m_mod=None):
    key = ("clamped", G, m_mod)
    if key not in _CASES:
        win, st0 = _source(N_EDGES, 240, 7)
        counts = edge_counts(G, m_mod)
        case = _layout(f"clamped({G})" if m_mod is None else f"clamped({G}, m%32={m_mod})", win, st0, counts, 100 + G)
        only_zero, only_clamped = 4, 5              # G and G + 1 rows
        plant_clamped(case, 200 + G, only_clamped=only_clamped, only_zero=only_zero)
        case.extras.update(only_zero=only_zero, only_clamped=only_clamped)
        sh = trace_shares(case)
        live_w = np.bincount(case.ii, weights=(case.conf > 0) & ~case.moved, minlength=case.n) > 0
        mov_w = np.bincount(case.ii, weights=(case.conf > 0) & case.moved, minlength=case.n) > 0
        both = live_w & mov_w
        assert both.sum() >= 20 and np.all((sh[both] >= 0.1) & (sh[both] <= 0.9)), sh[both]
        assert np.all(case.conf[case.ii == only_zero] == 0.0) and np.all(case.extras["clamped"][case.ii == only_clamped])
        assert {float(d) for d in case.extras["depth"][case.moved]} == set(DEPTHS)
        _CASES[key] = case
    return _CASES[key]


WALK_POSES = (130, 129, 97, 65, 64, 33, 32, 2)
WALK_WINDOWS = 1024
WALK_N_MAX = 130


def walk():
    """The 8 distinct windows of the group walk (window w of the handle holds ``walk()[w % 8]``)."""
    if "walk" not in _CASES:
        out = []
        for k, n in enumerate(WALK_POSES):
            win, st0 = _source(n, 3, 300 + k)
            counts = np.bincount(win.ii, minlength=n)
            case = _layout(f"walk[{n}]", win, st0, counts, 400 + k)
            if n == 97:
                plant_clamped(case, 500, fraction=0.10)
            out.append(case)
        _CASES["walk"] = out
    return _CASES["walk"]


def walk_groups(lanes, W=WALK_WINDOWS, n_max=WALK_N_MAX):
    """What launch_obs_accumulate chooses for a batched handle: (groups of poses a block walks, blocks per window)."""
    nb = (n_max * lanes + 255) // 256
    groups = 4
    while groups > 1 and W * ((nb + groups - 1) // groups) < 2048:
        groups >>= 1
    return groups, (nb + groups - 1) // groups
