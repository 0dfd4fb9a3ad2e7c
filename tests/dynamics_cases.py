"""Windows whose pose counts and gaps sit on the edges of the index arithmetic of the pose-chain kernels (vinsat_amd/csrc/vba_dyn.hip,
vba_dyn_body.h): 8 lanes per pose and 32 poses per block in ``dynamics_block``, two lanes per pose and 128 poses per block with four
virtual 32-pose partials in ``k_dynamics_pair``, 4 or 16 poses per block with a halo slot for pose i0 - 1 in the assembly kernels,
256 poses per block in ``k_init_step``.  No GPU needed (the library's host code is: build first).

A window is made the way ``synth.make_sequence`` makes one, with frames at times of the case's choosing: the orbit is the same 1 Hz
J2 trajectory, so the truth is consistent with the gaps and the dynamics residual at the case's states is that of a small
perturbation -- ``od_pipe.prepare_window`` then builds the window as for any sequence.  (Replacing ``time_idx`` of a 5 s window, as
tests/random_windows.py does, leaves states whose residual is hundreds of km.)  The driver puts a knot pose on every multiple of
1000 s that carries no frame; the gaps are drawn so that a frame lands on each, which keeps the pose count.

States: the truth plus a tenth of the driver's initial perturbation (``od_pipe.initial_guess``), as tests/accumulate_cases.py: the
oracle accepts the first trial of every call examined (tests/test_dynamics_reference_host.py asserts it).

Gap variants (``kind``):
  mixed     1 .. 60 s, neighbours differ: the lanes of one wave run different step counts
  steps64   the same with a 64-step gap (the longest short edge) followed by a 1-step gap at edges 0 / 1 and, from 13 poses on, 9 / 10
  long31    gaps of 1 .. 20 s with a 65 s (long) edge behind pose 31, the last pose of a dynamics block
  long32    ... behind pose 32, the first pose of the next block
"""
from dataclasses import dataclass

import numpy as np

POSES_4 = (2, 3, 4, 5, 8, 9)
POSES_32 = (15, 16, 17, 31, 32, 33, 64, 65)
POSES_128 = (127, 128, 129)
POSES_256 = (255, 256, 257)
POSES = POSES_4 + POSES_32 + POSES_128 + POSES_256
BOUNDARIES = (4, 16, 32, 128, 256)
RAGGED = (129, 2, 33, 128)
ROWS = 4                        # rows per pose (3 .. 6)
T0 = 10
IT, IT_INIT = 12, 3             # the calls the cases are made for: full phase (alpha = 1, sigma = 1e6) and landmark-only
LAM, LAM_INIT = 1e-4, 0.3       # 0.3: float32(0.3) is 1.2e-8 away, which a landmark-only block of H_tt ~ 1e2 shows (lamda for lam32)
GUESS_SCALE = 0.1
_TRAJ = {}
_CASES = {}


@dataclass
class Case:
    name: str
    states: np.ndarray          # [n, 10]
    xyz: np.ndarray             # [m, 3]
    uv: np.ndarray              # [m, 2]
    conf: np.ndarray            # [m]
    ii: np.ndarray              # [m] int64
    K: np.ndarray               # [n, 4]
    cumrot: np.ndarray          # [n, 4]
    t: np.ndarray               # [n] int64
    truth: np.ndarray           # [n, 10]

    @property
    def n(self):
        return self.states.shape[0]

    @property
    def m(self):
        return self.ii.size

    def args(self, states=None):
        """The arguments of ``dynamics_reference.oracle_levels``."""
        return (self.states if states is None else states, self.cumrot, self.uv, self.xyz, self.ii, self.t, self.K, self.conf)

    def prior(self):
        """A per-pose prior for BA_reg: the truth moved by 0.5 km, symmetric positive definite 6x6 weights of 0.5 .. 3."""
        rng = np.random.default_rng(1000 + self.n)
        sp = self.truth.copy()
        sp[:, :3] += rng.normal(0, 0.5, (self.n, 3))
        Hs = np.stack([np.eye(6) * s for s in rng.uniform(0.5, 3.0, self.n)])
        B = rng.normal(0, 0.1, (self.n, 6, 6))
        return sp, Hs + B @ np.swapaxes(B, 1, 2)


def gaps_for(n, kind, seed):
    """[n - 1] gaps in seconds and the edges whose gap the variant fixes."""
    rng = np.random.default_rng(seed)
    hi = 21 if kind.startswith("long") else 61
    g = rng.integers(1, hi, size=n - 1)
    for k in range(1, n - 1):                   # neighbours differ
        if g[k] == g[k - 1]:
            g[k] = g[k] % (hi - 1) + 1
    fixed = {}
    if kind == "steps64":
        fixed[0] = 64
        if n > 2:
            fixed[1] = 1
        if n >= 13:
            fixed[9], fixed[10] = 64, 1
    elif kind in ("long31", "long32"):
        fixed[int(kind[4:])] = 65
    elif kind != "mixed":
        raise ValueError(kind)
    assert all(k < n - 1 for k in fixed), (n, kind)
    for k, v in fixed.items():
        g[k] = v
    # a frame on every multiple of 1000 s that the window passes (no knot pose), none within 6 s below one at the end
    t = T0
    for k in range(n - 1):
        nxt = (t // 1000 + 1) * 1000
        if t + g[k] > nxt:
            assert k not in fixed
            g[k] = nxt - t
        t += int(g[k])
    if t % 1000 >= 994:
        k = n - 2
        assert k not in fixed and g[k] > t % 1000 - 993
        g[k] -= t % 1000 - 993
    return g.astype(np.int64), fixed


def _trajectory(n_sec):
    from vinsat_amd import synth
    have = _TRAJ.get("traj")
    if have is None or have.shape[0] < n_sec:
        have = synth.integrate_orbit(max(n_sec, 9000))
        _TRAJ["traj"] = have
    return have[:n_sec]


def sequence(frames_t, rows, seed, pixel_noise=1.0, conf=0.95):
    """``synth.make_sequence`` with the frames at ``frames_t``: (detections [M, 6], orbit_np [N, 12])."""
    from vinsat_amd import frames, synth
    frames_t = np.asarray(frames_t, dtype=np.int64)
    n_sec = int(frames_t[-1]) + 6
    traj = _trajectory(n_sec)
    times = np.arange(n_sec)
    ecef_km = frames.eci_to_ecef(traj[:, :3], times)
    orbit_np = np.zeros((n_sec, 12))
    orbit_np[:, :3] = ecef_km * 1000.0
    xe, ye, ze = frames.ecef_to_eci(orbit_np[:, 0] / 1000, orbit_np[:, 1] / 1000, orbit_np[:, 2] / 1000, times)
    pos_eci = np.stack([xe, ye, ze], -1)
    rng = np.random.default_rng(seed)
    frame_col = np.repeat(frames_t, rows)
    m = frame_col.size
    sub = ecef_km[frames_t]
    sub_lat = np.rad2deg(np.arcsin(sub[:, 2] / np.linalg.norm(sub, axis=-1)))
    sub_lon = np.rad2deg(np.arctan2(sub[:, 1], sub[:, 0]))
    lat = np.repeat(sub_lat, rows) + rng.uniform(-1.2, 1.2, size=m)
    lon = np.repeat(sub_lon, rows) + rng.uniform(-2.0, 2.0, size=m)
    xyz = frames.latlon_to_eci(lat, lon, frame_col)
    p = np.repeat(pos_eci[frames_t], rows, axis=0)
    q = np.repeat(frames.nadir_quaternion(pos_eci[frames_t]), rows, axis=0)
    uv = synth.project(p, q, xyz, synth.INTRINSICS) + rng.normal(0.0, pixel_noise, size=(m, 2))
    det = np.stack([frame_col.astype(np.float64), lon, lat, uv[:, 0], uv[:, 1], np.full(m, conf)], -1)
    return det, orbit_np


def case(n, kind="mixed", seed=None):
    """The window of ``n`` poses with the gaps of ``kind``, made once per session and left unchanged."""
    seed = 7000 + n if seed is None else seed
    key = (n, kind, seed)
    if key not in _CASES:
        from vinsat_amd import od_pipe, quat
        g, _fixed = gaps_for(n, kind, seed)
        frames_t = np.concatenate([[T0], T0 + np.cumsum(g)]).astype(np.int64)
        win = od_pipe.prepare_window(*sequence(frames_t, ROWS, seed))
        assert np.array_equal(win.time_idx, frames_t), (n, kind, win.time_idx.size)
        gt, guess = win.states_gt, od_pipe.initial_guess(win, seed=seed)
        st = gt + GUESS_SCALE * (guess - gt)
        st[:, 3:7] = quat.qexp(quat.qlog(gt[:, 3:7]) + GUESS_SCALE * (quat.qlog(guess[:, 3:7]) - quat.qlog(gt[:, 3:7])))
        _CASES[key] = Case(f"{kind}[{n}]", st, win.landmarks_xyz.copy(), win.landmarks_uv.copy(), win.confidences.copy(),
                           win.ii.astype(np.int64), win.intrinsics.copy(), win.cumrot_last.copy(), frames_t, gt.copy())
    return _CASES[key]


STEPS64_POSES = (2, 3, 17, 33, 129)
LONG_POSES = (33, 65, 129)


def factor_cases():
    """Every window of the factor and assembly tests: (n, kind)."""
    out = [(n, "mixed") for n in POSES] + [(n, "steps64") for n in STEPS64_POSES]
    return out + [(n, k) for n in LONG_POSES for k in ("long31", "long32") if not (n == 33 and k == "long32")] + [(34, "long32")]


def ragged():
    return [case(n) for n in RAGGED]
