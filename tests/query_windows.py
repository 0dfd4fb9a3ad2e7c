"""Windows and engines shared by the GPU tests of the three uncertainty queries (test_gpu_covariance.py, test_gpu_reliability.py,
test_gpu_outlier_power.py): the synthetic configurations on a fresh engine, the 20-call schedule, the arguments of ``ba.BA``, and
the smallest shapes that can break the row-to-lane mapping of the row pass."""
import numpy as np

import random_windows

INITS = [it < 10 for it in range(20)]


def _win(cfg, seed=0):
    from vinsat_amd import od_pipe, synth
    det, orb = synth.make_sequence(cfg, seed=seed)
    return od_pipe.prepare_window(det, orb)


def _engine(win, **kw):
    from vinsat_amd.engine import BAEngine
    n = win.states_gt.shape[0]
    eng = BAEngine(n, win.ii.size, **kw)
    eng.upload_observations(win.landmarks_xyz, win.landmarks_uv, win.confidences, win.ii, n)
    eng.upload_window(win.intrinsics, win.cumrot_last, win.time_idx)
    return eng


def _scheduled(win, eng, calls=20):
    from vinsat_amd import od_pipe
    eng.set_states(od_pipe.initial_guess(win), 1e-4)
    eng.run_schedule(list(range(calls)), INITS[:calls])
    st, lam, _, _, _ = eng.get_states()
    return st, lam


def _ba_args(w):
    imu = np.zeros((1, w.states_gt.shape[0], 2, 10))
    imu[0, :, -1, 6:10] = w.cumrot_last
    return imu, w.landmarks_uv[None], w.landmarks_xyz[None], w.ii, w.time_idx, w.intrinsics[None], w.confidences


# ------------------------------------------------------------------------------------------------ smallest shapes
class _Small:
    """A window cut from one of tests/random_windows.py: its first ``n`` poses, and of each pose the first ``rows[i]`` rows
    (poses not named keep theirs)."""

    def __init__(self, seed, n, rows):
        win = random_windows.make(seed)[0]
        assert win.time_idx.size >= n
        keep = []
        for i in range(n):
            k = np.nonzero(win.ii == i)[0]
            want = rows.get(i, k.size)
            assert k.size >= want, (seed, i, k.size)
            keep.append(k[:want])
        keep = np.concatenate(keep)
        order = np.random.default_rng(seed).permutation(keep.size)       # (not pose sorted)
        keep = keep[order]
        self.landmarks_xyz, self.landmarks_uv = win.landmarks_xyz[keep], win.landmarks_uv[keep]
        self.confidences, self.ii = win.confidences[keep], win.ii[keep]
        self.intrinsics, self.cumrot_last, self.time_idx = win.intrinsics[:n], win.cumrot_last[:n], win.time_idx[:n]
        self.states0 = win.states_gt[:n].copy()
        self.n, self.m = n, keep.size


# The damping of the small windows' query.  Three rows on one pose of two determine that pose's six coordinates and no more: the
# redundancy the rows lack comes from the damping, and so does the conditioning -- the dynamics factors weigh 1e4 .. 1e6 against
# it.  At 100 the dense references of the 2-pose window differ (LU against Cholesky, at these states) by 2.4e-10 in del_pos and
# 2.3e-10 in ext_pos, less elsewhere (17 poses: 2.9e-11), so the 1e-8 bar holds ten times the spread; at 1 they differ by 9.6e-8.
SMALL_LAMDA = 100.0


def _small_windows():
    seed = next(s for s in range(200) if _fits(s))
    two = _Small(seed, 2, {0: 3, 1: 0})
    many = _Small(seed, 17, {0: 1, 1: 16, 2: 17, 3: 33})
    dead = _Small(seed, 17, {})
    dead.confidences = np.zeros_like(dead.confidences)
    return two, many, dead


def _fits(seed):
    win = random_windows.make(seed)[0]
    if win.time_idx.size < 17:
        return False
    c = np.bincount(win.ii, minlength=17)
    return c[0] >= 3 and c[1] >= 16 and c[2] >= 17 and c[3] >= 33


def _batch_engine(wins, chunk=None, sizes=None, **kw):
    from vinsat_amd.engine import BAEngine
    n_max, m_max = sizes or (max(w.n for w in wins), max(w.m for w in wins))
    eng = BAEngine(n_max, m_max, windows=len(wins), **kw)
    if chunk is not None:
        eng.set_solver(chunk)
    for k, w in enumerate(wins):
        eng.upload_observations(w.landmarks_xyz, w.landmarks_uv, w.confidences, w.ii, w.n, window=k)
        eng.upload_window(w.intrinsics, w.cumrot_last, w.time_idx, window=k)
        eng.set_states(w.states0, SMALL_LAMDA, window=k)
    return eng
