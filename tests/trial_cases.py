"""Windows on the seams of the trial kernel's index arithmetic (``k_trial``, vinsat_amd/csrc/vba_trial.hip).  No GPU needed (the
library's host code is: build first).  Every window is small -- n <= 300, m <= 2300 -- and is made once per session.

They are the windows of tests/dynamics_cases.py (``case(n, kind)``: consistent orbit, the truth plus a tenth of the driver's
perturbation, so the oracle accepts the first trial), with their rows laid out anew where the layout is the point (``relayout``: the
first ``counts[i]`` rows of pose i, repeated in turn like tests/accumulate_cases.py does, shuffled).

  seams16        2, 15, 16, 17, 30, 31, 32, 46 poses: 15 edges per pose-chain block of the 16-lane geometry -- the 16th pose of a block,
                 and the last pose under ``j / 15 >= nblk_dyn`` when n_max - 1 is a multiple of 15 (16, 31, 46);
                 16 poses again on handles of n_max = 31 and 129 (``Spec.n_max``)
  seams256       255, 256, 257 poses: block 1 of the plain geometry holds one edge-less pose / one edge
  leaders        300 poses with one row each (observation block 0 numbers 256 leading rows; 16 rounds of 16 trial states in LDS);
                 17 poses in one block (two rounds, one live group in the second);
                 46 poses with row counts 0 (first), 1, 7, 0, ... 0 (last), 260 rows: poses without rows, a block whose first row
                 continues a pose
  tiles          32 poses, m = 255, 257, 768, 1000, 1025, 2047, 2300 rows: 1, 2, 3, 4, 5, 8, 9 observation tiles -- m = 255, 0, 1 mod 256,
                 ragged last blocks for 2 / 4 / 8 tiles per block; uneven counts, so tiles begin inside a pose
  long           dynamics_cases ``long31`` at 65 poses: the slot behind the pose-chain blocks is occupied
  BA_reg         ``Spec.reg``: 16, 31, 46, 257 poses and the 1025-row window with the per-pose prior of ``Case.prior``
  ragged()       46, 2, 32 (1025 rows), 17 poses on one handle of n_max = 46, m_max = 1025: a window below a whole tile beside one of five
"""
from dataclasses import dataclass, replace

import numpy as np

import dynamics_cases as D

IT, IT_INIT, LAM, LAM_INIT = D.IT, D.IT_INIT, D.LAM, D.LAM_INIT
SEAMS16 = (2, 15, 16, 17, 30, 31, 32, 46)
SEAMS256 = (255, 256, 257)
TILE_ROWS = (255, 257, 768, 1000, 1025, 2047, 2300)
_CASES = {}


@dataclass(frozen=True)
class Spec:
    case: object                # dynamics_cases.Case
    n_max: int
    m_max: int
    reg: bool = False

    @property
    def name(self):
        c = self.case
        return f"{c.name}{' reg' if self.reg else ''}" + (f" on n_max {self.n_max}" if self.n_max != c.n else "")


def relayout(c, counts, name, seed):
    """``c`` with the first ``counts[i]`` rows of pose i (repeated in turn where it has fewer), shuffled."""
    key = ("relayout", name)
    if key not in _CASES:
        rng = np.random.default_rng(seed)
        take = []
        for i, k in enumerate(counts):
            own = np.nonzero(c.ii == i)[0]
            take.append(np.resize(own, int(k)) if k else own[:0])
        take = np.concatenate(take)
        take = take[rng.permutation(take.size)]
        _CASES[key] = replace(c, name=name, xyz=c.xyz[take].copy(), uv=c.uv[take].copy(), conf=c.conf[take].copy(), ii=c.ii[take].copy())
    return _CASES[key]


def one_row_each():
    c = D.case(300)
    return relayout(c, np.ones(300, dtype=np.int64), "one-row-each[300]", 11)


def holes():
    """46 poses, 260 rows: the first and the last pose and every fourth without rows; tile 1 begins inside a pose (asserted)."""
    cnt = np.array([(0, 1, 7, 13)[i % 4] for i in range(46)], dtype=np.int64)
    cnt[-1] = 0
    cnt[21] += 260 - int(cnt.sum())
    c = relayout(D.case(46), cnt, "holes[46]", 12)
    s = np.sort(c.ii)
    assert c.m == 260 and s[255] == s[256] and cnt[0] == 0 and cnt[-1] == 0
    return c


def rich(n, rows, seed=None):
    """``dynamics_cases.case(n)`` with ``rows`` rows per pose instead of 4 (the same gaps, the same way to the states)."""
    seed = 7000 + n if seed is None else seed
    key = ("rich", n, rows, seed)
    if key not in _CASES:
        from vinsat_amd import od_pipe, quat
        g, _fixed = D.gaps_for(n, "mixed", seed)
        frames_t = np.concatenate([[D.T0], D.T0 + np.cumsum(g)]).astype(np.int64)
        win = od_pipe.prepare_window(*D.sequence(frames_t, rows, seed))
        assert np.array_equal(win.time_idx, frames_t)
        gt, guess = win.states_gt, od_pipe.initial_guess(win, seed=seed)
        st = gt + D.GUESS_SCALE * (guess - gt)
        st[:, 3:7] = quat.qexp(quat.qlog(gt[:, 3:7]) + D.GUESS_SCALE * (quat.qlog(guess[:, 3:7]) - quat.qlog(gt[:, 3:7])))
        _CASES[key] = D.Case(f"rich[{n}]", st, win.landmarks_xyz.copy(), win.landmarks_uv.copy(), win.confidences.copy(),
                             win.ii.astype(np.int64), win.intrinsics.copy(), win.cumrot_last.copy(), frames_t, gt.copy())
    return _CASES[key]


def tiles(m):
    """32 poses, ``m`` rows out of 100 per pose, uneven counts (0 .. ~3 m / 32), so that tile boundaries fall inside poses."""
    rng = np.random.default_rng(2000 + m)
    w = rng.uniform(0.0, 1.0, 32)
    w[5] = 0.0
    cnt = np.floor(w / w.sum() * m).astype(np.int64)
    cnt[17] += m - int(cnt.sum())
    c = relayout(rich(32, 100), cnt, f"tiles[{m}]", 13 + m)
    assert c.m == m
    return c


def spec(c, n_max=None, m_max=None, reg=False):
    return Spec(c, c.n if n_max is None else n_max, c.m if m_max is None else m_max, reg)


GROUPS = {
    "seams16": lambda: [spec(D.case(n)) for n in SEAMS16] + [spec(D.case(16), n_max=31), spec(D.case(16), n_max=129)],
    "seams256": lambda: [spec(D.case(n)) for n in SEAMS256],
    "leaders": lambda: [spec(one_row_each()), spec(D.case(17, "steps64")), spec(holes())],
    "tiles": lambda: [spec(tiles(m)) for m in TILE_ROWS],
    "long": lambda: [spec(D.case(65, "long31"))],
    "BA_reg": lambda: [spec(D.case(n), reg=True) for n in (16, 31, 46, 257)] + [spec(tiles(1025), reg=True)],
}


def group(name):
    return GROUPS[name]()


def all_specs():
    return [s for g in GROUPS for s in group(g)]


def ragged():
    """The windows of the ragged batch, and the handle's (n_max, m_max)."""
    wins = [D.case(46), D.case(2), tiles(1025), D.case(17)]
    return wins, 46, 1025
