"""The cases of the covariance path tests (tests/test_cov_reference_host.py, tests/test_gpu_covariance_paths.py): synthetic windows
from the generator of the solve-path tests, pose counts chosen for their position relative to a chunk.

Pose counts per chunk size s -- the smallest that reach each branch of k_cov_chunk / k_cov_sep / k_cov_fix (csrc/vba_cov.hip, csrc/vba_cov_walk.h), with
P = ceil(n / s) chunks, P - 1 separators, the last chunk holding n - (P - 1) s poses:

  P = 1 (n <= s: no separator, k_cov_sep returns at once, k_cov_fix adds a zero correction)      s=2: 2;  3: 3;  5: 4, 5;  8: 8
  last chunk of 1 pose (n = k s + 1)            s=2: 3, 5, 9;  3: 4, 7, 10;  5: 6, 11, 16;  8: 9, 17, 33;  12: 13, 25;  60: 61
  last chunk of s - 1 poses                     s=2: the same;  5: 9;  8: 15
  last chunk of s poses (n = k s)               s=2: 4;  3: 6;  5: 10;  8: 16;  12: 24;  60: 120
  one interior pose per chunk                   s=2 throughout
  P = 2: first and last chunk only, each coupled on one side; P >= 3: chunks coupled on both sides

``ROWS`` = 400 rows per pose and ``GAP`` = 60 s between frames (window_for's ``gaps``), not the 3 rows and 5 s of the solve-path
tests: with those the undamped system is indefinite (INDEFINITE in the fp64 recurrence, smallest eigenvalue -0.1 .. -0.8 against
4e10), at the initial guess and after calls 9 and 10 alike.  The dynamics factor leaves the orbit's six initial conditions to the
observations, and the velocities are seen only through positions a gap apart: their information grows with rows x gap^2.
400 rows and not fewer because tests/test_cov_reference_host.py holds the systems the device query meets (after calls 9 and 10)
to the same condition as the start states -- the smallest planted fault 100 times above 16 x the worst fp64 reference figure of any
case, i.e. that figure below 6.25e-10: 20 rows / 60 s reach 1.1e-9 there (n = 2), 100 rows 1.5e-9 (n = 120), 400 rows 5.4e-10.
Gaps of 60 s stay on the ordinary dynamics path (no long-gap edges)."""
import numpy as np

import solve_residual as S

ROWS = 400
GAP = 60                        # seconds between frames (window_for's ``gaps``)
SCHEDULE = ((9, True), (10, False))     # the calls in front of the query, from the initial guess with lamda 1e-4
QUERY_ITER = 14
CHUNKED = {2: (2, 3, 4, 5, 9), 3: (3, 4, 6, 7, 10), 5: (4, 5, 6, 9, 10, 11, 16), 8: (8, 9, 15, 16, 17, 33), 12: (13, 24, 25), 60: (61, 120)}
# vba_upload_observations / vba_upload_window accept 2 <= n <= n_max: 2 is the smallest window
SEQUENTIAL = (2, 3, 65)
LOOSE = 48                      # n_max of the loose handle (n + 7 where n > 48): the grid then holds chunks with ch >= P


def loose_n_max(n):
    return LOOSE if n <= LOOSE else n + 7


def batch(s, n_max):
    """Pose counts of the five-window handle: (n_max, s + 1, s, 2, 2 s - 1)."""
    return (n_max, s + 1, s, 2, 2 * s - 1)


BATCHES = ((5, 16), (2, 9))     # (s, n_max)

_WINDOWS = {}


def window(n, seed=None):
    """(win, time_idx, states0) of ``n`` poses, made once per session and left unchanged (seed: n unless given)."""
    key = (n, n if seed is None else seed)
    if key not in _WINDOWS:
        _WINDOWS[key] = S.window_for(n, ROWS, key[1], gaps=np.full(n - 1, GAP))
    return _WINDOWS[key]


def batch_windows(s, n_max):
    return [window(n, seed=500 + 10 * s + k) for k, n in enumerate(batch(s, n_max))]


def oracle_bands(w, stepped):
    """(bands [n, 3, 9, 9], lamda) of a full-phase call QUERY_ITER by the NumPy oracle: at the window's start states (initial
    guess, lamda 1e-4), or, ``stepped``, at the states SCHEDULE leaves from there -- the system the device query inverts."""
    from oracle import ba_oracle as O
    win, t, st = w
    lam = 1e-4
    args = (win.cumrot_last, win.landmarks_uv, win.landmarks_xyz, win.ii, t, win.intrinsics, win.confidences)
    for it, init in (SCHEDULE if stepped else ()):
        st, lam = O.ba_iteration(it, st, *args, lam, initialize=init)[:2]
    d = {}
    O.ba_iteration(QUERY_ITER, st, *args, lam, initialize=False, debug=d)
    return d["bands"], lam


def all_single_cases():
    """[(s, n)] of every single-window case; s = 0: the sequential walk."""
    return [(s, n) for s, ns in CHUNKED.items() for n in ns] + [(0, n) for n in SEQUENTIAL]
