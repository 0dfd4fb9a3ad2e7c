"""The planted-outlier window of the data snooping tests (tests/test_snoop_host.py vets it on the CPU, tests/test_gpu_snoop.py
runs it on the device) and the snooping loop over an abstract engine, so that both run the same rounds.

The values below were chosen on the CPU (tests/test_snoop_host.py asserts what they must deliver; DESIGN.md section 16 records
the oracle's counts): detections of the C2 sequence moved by DISP pixels in a random direction, inside the 1000 px ground-truth
mask of the data preparation, so the planted rows stay in the window."""
import functools

import numpy as np

CFG, DISP, FRACTION, SEED = "C2", 300.0, 0.02, 5
CRIT, ROUNDS, CALLS, MODE, MIN_ROWS = 6.0, 8, 4, 0, 6        # crit in wtest's own units
ITER = 19


@functools.lru_cache(maxsize=None)
def planted():
    """(detections with the planted rows, orbit, window, planted rows of the window in input order)."""
    from vinsat_amd import od_pipe, synth
    det, orb = synth.make_sequence(CFG, seed=0)
    clean = od_pipe.prepare_window(det, orb)
    rng = np.random.default_rng(SEED)
    rows = np.sort(rng.choice(det.shape[0], int(round(FRACTION * det.shape[0])), replace=False))
    ang = rng.uniform(0.0, 2.0 * np.pi, rows.size)
    bad = det.copy()
    bad[rows, 3] += DISP * np.cos(ang)
    bad[rows, 4] += DISP * np.sin(ang)
    win = od_pipe.prepare_window(bad, orb)
    assert win.ii.size == clean.ii.size             # (the mask of the preparation kept every planted row)
    idx = np.nonzero((win.landmarks_uv != clean.landmarks_uv).any(axis=1))[0]
    assert idx.size == rows.size
    return bad, orb, win, idx


def oracle_calls(win, conf, st, lam, iters, inits):
    from oracle import ba_oracle as O
    for it, ini in zip(iters, inits):
        st, lam, _, _ = O.ba_iteration(it, st, win.cumrot_last, win.landmarks_uv, win.landmarks_xyz, win.ii, win.time_idx,
                                       win.intrinsics, conf, lam, initialize=ini)
    return st, lam


@functools.lru_cache(maxsize=None)
def oracle_loop():
    """The snooping loop on the CPU oracle alone.  Returns dict(rounds=[dict(mask, ambiguous, margin)], total, err_before,
    err_after): position errors in km (mean over the poses) without and with snooping."""
    import snoop_oracle as S
    from vinsat_amd import od_pipe
    _, _, win, _ = planted()
    n = win.states_gt.shape[0]
    conf = win.confidences.copy()
    st, lam = oracle_calls(win, conf, od_pipe.initial_guess(win), 1e-4, range(20), [it < 10 for it in range(20)])
    err_before = float(np.linalg.norm(st[:, :3] - win.states_gt[:, :3], axis=1).mean())
    rounds, total = [], np.zeros(win.ii.size, dtype=bool)
    for _ in range(ROUNDS):
        wt, w = S.at_states(win, st, lam, it=ITER, conf=conf)
        mask, _ = S.select(wt, w, win.ii, n, CRIT, MODE, MIN_ROWS)
        rounds.append(dict(mask=mask, ambiguous=S.ambiguous(wt, w, win.ii, n, CRIT, MODE, MIN_ROWS), margin=S.margin_of(wt)))
        if not mask.any():
            break
        total |= mask
        conf[mask] = 0.0
        st, lam = oracle_calls(win, conf, st, lam, [ITER] * CALLS, [False] * CALLS)
    err_after = float(np.linalg.norm(st[:, :3] - win.states_gt[:, :3], axis=1).mean())
    return dict(rounds=rounds, total=total, err_before=err_before, err_after=err_after)
