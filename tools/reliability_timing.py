"""Time of the reliability query (vba_reliability, HIP events on the handle's stream: front + inversion + row pass) next to the
covariance query alone (front + inversion) on the same handle, after the 20-call schedule.  Cases: C3 (500 poses, 50 000 rows) as
one window and as 256 windows.  Each figure is the median of --reps HIP-event intervals after two warm-up queries; the two
queries alternate, so that clock and cache state drift hits both alike.  The row pass is reported as the difference of the medians
and as achieved bytes/s over the bytes it moves per row (seven doubles and an index read, two doubles written: 76 B) plus the
per-pose block.

    python tools/reliability_timing.py [--out profiles/r07_reliability_timing.json] [--cases w1,w256] [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROW_BYTES = 7 * 8 + 4 + 2 * 8           # ox..oconf, wraw, perm; leverage, wtest
POSE_BYTES = 21 * 8 + 14 * 8 + 8 + 24   # S_i's upper triangle, state + intrinsics, CSR range, pose_stats


def _case(name, W, reps):
    from vinsat_amd import od_pipe, synth
    from vinsat_amd.engine import BAEngine
    det, orb = synth.make_sequence("C3")
    win = od_pipe.prepare_window(det, orb)
    n, m = win.states_gt.shape[0], win.ii.size
    eng = BAEngine(n, m, windows=W)
    st0 = od_pipe.initial_guess(win)
    for w in range(W):
        eng.upload_observations(win.landmarks_xyz, win.landmarks_uv, win.confidences, win.ii, n, window=w)
        eng.upload_window(win.intrinsics, win.cumrot_last, win.time_idx, window=w)
        eng.set_states(st0, 1e-4, window=w)
    eng.run_schedule(list(range(20)), [it < 10 for it in range(20)])
    for _ in range(2):
        eng.covariance(19, damped=True)
        eng.reliability(19, damped=True)
    cov, rel = [], []
    for _ in range(reps):
        eng.covariance(19, damped=True)
        cov.append(eng.last_covariance_ms())
        eng.reliability(19, damped=True)
        rel.append(eng.last_reliability_ms())
    mode, chunk = eng.mode()
    eng.close()
    c, r = float(np.median(cov)), float(np.median(rel))
    moved = W * (m * ROW_BYTES + n * POSE_BYTES)
    row_ms = r - c
    return dict(case=name, config="C3", windows=W, poses=n, rows=m, mode=mode, chunk=chunk, reps=reps,
                covariance_ms_median=c, covariance_ms_min=float(np.min(cov)), covariance_ms_all=[float(x) for x in cov],
                reliability_ms_median=r, reliability_ms_min=float(np.min(rel)), reliability_ms_all=[float(x) for x in rel],
                row_pass_ms=row_ms, row_pass_bytes=moved, row_pass_GBps=(moved / (row_ms * 1e-3) / 1e9) if row_ms > 0 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_reliability_timing.json"))
    ap.add_argument("--cases", default="w1,w256")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    table = dict(w1=1, w256=256)
    res = []
    for c in a.cases.split(","):
        r = _case(c, table[c], a.reps)
        print(json.dumps(r), flush=True)
        res.append(r)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
