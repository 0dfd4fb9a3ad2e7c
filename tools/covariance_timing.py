"""Time of the covariance query (vba_covariance, HIP events on the handle's stream, after warm-up) beside the 20-call schedule of
the same handle.  Cases: one C3 window (its default partitioned path, and the sequential walk forced by chunk 0), 22 C3 windows
(ragged: pose counts 500 .. 479), 4096 C2 windows.  The two figures are different kinds of measurement: the query is the median of
HIP-event intervals on the stream (front + inversion), the schedule the median host wall time of a synchronous vba_run_schedule
(launch and synchronisation included).

    python tools/covariance_timing.py [--out profiles/covariance_timing.json] [--cases c3,w22,w4096] [--reps 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _handle(cfg, W, ragged):
    from vinsat_amd import od_pipe, synth
    from vinsat_amd.engine import BAEngine
    det, orb = synth.make_sequence(cfg)
    win = od_pipe.prepare_window(det, orb)
    n, m = win.states_gt.shape[0], win.ii.size
    eng = BAEngine(n, m, windows=W)
    st0 = od_pipe.initial_guess(win)
    for w in range(W):
        k = n - (w if ragged else 0)
        rows = win.ii < k
        eng.upload_observations(win.landmarks_xyz[rows], win.landmarks_uv[rows], win.confidences[rows], win.ii[rows], k, window=w)
        eng.upload_window(win.intrinsics[:k], win.cumrot_last[:k], win.time_idx[:k], window=w)
        eng.set_states(st0[:k], 1e-4, window=w)
    return eng, st0


def _case(name, cfg, W, ragged, reps, chunk=None):
    eng, _ = _handle(cfg, W, ragged)
    if chunk is not None:
        eng.set_solver(chunk)
    inits = [it < 10 for it in range(20)]
    S0, L0, _, _, _ = eng.get_states_all()
    eng.run_schedule(list(range(20)), inits)        # warm-up (graph capture)
    walls = []
    for _ in range(5):
        eng.set_states_all(S0, L0)
        t0 = time.perf_counter()
        eng.run_schedule(list(range(20)), inits)
        walls.append((time.perf_counter() - t0) * 1e3)
    sched_ms = float(np.median(walls))
    for _ in range(2):
        eng.covariance(19, damped=True)
    qs = []
    for _ in range(reps):
        eng.covariance(19, damped=True)
        qs.append(eng.last_covariance_ms())
    mode, chunk = eng.mode()
    eng.close()
    return dict(case=name, config=cfg, schedule20_wall_ms_all=walls, windows=W, ragged=ragged, mode=mode, chunk=chunk, schedule20_wall_ms=sched_ms,
                query_ms_median=float(np.median(qs)), query_ms_min=float(np.min(qs)), query_ms_all=[float(x) for x in qs],
                query_over_schedule=float(np.median(qs)) / sched_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance_timing.json"))
    ap.add_argument("--cases", default="c3,c3seq,w22,w4096")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    table = dict(c3=("C3", 1, False), c3seq=("C3", 1, False, 0), w22=("C3", 22, True), w4096=("C2", 4096, False))
    res = []
    for c in a.cases.split(","):
        r = _case(c, *table[c][:3], a.reps, *table[c][3:])
        print(json.dumps(r), flush=True)
        res.append(r)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
