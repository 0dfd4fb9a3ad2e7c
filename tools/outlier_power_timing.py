"""Time of the outlier power query (vba_outlier_power, HIP events on the handle's stream: front + inversion + row pass + window
totals) beside the reliability query (front + inversion + its row pass) on the same handle, after the 20-call schedule.  Cases:
one C3 window, 22 C3 windows (ragged: pose counts 500 .. 479), 4096 C2 windows.  Each figure is the median of --reps HIP-event
intervals after two warm-up queries each; the two queries alternate, so that clock and cache state drift hits both alike.  The
question the ratio answers: does the query cost less than 1.3 x the reliability query (the row pass reads the same streams and
writes twice the outputs; the front and the inversion are shared)?

    python tools/outlier_power_timing.py [--out profiles/r07_outlier_power_timing.json] [--cases c3,w22,w4096] [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from covariance_timing import _handle  # noqa: E402  (the same handles: tools/covariance_timing.py)


def _case(name, cfg, W, ragged, reps):
    eng, _ = _handle(cfg, W, ragged)
    eng.run_schedule(list(range(20)), [it < 10 for it in range(20)])
    for _ in range(2):
        eng.reliability(19, damped=True)
        eng.outlier_power(19, damped=True, crit=3.29)
    rel, pw = [], []
    for _ in range(reps):
        eng.reliability(19, damped=True)
        rel.append(eng.last_reliability_ms())
        eng.outlier_power(19, damped=True, crit=3.29)
        pw.append(eng.last_outlier_power_ms())
    mode, chunk = eng.mode()
    rows = int(sum(eng.m))
    eng.close()
    r, p = float(np.median(rel)), float(np.median(pw))
    return dict(case=name, config=cfg, windows=W, ragged=ragged, rows=rows, mode=mode, chunk=chunk, reps=reps,
                reliability_ms_median=r, reliability_ms_min=float(np.min(rel)), reliability_ms_all=[float(x) for x in rel],
                outlier_power_ms_median=p, outlier_power_ms_min=float(np.min(pw)), outlier_power_ms_all=[float(x) for x in pw],
                ratio=p / r, expected_below=1.3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_outlier_power_timing.json"))
    ap.add_argument("--cases", default="c3,w22,w4096")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    table = dict(c3=("C3", 1, False), w22=("C3", 22, True), w4096=("C2", 4096, False))
    res = []
    for c in a.cases.split(","):
        r = _case(c, *table[c], a.reps)
        print(json.dumps(r), flush=True)
        res.append(r)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
