"""Time of scaled data snooping in one call (vba_snoop_scaled: front + inversion + three launches, HIP events on the handle's
stream) beside the two-step form it replaces (vba_outlier_power for s0, a host multiply, vba_snoop at quantile * s0: two fronts
and two inversions) on the same handle, after the 20-call schedule.  Cases: one C3 window; 22 C3 windows (ragged: pose counts
500 .. 479), where the two-step form needs one vba_snoop per distinct critical value -- 22 calls, each over the whole handle, timed
as such (their masks are not those of the one-call form: a call applies its one value to every window; this tool times, the
tests compare).  Each figure is the median of --reps HIP-event intervals after two warm-ups; the two forms alternate, with
vba_snoop_restore between them, so that both start from the same confidences and clock and cache drift hits both alike.

    python tools/snoop_scaled_timing.py [--out profiles/r08_snoop_scaled_timing.json] [--cases c3,w22] [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from covariance_timing import _handle  # noqa: E402  (the same handles: tools/covariance_timing.py)

QUANTILE = 3.29


def _one_call(eng):
    eng.snoop_scaled(19, QUANTILE, damped=True)
    ms = eng.last_snoop_ms()
    eng.snoop_restore()
    return ms


def _two_step(eng, W):
    fit = eng.outlier_power(19, damped=True)[5]
    ms = eng.last_outlier_power_ms()
    calls = 0
    for crit in QUANTILE * np.sqrt(fit[:W, 4]):
        if crit > 0:                            # (a window without an s0 has no critical value)
            eng.snoop(19, float(crit), damped=True)
            ms += eng.last_snoop_ms()
            calls += 1
    eng.snoop_restore()
    return ms, calls


def _case(name, cfg, W, ragged, reps):
    eng, _ = _handle(cfg, W, ragged)
    eng.run_schedule(list(range(20)), [it < 10 for it in range(20)])
    for _ in range(2):
        _one_call(eng)
        _two_step(eng, W)
    one, two, calls = [], [], 0
    for _ in range(reps):
        one.append(_one_call(eng))
        ms, calls = _two_step(eng, W)
        two.append(ms)
    mode, chunk = eng.mode()
    rows = int(sum(eng.m))
    eng.close()
    a, b = float(np.median(one)), float(np.median(two))
    return dict(case=name, config=cfg, windows=W, ragged=ragged, rows=rows, mode=mode, chunk=chunk, reps=reps, quantile=QUANTILE,
                snoop_scaled_ms_median=a, snoop_scaled_ms_min=float(np.min(one)), snoop_scaled_ms_all=[float(x) for x in one],
                two_step_ms_median=b, two_step_ms_min=float(np.min(two)), two_step_ms_all=[float(x) for x in two],
                two_step_snoop_calls=calls, ratio=a / b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_snoop_scaled_timing.json"))
    ap.add_argument("--cases", default="c3,w22")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    table = dict(c3=("C3", 1, False), w22=("C3", 22, True))
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
