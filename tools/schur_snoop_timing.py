#!/usr/bin/env python
"""Time of free-landmark data snooping (``vba_schur_snoop``) next to ``vba_schur_reliability`` on the same handle.

500 poses / 20 000 landmarks / 247 517 rows (the problem of ``tools/schur_reliability_timing.py``).  Per
repeat, from the same state and the same (restored) weights: one reliability query, one snoop at ``crit = +inf`` (the passes of
the rule run and reject nothing), one snoop at a critical value that rejects about 1 % of the rows, then ``restore_rejected``.
At most one row per pose goes by its own test (500 of 247 517 rows: 0.2 %), so the landmark part of the state is set one
catalogue sigma off the catalogue (seeded): catalogue entries are then rejected too, each with its whole track.  The critical
value is the percentile of the finite tests of the first query, among a fixed list, whose rejected share comes closest to 1 %
(unscaled, ``min_rows`` 6, ``min_track`` 3); with one rejection per group and call the share stays well below that on this
problem, and the record tells what it was.  Two warm-ups, then
the median of 20 HIP-event intervals of each (``last_reliability_ms``, ``last_snoop_ms``); the calls are interleaved so that a
drift of the clocks meets all of them alike.  The figure is the ratio of a snoop to the reliability query of the same run, with
its range over the extremes.  Writes one JSON record (default ``profiles/schur_snoop_timing.json``) and prints it.

    python tools/schur_snoop_timing.py [--poses 500] [--landmarks 20000] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=500)
    ap.add_argument("--landmarks", type=int, default=20000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schur_snoop_timing.json"))
    a = ap.parse_args()
    from vinsat_amd import synth
    from vinsat_amd.schur import SchurBA
    d = synth.make_tracked_landmarks(n_poses=a.poses, n_landmarks=a.landmarks, seed=0)
    st = d["states_gt"].copy()
    st[:, :3] += np.random.default_rng(1).normal(0, 2.0, st[:, :3].shape)
    sb = SchurBA(st, d["X0"], d["uv"], np.full(d["uv"].shape[0], 0.95), d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], sigma_prior=d["sigma"])
    X = d["X0"] + np.random.default_rng(2).normal(0, d["sigma"], d["X0"].shape)
    sb.set_state(st, X)
    rel = sb.reliability(0.0)
    tests = np.concatenate([rel["wtest"], rel["lm_wtest"]])
    tests = tests[np.isfinite(tests)]
    tried = {}
    for pct in (99.9, 99.5, 99.0, 98.0, 95.0, 90.0, 80.0, 50.0):
        c = float(np.percentile(tests, pct))
        got = sb.snoop(0.0, c, False, 6, 3)
        sb.restore_rejected()
        tried[pct] = (c, (got["rows"] + got["rows_via_landmarks"]) / float(d["uv"].shape[0]))
    pct = min(tried, key=lambda q: abs(tried[q][1] - 0.01))
    crit = tried[pct][0]
    r_ms, none_ms, some_ms, counts = [], [], [], None
    for k in range(a.warmup + a.repeats):
        sb.reliability(0.0)
        r = sb.last_reliability_ms()
        none = sb.snoop(0.0, float("inf"), False, 6, 3)
        s_none = sb.last_snoop_ms()
        some = sb.snoop(0.0, crit, False, 6, 3)
        s_some = sb.last_snoop_ms()
        sb.restore_rejected()
        assert (none["rows"], none["landmarks"]) == (0, 0) and (counts is None or counts == some)
        counts = some
        if k >= a.warmup:
            r_ms.append(r)
            none_ms.append(s_none)
            some_ms.append(s_some)
    med = lambda x: float(np.median(x))
    span = lambda x: [float(min(x)), float(max(x))]
    ratio = lambda x: {"median": med(x) / med(r_ms), "min_max": [float(min(x) / max(r_ms)), float(max(x) / min(r_ms))]}
    rec = {"poses": a.poses, "landmarks": int(d["X0"].shape[0]), "rows": int(d["uv"].shape[0]), "repeats": a.repeats, "warmup": a.warmup,
           "crit_some": crit, "crit_some_percentile_of_tests": pct, "rejected_some": {k: counts[k] for k in ("rows", "landmarks", "rows_via_landmarks")},
           "rejected_share_of_rows": (counts["rows"] + counts["rows_via_landmarks"]) / float(d["uv"].shape[0]),
           "reliability_ms_median": med(r_ms), "reliability_ms_min_max": span(r_ms),
           "snoop_none_ms_median": med(none_ms), "snoop_none_ms_min_max": span(none_ms),
           "snoop_some_ms_median": med(some_ms), "snoop_some_ms_min_max": span(some_ms),
           "rule_passes_ms_median": med(np.array(none_ms) - np.array(r_ms)),
           "ratio_snoop_none_over_reliability": ratio(none_ms), "ratio_snoop_some_over_reliability": ratio(some_ms),
           "s0sq": rel["fit"]["s0sq"], "max_wtest": rel["fit"]["max_wtest"]}
    sb.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
