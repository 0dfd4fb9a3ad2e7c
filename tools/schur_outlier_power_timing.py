#!/usr/bin/env python
"""Time of the free-landmark outlier power query (``vba_schur_outlier_power``) next to ``vba_schur_reliability`` on the same handle.

500 poses / 20 000 landmarks (the 3 000 x 3 000 reduced system of DESIGN section 9, as ``bench.py`` builds it): two warm-ups, then
the median of 20 HIP-event intervals of each (``last_outlier_power_ms``, ``last_reliability_ms``), both from the same state and
interleaved so that a drift of the clocks meets them alike.  The power query runs the device part of the reliability query with its
own row pass in the place of ``k_rel_rows`` and two short passes behind it: the ratio is what those cost.  The spread of each
(min, max) is recorded beside its median.  Writes one JSON record (default ``profiles/schur_outlier_power_timing.json``) and prints it.

    python tools/schur_outlier_power_timing.py [--poses 500] [--landmarks 20000] [--out FILE]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schur_outlier_power_timing.json"))
    a = ap.parse_args()
    from vinsat_amd import synth
    from vinsat_amd.schur import SchurBA
    d = synth.make_tracked_landmarks(n_poses=a.poses, n_landmarks=a.landmarks, seed=0)
    st = d["states_gt"].copy()
    st[:, :3] += np.random.default_rng(1).normal(0, 2.0, st[:, :3].shape)
    sb = SchurBA(st, d["X0"], d["uv"], np.full(d["uv"].shape[0], 0.95), d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], sigma_prior=d["sigma"])
    p_ms, r_ms = [], []
    for k in range(a.warmup + a.repeats):
        sb.set_state(st, d["X0"])
        r = sb.reliability(0.0)
        p = sb.outlier_power(0.0)
        if k >= a.warmup:
            r_ms.append(sb.last_reliability_ms())
            p_ms.append(sb.last_outlier_power_ms())
    med = lambda x: float(np.median(x))
    span = lambda x: [float(min(x)), float(max(x))]
    fin = lambda x: float(np.max(x[np.isfinite(x)], initial=0.0))
    rec = {"poses": a.poses, "landmarks": int(d["X0"].shape[0]), "rows": int(d["uv"].shape[0]), "reduced_system": 6 * a.poses,
           "repeats": a.repeats, "warmup": a.warmup,
           "outlier_power_ms_median": med(p_ms), "outlier_power_ms_min_max": span(p_ms),
           "reliability_ms_median": med(r_ms), "reliability_ms_min_max": span(r_ms),
           "extra_ms_median": med(np.array(p_ms) - np.array(r_ms)),
           "ratio_power_over_reliability": med(p_ms) / med(r_ms),
           "ratio_power_over_reliability_min_max": [float(min(p_ms) / max(r_ms)), float(max(p_ms) / min(r_ms))],
           "info": int(p["info"]), "leading_fit_equal": list(p["fit"].values())[:8] == list(r["fit"].values()),
           "median_mdb_px": med(p["mdb"]), "max_ext_pos_km": p["fit"]["max_ext_pos"], "median_lm_mdb_km": med(p["lm_mdb"][np.isfinite(p["lm_mdb"])]),
           "max_lm_del_pos_km": fin(p["lm_del_pos"])}
    sb.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
