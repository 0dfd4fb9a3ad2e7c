#!/usr/bin/env python
"""Time of the free-landmark reliability query (``vba_schur_reliability``) next to ``vba_schur_covariance`` and one
``vba_schur_iterate`` on the same handle.

500 poses / 20 000 landmarks (the 3 000 x 3 000 reduced system of DESIGN section 9, as ``bench.py`` builds it): two warm-ups,
then the median of 20 HIP-event intervals of each (``last_reliability_ms``; ``last_covariance_ms``; build + factor + solve of
``last_ms``), every call from the same state, the three interleaved so that a drift of the clocks meets all of them alike.
The spread of each (min, max) is recorded beside its median: the covariance query and the iterate run the code they ran before
the reliability query existed, and are to be compared with ``profiles/schur_covariance_timing.json`` within that spread.
Writes one JSON record (default ``profiles/schur_reliability_timing.json``) and prints it.

    python tools/schur_reliability_timing.py [--poses 500] [--landmarks 20000] [--out FILE]
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
    ap.add_argument("--lamda", type=float, default=1e-4, help="damping of the iterate (the queries run at 0)")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schur_reliability_timing.json"))
    a = ap.parse_args()
    from vinsat_amd import synth
    from vinsat_amd.schur import SchurBA, tile_bandwidth_of
    d = synth.make_tracked_landmarks(n_poses=a.poses, n_landmarks=a.landmarks, seed=0)
    st = d["states_gt"].copy()
    st[:, :3] += np.random.default_rng(1).normal(0, 2.0, st[:, :3].shape)
    sb = SchurBA(st, d["X0"], d["uv"], np.full(d["uv"].shape[0], 0.95), d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], sigma_prior=d["sigma"])
    it_ms, parts, c_ms, r_ms = [], [], [], []
    for k in range(a.warmup + a.repeats):
        sb.set_state(st, d["X0"])
        sb.iterate(a.lamda)
        ms = sb.last_ms()
        sb.set_state(st, d["X0"])
        c = sb.covariance(0.0)
        r = sb.reliability(0.0)
        if k >= a.warmup:
            it_ms.append(ms["build"] + ms["factor"] + ms["solve"])
            parts.append(ms)
            c_ms.append(sb.last_covariance_ms())
            r_ms.append(sb.last_reliability_ms())
    med = lambda x: float(np.median(x))
    span = lambda x: [float(min(x)), float(max(x))]
    track = np.bincount(d["landmark_of_row"], minlength=d["X0"].shape[0])
    rec = {"poses": a.poses, "landmarks": int(d["X0"].shape[0]), "rows": int(d["uv"].shape[0]), "reduced_system": 6 * a.poses,
           "blocks": int(sb.structure["blk_i"].size), "row_pairs": int(sb.structure["pair_k"].size), "longest_track": int(track.max()),
           "tile_bandwidth": tile_bandwidth_of(sb.structure), "repeats": a.repeats, "warmup": a.warmup,
           "iterate_ms_median": med(it_ms), "iterate_ms_min_max": span(it_ms),
           "iterate_parts_ms_median": {k: med([p[k] for p in parts]) for k in parts[0]},
           "covariance_ms_median": med(c_ms), "covariance_ms_min_max": span(c_ms),
           "reliability_ms_median": med(r_ms), "reliability_ms_min_max": span(r_ms),
           "row_pass_ms_median": med(np.array(r_ms) - np.array(c_ms)),
           "ratio_reliability_over_covariance": med(r_ms) / med(c_ms),
           "ratio_reliability_over_covariance_min_max": [float(min(r_ms) / max(c_ms)), float(max(r_ms) / min(c_ms))],
           "info": int(r["info"]), "info_covariance": int(c["info"]), "s0sq": r["fit"]["s0sq"], "max_wtest": r["fit"]["max_wtest"]}
    sb.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
