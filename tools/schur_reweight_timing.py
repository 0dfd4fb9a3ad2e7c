#!/usr/bin/env python
"""Time of the free-landmark fit's robust re-weighting (``vba_schur_reweight``) next to the ``build`` part of an LM trial
(``vba_schur_last_ms``) on the same handle.

Two problems: 129 poses / 1300 landmarks (case "129" of tests/schur_cases.py) and 500 poses / 20 000 landmarks / 247 517 rows (the
problem of ``tools/schur_snoop_timing.py``).  Per repeat, from the same state: one re-weighting at
``alpha = 1`` (the power is evaluated), one at ``alpha = 2`` (it is not; the uploaded weights are back), one ``iterate`` at a damping
that rejects nothing of interest (the state is set back after it).  Two warm-ups, then the median of 20 HIP-event intervals of each
(``last_reweight_ms``, ``last_ms()["build"]``); the calls are interleaved so that a drift of the clocks meets all of them alike.
Writes one JSON record (default ``profiles/schur_reweight_timing.json``) and prints it.

    python tools/schur_reweight_timing.py [--repeats 20] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(n_poses, n_landmarks, seed, repeats, warmup):
    from vinsat_amd import synth
    from vinsat_amd.schur import SchurBA
    d = synth.make_tracked_landmarks(n_poses=n_poses, n_landmarks=n_landmarks, seed=seed)
    st = d["states_gt"].copy()
    st[:, :3] += np.random.default_rng(1).normal(0, 2.0, st[:, :3].shape)
    sb = SchurBA(st, d["X0"], d["uv"], np.full(d["uv"].shape[0], 0.95), d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], sigma_prior=d["sigma"])
    one_ms, two_ms, build_ms, c_obs = [], [], [], None
    for k in range(warmup + repeats):
        one = sb.reweight(1.0)
        t1 = sb.last_reweight_ms()
        two = sb.reweight(2.0)
        t2 = sb.last_reweight_ms()
        sb.iterate(1e-3)
        tb = sb.last_ms()["build"]
        sb.set_state(st, d["X0"])
        assert one["status"] == 0 and two["status"] == 0 and one["c_obs"] == two["c_obs"] and (c_obs is None or c_obs == one["c_obs"])
        c_obs = one["c_obs"]
        if k >= warmup:
            one_ms.append(t1)
            two_ms.append(t2)
            build_ms.append(tb)
    sb.close()
    med = lambda x: float(np.median(x))
    span = lambda x: [float(min(x)), float(max(x))]
    return {"poses": n_poses, "landmarks": int(d["X0"].shape[0]), "rows": int(d["uv"].shape[0]), "keys": 2 * int(d["uv"].shape[0]), "c_obs": c_obs,
            "reweight_alpha1_ms_median": med(one_ms), "reweight_alpha1_ms_min_max": span(one_ms),
            "reweight_alpha2_ms_median": med(two_ms), "reweight_alpha2_ms_min_max": span(two_ms),
            "build_ms_median": med(build_ms), "build_ms_min_max": span(build_ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schur_reweight_timing.json"))
    a = ap.parse_args()
    rec = {"repeats": a.repeats, "warmup": a.warmup,
           "problems": [measure(129, 1300, 1, a.repeats, a.warmup), measure(500, 20000, 0, a.repeats, a.warmup)]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
