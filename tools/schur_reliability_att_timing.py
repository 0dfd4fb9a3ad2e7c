#!/usr/bin/env python
"""Time of the reliability query of a handle with the dynamics AND the attitude factor (``vba_schur_reliability_att``) next to the
state-covariance query (``vba_schur_covariance_dyn``) and one ``vba_schur_iterate`` on the same handle.

The 500-pose / 20 000-landmark problem of ``tools/schur_reliability_dyn_timing.py`` (stride 5 s, the 4 500 x 4 500 reduced system) at
``sigma_dyn = 1e4``, ``sigma_att = 5e5``, the gap rotations those of the true attitudes: the three calls interleaved on one handle,
every call from the same state; two warm-ups, then the median of 20 HIP-event intervals of each (``last_attitude_reliability_ms``,
``last_state_covariance_ms``; build + factor + solve of ``last_ms``) with the range.  The query costs what the covariance query costs
plus the row pass and the two edge passes: the record holds the ratio of the two medians of this run.  Writes one JSON record (default
``profiles/schur_reliability_att_timing.json``) and prints it as one line.

    python tools/schur_reliability_att_timing.py [--repeats 20] [--sigma-dyn 1e4] [--sigma-att 5e5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STRIDE, T0 = 5, 10          # synth.make_tracked_landmarks' defaults, as bench.py uses them


def qmul(p, q):
    """Hamilton product, scalar last, row by row."""
    pv, pw, qv, qw = p[:, :3], p[:, 3:], q[:, :3], q[:, 3:]
    return np.concatenate([pw * qv + qw * pv + np.cross(pv, qv), pw * qw - (pv * qv).sum(1, keepdims=True)], 1)


def gap_rotations(q):
    """``cumrot[i] = conj(q_i) (x) q_{i+1}``, the last row the identity (it is ignored)."""
    c = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (q.shape[0], 1))
    c[:-1] = qmul(q[:-1] * np.array([-1.0, -1.0, -1.0, 1.0]), q[1:])
    return c / np.linalg.norm(c, axis=1, keepdims=True)


def measure(n_poses, n_landmarks, repeats, warmup, sigma_dyn, sigma_att, lamda):
    from vinsat_amd import synth
    from vinsat_amd.schur import SchurBA
    d = synth.make_tracked_landmarks(n_poses=n_poses, n_landmarks=n_landmarks, seed=0, stride=STRIDE, t0=T0)
    st = d["states_gt"].copy()
    st[:, :3] += np.random.default_rng(1).normal(0, 2.0, st[:, :3].shape)
    sb = SchurBA(st, d["X0"], d["uv"], np.full(d["uv"].shape[0], 0.95), d["pose_of_row"], d["landmark_of_row"], d["intrinsics"],
                 sigma_prior=d["sigma"], time_idx=T0 + STRIDE * np.arange(n_poses), sigma_dyn=sigma_dyn,
                 cumrot=gap_rotations(d["states_gt"][:, 3:7]), sigma_att=sigma_att)
    it_ms, cov_ms, rel_ms = [], [], []
    for k in range(warmup + repeats):
        sb.set_state(st, d["X0"])
        rel = sb.attitude_reliability(0.0)
        sb.state_covariance(0.0)
        sb.iterate(lamda)
        ms = sb.last_ms()
        if k >= warmup:
            rel_ms.append(sb.last_attitude_reliability_ms())
            cov_ms.append(sb.last_state_covariance_ms())
            it_ms.append(ms["build"] + ms["factor"] + ms["solve"])
    sb.close()
    med = lambda x: float(np.median(x))
    span = lambda x: [float(min(x)), float(max(x))]
    fit = rel["fit"]
    return {"repeats": repeats, "warmup": warmup, "sigma_dyn": sigma_dyn, "sigma_att": sigma_att, "poses": n_poses,
            "landmarks": int(d["X0"].shape[0]), "rows": int(d["uv"].shape[0]), "reduced_system": 9 * n_poses,
            "iterate_ms_median": med(it_ms), "iterate_ms_min_max": span(it_ms),
            "covariance_ms_median": med(cov_ms), "covariance_ms_min_max": span(cov_ms),
            "reliability_ms_median": med(rel_ms), "reliability_ms_min_max": span(rel_ms),
            "ratio_reliability_over_covariance": med(rel_ms) / med(cov_ms), "ratio_reliability_over_iterate": med(rel_ms) / med(it_ms),
            "info": int(rel["info"]), "rho": fit["rho"], "t_edges": fit["t_edges"], "t_att": fit["t_att"], "max_att_wtest": fit["max_att_wtest"],
            "edges": n_poses - 1,
            "identity_minus_unknowns": fit["t_rows"] + fit["t_prior"] + fit["t_edges"] + fit["t_att"] - (9 * n_poses + 3 * int(d["X0"].shape[0]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=500)
    ap.add_argument("--landmarks", type=int, default=20000)
    ap.add_argument("--lamda", type=float, default=1e-3, help="damping of the iterate (the queries run at 0)")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sigma-dyn", type=float, default=1e4)
    ap.add_argument("--sigma-att", type=float, default=5e5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schur_reliability_att_timing.json"))
    a = ap.parse_args()
    rec = measure(a.poses, a.landmarks, a.repeats, a.warmup, a.sigma_dyn, a.sigma_att, a.lamda)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
