#!/usr/bin/env python
"""Time of the state-covariance query of a handle with the dynamics factor (``vba_schur_covariance_dyn``) next to one
``vba_schur_iterate`` on the same handle, with the selected ``W^T W`` product and with the full one.

The 500-pose / 20 000-landmark problem of ``tools/schur_dynamics_timing.py`` (stride 5 s, the 4 500 x 4 500 reduced system) at
``sigma_dyn = 1e4``: two warm-ups, then the median of 20 HIP-event intervals of each (``last_state_covariance_ms``; build + factor +
solve of ``last_ms``), every call from the same state.  The full product (``VBA_SCHUR_COV_FULL=1``, read when a handle is created)
is measured by a child process of its own running this file with ``--child``.  Writes one JSON record (default
``profiles/schur_covariance_dyn_timing.json``) and prints it as one line.

    python tools/schur_covariance_dyn_timing.py [--repeats 20] [--sigma-dyn 1e4] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STRIDE, T0 = 5, 10          # synth.make_tracked_landmarks' defaults, as bench.py uses them


def measure(n_poses, n_landmarks, repeats, warmup, sigma_dyn, lamda):
    from vinsat_amd import synth
    from vinsat_amd.schur import SchurBA
    d = synth.make_tracked_landmarks(n_poses=n_poses, n_landmarks=n_landmarks, seed=0, stride=STRIDE, t0=T0)
    st = d["states_gt"].copy()
    st[:, :3] += np.random.default_rng(1).normal(0, 2.0, st[:, :3].shape)
    sb = SchurBA(st, d["X0"], d["uv"], np.full(d["uv"].shape[0], 0.95), d["pose_of_row"], d["landmark_of_row"], d["intrinsics"],
                 sigma_prior=d["sigma"], time_idx=T0 + STRIDE * np.arange(n_poses), sigma_dyn=sigma_dyn)
    it_ms, q_ms = [], []
    for k in range(warmup + repeats):
        sb.set_state(st, d["X0"])
        sb.iterate(lamda)
        ms = sb.last_ms()
        sb.set_state(st, d["X0"])
        c = sb.state_covariance(0.0)
        if k >= warmup:
            it_ms.append(ms["build"] + ms["factor"] + ms["solve"])
            q_ms.append(sb.last_state_covariance_ms())
    sb.close()
    med = lambda x: float(np.median(x))
    pos = np.sqrt(np.diagonal(c["state"], axis1=1, axis2=2))
    return {"full_product": bool(int(os.environ.get("VBA_SCHUR_COV_FULL") or 0)), "poses": n_poses, "landmarks": int(d["X0"].shape[0]),
            "rows": int(d["uv"].shape[0]), "reduced_system": 9 * n_poses, "used_tiles_per_side": (9 * n_poses + 63) // 64,
            "iterate_ms_median": med(it_ms), "iterate_ms_min_max": [float(min(it_ms)), float(max(it_ms))],
            "covariance_ms_median": med(q_ms), "covariance_ms_min_max": [float(min(q_ms)), float(max(q_ms))],
            "ratio_query_over_iterate": med(q_ms) / med(it_ms), "info": int(c["info"]),
            "median_sigma_position_km": med(pos[:, :3]), "median_sigma_velocity_km_s": med(pos[:, 6:])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--poses", type=int, default=500)
    ap.add_argument("--landmarks", type=int, default=20000)
    ap.add_argument("--lamda", type=float, default=1e-3, help="damping of the iterate (the query runs at 0)")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sigma-dyn", type=float, default=1e4)
    ap.add_argument("--child", action="store_true", help="measure in this process with the environment as it is; print the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schur_covariance_dyn_timing.json"))
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.poses, a.landmarks, a.repeats, a.warmup, a.sigma_dyn, a.lamda)))
        return
    runs = {}
    for name, full in (("selected", "0"), ("full", "1")):       # a fresh process each: the switch is read when a handle is created
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--poses", str(a.poses), "--landmarks", str(a.landmarks), "--lamda", str(a.lamda),
               "--repeats", str(a.repeats), "--warmup", str(a.warmup), "--sigma-dyn", str(a.sigma_dyn)]
        p = subprocess.run(cmd, env=dict(os.environ, VBA_SCHUR_COV_FULL=full), capture_output=True, text=True, check=True)
        runs[name] = json.loads(p.stdout.strip().splitlines()[-1])
    sel, full = runs["selected"], runs["full"]
    rec = {"repeats": a.repeats, "warmup": a.warmup, "sigma_dyn": a.sigma_dyn, "selected": sel, "full": full,
           "full_over_selected": full["covariance_ms_median"] / sel["covariance_ms_median"],
           "selected_faster_beyond_the_spread": sel["covariance_ms_min_max"][1] < full["covariance_ms_min_max"][0]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
