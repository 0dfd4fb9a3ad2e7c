#!/usr/bin/env python
"""Time of one LM trial of the free-landmark mode with and without the orbit-dynamics factor (``vba_schur_enable_dynamics``):
build / factor / solve of ``vba_schur_last_ms`` on the 500-pose problem that ``bench.py`` builds for the add-on (500 poses, 20 000
landmarks, stride 5 s: the reduced system is 3 000 x 3 000 without the factor and 4 500 x 4 500 with it).

Two handles on the same problem and start; per repeat one ``iterate`` on each at a damping of 1e-3 from the same state (the state is
set back after it), the two handles interleaved so that a drift of the clocks meets both alike.  Two warm-ups, then the median of
20 HIP-event intervals.  Writes one JSON record (default ``profiles/schur_dynamics_timing.json``) and prints it as one line.

    python tools/schur_dynamics_timing.py [--repeats 20] [--sigma-dyn 1e4] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STRIDE, T0 = 5, 10          # synth.make_tracked_landmarks' defaults, as bench.py uses them


def measure(n_poses, n_landmarks, seed, repeats, warmup, sigma_dyn, lamda=1e-3):
    from vinsat_amd import synth
    from vinsat_amd.schur import SchurBA
    d = synth.make_tracked_landmarks(n_poses=n_poses, n_landmarks=n_landmarks, seed=seed, stride=STRIDE, t0=T0)
    st = d["states_gt"].copy()
    st[:, :3] += np.random.default_rng(1).normal(0, 2.0, st[:, :3].shape)
    a = (st, d["X0"], d["uv"], np.full(d["uv"].shape[0], 0.95), d["pose_of_row"], d["landmark_of_row"], d["intrinsics"])
    handles = {"plain": SchurBA(*a, sigma_prior=d["sigma"]),
               "dynamics": SchurBA(*a, sigma_prior=d["sigma"], time_idx=T0 + STRIDE * np.arange(n_poses), sigma_dyn=sigma_dyn)}
    ms = {k: {"build": [], "factor": [], "solve": []} for k in handles}
    trial = {}
    for k in range(warmup + repeats):
        for name, sb in handles.items():
            c0, c1, ok = sb.iterate(lamda)
            t = sb.last_ms()
            sb.set_state(st, d["X0"])
            assert sb.last_info() == 0 and (name not in trial or trial[name] == (c0, c1, ok))
            trial[name] = (c0, c1, ok)
            if k >= warmup:
                for part in t:
                    ms[name][part].append(t[part])
    for sb in handles.values():
        sb.close()
    out = {"poses": n_poses, "landmarks": int(d["X0"].shape[0]), "rows": int(d["uv"].shape[0]), "lamda": lamda, "sigma_dyn": sigma_dyn}
    for name in handles:
        out[name] = {"reduced_system": (9 if name == "dynamics" else 6) * n_poses, "cost_before": trial[name][0], "cost_after": trial[name][1],
                     "accepted": bool(trial[name][2])}
        for part, v in ms[name].items():
            out[name][part + "_ms_median"] = float(np.median(v))
            out[name][part + "_ms_min_max"] = [float(min(v)), float(max(v))]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sigma-dyn", type=float, default=1e4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schur_dynamics_timing.json"))
    a = ap.parse_args()
    rec = {"repeats": a.repeats, "warmup": a.warmup, "problem": measure(500, 20000, 0, a.repeats, a.warmup, a.sigma_dyn)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
