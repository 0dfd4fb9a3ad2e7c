#!/usr/bin/env python
"""Time of one LM trial of the free-landmark mode on a handle with the dynamics and the attitude factor, with and without a state
prior on every pose (``vba_schur_enable_state_prior``), and of the window hand-off (``vba_schur_handoff``) at 935 steps beside the
state-covariance query of the same handle: the 500-pose problem that ``bench.py`` builds for the add-on (500 poses, 20 000 landmarks,
stride 5 s; the reduced system is 4 500 x 4 500 either way; the prior adds 500 blocks to the build, two kernels, and one kernel to each
of the two cost evaluations, which lie outside the three intervals).

Two handles on the same problem and start (2 km in position, 2e-3 in attitude off the truth); per repeat one ``iterate`` on each at a
damping of 1e-3 from the same state (the state is set back after it), the two handles interleaved so that a drift of the clocks meets
both alike; then, interleaved too, ``state_covariance(0)`` and ``handoff(935, ...)`` on the handle without the prior.  Two warm-ups,
then the median of 20 HIP-event intervals.  Writes one JSON record (default ``profiles/schur_prior_timing.json``) and prints it as one
line.  Figures as measured: no target.

    python tools/schur_prior_timing.py [--repeats 20] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STRIDE, T0 = 5, 10          # synth.make_tracked_landmarks' defaults, as bench.py uses them
SIGMAS = np.repeat(np.array([0.1, 1e-3, 1e-4]), 3)      # km, rad, km/s: the priors of tests/schur_prior_cases.py
HANDOFF_STEPS = 935


def measure(n_poses, n_landmarks, seed, repeats, warmup, sigma_dyn, sigma_att, lamda=1e-3):
    from vinsat_amd import quat, synth
    from vinsat_amd.schur import SchurBA
    d = synth.make_tracked_landmarks(n_poses=n_poses, n_landmarks=n_landmarks, seed=seed, stride=STRIDE, t0=T0)
    gt = d["states_gt"]
    rng = np.random.default_rng(1)
    st = gt.copy()
    st[:, :3] += rng.normal(0, 2.0, st[:, :3].shape)
    dq = np.concatenate([rng.normal(0, 2e-3, (n_poses, 3)), np.ones((n_poses, 1))], 1)
    st[:, 3:7] = quat.qmul(st[:, 3:7], dq / np.linalg.norm(dq, axis=1, keepdims=True))
    cumrot = np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (n_poses, 1))
    cumrot[:-1] = quat.qmul(gt[:-1, 3:7] * np.array([-1.0, -1.0, -1.0, 1.0]), gt[1:, 3:7])
    M = np.eye(9) + 0.3 * rng.normal(0, 1, (n_poses, 9, 9))
    infos = M @ np.swapaxes(M, 1, 2) / (SIGMAS[:, None] * SIGMAS[None, :])
    infos = (infos + np.swapaxes(infos, 1, 2)) / 2
    prior = (np.arange(n_poses, dtype=np.int32), gt.copy(), infos)
    a = (st, d["X0"], d["uv"], np.full(d["uv"].shape[0], 0.95), d["pose_of_row"], d["landmark_of_row"], d["intrinsics"])
    kw = dict(sigma_prior=d["sigma"], time_idx=T0 + STRIDE * np.arange(n_poses), sigma_dyn=sigma_dyn, cumrot=cumrot, sigma_att=sigma_att)
    handles = {"attitude": SchurBA(*a, **kw), "prior": SchurBA(*a, **kw, state_prior=prior)}
    ms = {k: {"build": [], "factor": [], "solve": [], "trial_cost": []} for k in handles}
    trial = {}
    for k in range(warmup + repeats):
        for name, sb in handles.items():
            c0, c1, ok = sb.iterate(lamda)
            t = dict(sb.last_ms(), trial_cost=sb.last_trial_cost_ms())
            sb.set_state(st, d["X0"])
            assert sb.last_info() == 0 and (name not in trial or trial[name] == (c0, c1, ok))
            trial[name] = (c0, c1, ok)
            if k >= warmup:
                for part in t:
                    ms[name][part].append(t[part])
    sb = handles["attitude"]
    q = {"state_covariance": [], "handoff": []}
    for k in range(warmup + repeats):
        assert sb.state_covariance(0.0)["info"] == 0
        t_cov = sb.last_state_covariance_ms()
        assert sb.handoff(HANDOFF_STEPS, cumrot[0], (1e-8, 1e-12, 1e-14))["status"] == 0
        if k >= warmup:
            q["state_covariance"].append(t_cov)
            q["handoff"].append(sb.last_handoff_ms())
    for h in handles.values():
        h.close()
    out = {"poses": n_poses, "landmarks": int(d["X0"].shape[0]), "rows": int(d["uv"].shape[0]), "lamda": lamda, "sigma_dyn": sigma_dyn,
           "sigma_att": sigma_att, "priors": n_poses, "handoff_steps": HANDOFF_STEPS}
    for name in handles:
        out[name] = {"reduced_system": 9 * n_poses, "cost_before": trial[name][0], "cost_after": trial[name][1], "accepted": bool(trial[name][2])}
        for part, v in ms[name].items():
            out[name][part + "_ms_median"] = float(np.median(v))
            out[name][part + "_ms_min_max"] = [float(min(v)), float(max(v))]
    for name, v in q.items():
        out[name + "_ms_median"] = float(np.median(v))
        out[name + "_ms_min_max"] = [float(min(v)), float(max(v))]
    out["handoff_minus_state_covariance_ms"] = out["handoff_ms_median"] - out["state_covariance_ms_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sigma-dyn", type=float, default=1e4)
    ap.add_argument("--sigma-att", type=float, default=5e5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schur_prior_timing.json"))
    a = ap.parse_args()
    rec = {"repeats": a.repeats, "warmup": a.warmup, "problem": measure(500, 20000, 0, a.repeats, a.warmup, a.sigma_dyn, a.sigma_att)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
