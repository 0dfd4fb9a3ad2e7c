#!/usr/bin/env python
"""Time of one LM trial of the free-landmark mode with the dynamics factor ACROSS LONG GAPS (``vba_schur_enable_dynamics_long``):
the edges of more than 64 s propagated parallel in time against the same edges on the serial lanes (``VBA_SCHUR_LONG_SERIAL=1``, read
when the factor is enabled).  build / factor / solve of ``vba_schur_last_ms`` and the trial's cost of
``vba_schur_last_trial_cost_ms``, on

  two-pass   the pose times of the second batch of ``synth.make_two_pass_sequence`` (25 poses, gaps of 935 s and 510 s) with tracked
             landmarks
  ten-gaps   100 poses 5 s apart with ten gaps of 200 .. 1000 s between them

Two handles on the same problem and start; per repeat one ``iterate`` on each at a damping of 1e-3 from the same state (set back
after it: every repeat walks its chains anew, nothing is carried), the two handles interleaved so that a drift of the clocks meets
both alike.  Two warm-ups, then the median of 20 HIP-event intervals.  Writes one JSON record (default
``profiles/schur_dynamics_long_timing.json``) and prints it as one line.

    python tools/schur_dynamics_long_timing.py [--repeats 20] [--sigma-dyn 1e4] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARTS = ("build", "factor", "solve", "trial_cost")


def two_pass_times():
    from vinsat_amd import od_pipe, synth
    return np.asarray(od_pipe.prepare_window(*synth.make_two_pass_sequence()).time_idx, dtype=np.int64)


def ten_gap_times():
    gaps = np.full(99, 5, dtype=np.int64)
    gaps[9::9][:10] = np.linspace(200, 1000, 10).astype(np.int64)
    return 10 + np.concatenate([[0], np.cumsum(gaps)])


def measure(times, n_landmarks, seed, repeats, warmup, sigma_dyn, lamda=1e-3):
    from vinsat_amd import synth
    from vinsat_amd.schur import SchurBA
    d = synth.make_tracked_landmarks(n_landmarks=n_landmarks, seed=seed, times=times)
    st = d["states_gt"].copy()
    st[:, :3] += np.random.default_rng(1).normal(0, 2.0, st[:, :3].shape)
    a = (st, d["X0"], d["uv"], np.full(d["uv"].shape[0], 0.95), d["pose_of_row"], d["landmark_of_row"], d["intrinsics"])
    kw = dict(sigma_prior=d["sigma"], time_idx=times, sigma_dyn=sigma_dyn, long_gaps=True)
    handles = {"parallel": SchurBA(*a, **kw)}
    os.environ["VBA_SCHUR_LONG_SERIAL"] = "1"
    try:
        handles["serial"] = SchurBA(*a, **kw)
    finally:
        del os.environ["VBA_SCHUR_LONG_SERIAL"]
    long_edges = [int(i) for i in handles["parallel"].long_edges()]
    assert handles["serial"].long_edges().size == 0
    ms = {k: {p: [] for p in PARTS} for k in handles}
    trial = {}
    for k in range(warmup + repeats):
        for name, sb in handles.items():
            c0, c1, ok = sb.iterate(lamda)
            t = dict(sb.last_ms(), trial_cost=sb.last_trial_cost_ms())
            sb.set_state(st, d["X0"])
            assert sb.last_info() == 0 and (name not in trial or trial[name] == (c0, c1, ok))
            trial[name] = (c0, c1, ok)
            if k >= warmup:
                for part in PARTS:
                    ms[name][part].append(t[part])
    for sb in handles.values():
        sb.close()
    gaps = np.diff(times)
    out = {"poses": int(times.size), "landmarks": int(d["X0"].shape[0]), "rows": int(d["uv"].shape[0]), "lamda": lamda, "sigma_dyn": sigma_dyn,
           "long_edges": long_edges, "long_gaps_s": [int(gaps[i]) for i in long_edges]}
    for name in handles:
        out[name] = {"cost_before": trial[name][0], "cost_after": trial[name][1], "accepted": bool(trial[name][2])}
        for part, v in ms[name].items():
            out[name][part + "_ms_median"] = float(np.median(v))
            out[name][part + "_ms_min_max"] = [float(min(v)), float(max(v))]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sigma-dyn", type=float, default=1e4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "schur_dynamics_long_timing.json"))
    a = ap.parse_args()
    rec = {"repeats": a.repeats, "warmup": a.warmup,
           "two_pass": measure(two_pass_times(), 500, 0, a.repeats, a.warmup, a.sigma_dyn),
           "ten_gaps": measure(ten_gap_times(), 2000, 0, a.repeats, a.warmup, a.sigma_dyn)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
