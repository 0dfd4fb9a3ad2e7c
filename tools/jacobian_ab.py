#!/usr/bin/env python3
"""fp64 against fp32 Jacobians (VBA_OPT_JACOBIAN_F32) on the chained 20-call schedule (vba_run_schedule): C3 with W = 1, 256 and
4096 windows per handle, C5 with one.  Per case and mode: it/s (window-calls per second, host clock around synchronised
schedules, the two modes alternated rep by rep on one handle), the class times of the chain (VBA_OPT_CHAIN_PROFILE, a run of
its own) and the difference of the final states between the modes (position / velocity max-rel, attitude angle in rad).
usage: tools/jacobian_ab.py [reps] [case ...]   (cases: c3w1 c3w256 c3w4096 c5w1)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vinsat_amd import od_pipe, synth  # noqa: E402
from vinsat_amd.engine import BAEngine  # noqa: E402

CASES = dict(c3w1=("C3", 1), c3w256=("C3", 256), c3w4096=("C3", 4096), c5w1=("C5", 1))


def state_diff(a, b):
    pos = np.abs(a[:, :3] - b[:, :3]).max() / np.abs(b[:, :3]).max()
    vel = np.abs(a[:, 7:] - b[:, 7:]).max() / np.abs(b[:, 7:]).max()
    q = a[:, 3:7] / np.linalg.norm(a[:, 3:7], axis=1, keepdims=True)
    r = b[:, 3:7] / np.linalg.norm(b[:, 3:7], axis=1, keepdims=True)
    w1, v1, w2, v2 = q[:, 3], -q[:, :3], r[:, 3], r[:, :3]
    w = w1 * w2 - (v1 * v2).sum(1)
    v = w1[:, None] * v2 + w2[:, None] * v1 + np.cross(v1, v2)
    return float(pos), float(vel), float((2 * np.arctan2(np.linalg.norm(v, axis=1), np.abs(w))).max())


def run_case(name, reps):
    cfg, W = CASES[name]
    win = od_pipe.prepare_window(*synth.make_sequence(cfg))
    st0 = od_pipe.initial_guess(win)
    n, m = win.time_idx.size, win.ii.size
    e = BAEngine(n, m, windows=W)
    for w in range(W):
        e.upload_observations(win.landmarks_xyz, win.landmarks_uv, win.confidences, win.ii, n, window=w)
        e.upload_window(win.intrinsics, win.cumrot_last, win.time_idx, window=w)
    iters, inits = list(range(20)), [k < 10 for k in range(20)]

    def schedule(f32):
        e.set_jacobian_f32(f32)
        e.set_states(st0, 1e-4, window=-1)
        e.run_schedule(iters, inits)
        return e.get_states(window=0)[0]       # (a device-to-host copy: the schedule has finished)

    out, secs = {}, {False: [], True: []}
    for f32 in (False, True):       # warm-up: code objects, graph capture of each mode
        out[f32] = schedule(f32)
    for _ in range(reps):
        for f32 in (False, True):
            t0 = time.perf_counter()
            schedule(f32)
            secs[f32].append(time.perf_counter() - t0)
    prof = {}
    e.set_chain_profile(True)
    for f32 in (False, True):
        e.chain_profile(reset=True)
        schedule(f32)
        prof[f32] = {k: round(v[0] * 1e3, 3) for k, v in e.chain_profile(reset=True).items()}     # us per interval
    e.set_chain_profile(False)
    e.close()
    res = dict(case=name, config=cfg, windows=W, reps=reps, state_diff_pos_vel_att=state_diff(out[True], out[False]))
    for f32 in (False, True):
        tag = "fp32" if f32 else "fp64"
        best = min(secs[f32])
        res[tag] = dict(it_per_s=round(20 * W / best), it_per_s_median=round(20 * W / float(np.median(secs[f32]))),
                        class_us=prof[f32])
    res["speedup"] = round(res["fp32"]["it_per_s"] / res["fp64"]["it_per_s"], 4)
    return res


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    names = sys.argv[2:] or list(CASES)
    for name in names:
        print(json.dumps(run_case(name, reps)), flush=True)


if __name__ == "__main__":
    main()
