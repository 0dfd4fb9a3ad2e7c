#!/usr/bin/env python3
"""Where the host spends the time between two chained schedules of the C3 window (500 poses, 50 000 rows): needs a library built
with -DVBA_ENTRY_STAMPS (vba_context.h), selected through VBA_LIB.  Walks the benchmark's loop -- set_states + the 20-call
schedule -- and prints the mean of every interval of the entry cycle over the timed schedules, the wall clock per schedule
beside them.  argv[1]: schedules (default 200)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from ctypes import byref, c_int64
from vinsat_amd import od_pipe, synth, _lib
from vinsat_amd.engine import BAEngine, _p

INTERVALS = ["GPU work of the schedule + wait (graph launched -> wait of read_heads returned)",
             "back in the caller (wait returned -> vba_set_states entered)",
             "vba_set_states (entry -> exit)",
             "caller between the two (vba_set_states exit -> vba_run_schedule entry)",
             "vba_run_schedule up to the launch (entry -> just before hipGraphLaunch)",
             "hipGraphLaunch (before -> after)"]


def fetch(e):
    out = np.empty(12)
    cnt = c_int64()
    _lib.check(e.lib.vba_debug_fetch(e.h, 0, 103, _p(out), out.size, byref(cnt)), e.lib)
    return out.reshape(6, 2)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    win = od_pipe.prepare_window(*synth.make_sequence("C3"))
    st0 = od_pipe.initial_guess(win)
    n, m = win.time_idx.size, win.ii.size
    e = BAEngine(n, m)
    e.upload_observations(win.landmarks_xyz, win.landmarks_uv, win.confidences, win.ii, n)
    e.upload_window(win.intrinsics, win.cumrot_last, win.time_idx)
    iters, inits = list(range(20)), [k < 10 for k in range(20)]

    def schedules(k):
        for _ in range(k):
            e.set_states(st0, 1e-4)
            e.run_schedule(iters, inits)
    schedules(5)
    fetch(e)                    # (clears the sums of the warm-up)
    t0 = time.perf_counter()
    schedules(reps)
    wall = (time.perf_counter() - t0) / reps
    got = fetch(e)
    print(f"C3 window, {reps} schedules of 20 calls: {1e6 * wall:.1f} us per schedule wall clock ({1e6 * wall / 20:.2f} us per call)")
    idle = 0.0
    for k, name in enumerate(INTERVALS):
        cnt, ns = got[k]
        mean = ns / cnt / 1e3 if cnt else float("nan")
        if k:
            idle += mean
        print(f"  {mean:9.2f} us  x{int(cnt):4d}  {name}")
    print(f"  {idle:9.2f} us  host time per schedule with nothing of the next schedule launched yet (intervals 2 .. 6)")
    e.close()


if __name__ == "__main__":
    main()
