"""The entry of a chained schedule on a one-window latency-mode handle: vba_set_states only stages the states, the first kernel
of the pass (inside the schedule's graph) takes them, clears the unconsumed warm histogram and resets the call counters, and a
schedule that finds the handle's generation unchanged replays its graph without rebuilding a view.  None of that may move a bit:
every case compares with a handle that launches kernel by kernel, steps call by call, or is fresh.

Two small windows: the C1 fixture (10 poses, 200 rows: one chunk, one accumulate block) and a random window of 43 poses
(tests/random_windows.py, seed 2: several chunks, more than one accumulate block, a pose without rows, shuffled rows)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden, golden_inputs
import random_windows

pytestmark = pytest.mark.gpu

ITERS = list(range(20))
INITS = [k < 10 for k in range(20)]         # 10 landmark-only + 10 full calls


def _c1():
    g = load_golden("c1")
    inp = golden_inputs(g)
    return dict(inp, st0=g["states0"][0].copy())


def _rnd():
    win, xyz, uv, ii, conf, t, st0 = random_windows.make(2)
    assert t.size >= 33
    return dict(xyz=xyz, uv=uv, ii=ii, conf=conf, K=win.intrinsics, cumrot=win.cumrot_last, time_idx=t, st0=st0)


def _rej():
    g = load_golden("rej")
    return dict(golden_inputs(g), st0=g["states0"][0].copy(), iters=[int(x) for x in g["iters"]], inits=[bool(x) for x in g["initialize"]],
                n_trials=[int(x) for x in g["n_trials"]])


WINDOWS = {"c1": _c1, "rnd43": _rnd}


@pytest.fixture(scope="module", params=sorted(WINDOWS))
def win(request):
    return WINDOWS[request.param]()


def _engine(w, graph=True, time_idx=None):
    from vinsat_amd.engine import BAEngine
    n, m = w["K"].shape[0], w["xyz"].shape[0]
    e = BAEngine(n, m)
    assert e.mode()[0] == 1                 # latency mode: the handle stages
    if not graph:
        e.set_schedule_graph(False)
    e.upload_observations(w["xyz"], w["uv"], w["conf"], w["ii"], n)
    e.upload_window(w["K"], w["cumrot"], w["time_idx"] if time_idx is None else time_idx)
    return e


def _run(e, st, lam=1e-4, iters=ITERS, inits=INITS):
    e.set_states(st, lam)
    trials = e.run_schedule(iters, inits)
    return e.get_states() + (trials,)


def _same(a, b, what=None):
    """states, damping, last Hessian, trial count of the last call, flags, trials of the schedule: bit for bit"""
    assert np.array_equal(a[0], b[0]), what
    assert a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3:] == b[3:], (what, a[1], b[1], a[3:], b[3:])


def _perturbed(st0, k):
    return st0 + 1e-6 * np.random.default_rng(100 + k).standard_normal(st0.shape)


def test_replayed_entry_has_the_bits_of_kernel_by_kernel_launches(win):
    """First capture, replay, an odd-length schedule, then capture and replay on the other parity -- after every schedule the
    handle holds what a handle with the graph switched off holds."""
    a, b = _engine(win), _engine(win, graph=False)
    plan = [(ITERS, INITS), (ITERS, INITS), (ITERS[:7], INITS[:7]), (ITERS, INITS), (ITERS, INITS)]
    for k, (its, ins) in enumerate(plan):
        _same(_run(a, win["st0"], iters=its, inits=ins), _run(b, win["st0"], iters=its, inits=ins), k)
    assert a.schedule_graph_stats() == (3, 2) and b.schedule_graph_stats() == (0, 0)
    a.close()
    b.close()


def test_every_schedule_starts_from_the_states_it_was_given(win):
    """Five schedules from five different initial states on one handle (one capture, four replays reading the staging buffer
    afresh): each ends where a fresh handle given the same states ends."""
    a = _engine(win)
    for k in range(5):
        st = _perturbed(win["st0"], k)
        got = _run(a, st, lam=1e-4 * (k + 1))
        f = _engine(win)
        _same(got, _run(f, st, lam=1e-4 * (k + 1)), k)
        f.close()
    assert a.schedule_graph_stats() == (1, 4)
    a.close()


def test_set_states_has_read_the_callers_array_when_it_returns(win):
    a, b = _engine(win), _engine(win)
    want = _run(b, win["st0"])
    for rep in range(2):        # (captured, replayed)
        st = win["st0"].copy()
        a.set_states(st, 1e-4)
        st[:] = np.nan
        trials = a.run_schedule(ITERS, INITS)
        _same(a.get_states() + (trials,), want, rep)
    a.close()
    b.close()


def test_the_second_of_two_set_states_wins(win):
    a, b = _engine(win), _engine(win)
    want = _run(b, win["st0"], lam=1e-3)
    for rep in range(2):
        a.set_states(_perturbed(win["st0"], 9), 1e-4)
        _same(_run(a, win["st0"], lam=1e-3), want, rep)
    a.close()
    b.close()


def test_get_states_right_after_set_states_returns_what_was_set(win):
    a = _engine(win)
    for k in range(2):
        st = _perturbed(win["st0"], k)
        a.set_states(st, 0.25 * (k + 1))
        got = a.get_states()
        assert np.array_equal(got[0], st) and got[1] == 0.25 * (k + 1)
        # ... and a schedule behind the read-back starts from them all the same
        trials = a.run_schedule(ITERS, INITS)
        f = _engine(win)
        _same(a.get_states() + (trials,), _run(f, st, lam=0.25 * (k + 1)), k)
        f.close()
    a.close()


def test_a_changed_handle_is_not_served_a_stale_graph(win):
    """Between otherwise identical schedules: the window re-uploaded with one time index moved (a gap of more than 64 s: a long
    edge, i.e. other launches), the other integrator, another lane count of the accumulation (vba_set_option).  Each time the
    handle must end where a fresh handle configured the same way ends, on a newly captured graph; with the setting restored it
    must be back on the original bits."""
    t_long = np.array(win["time_idx"], dtype=np.int64).copy()
    t_long[t_long.size // 2:] += 100
    changes = [
        (lambda e: e.upload_window(win["K"], win["cumrot"], t_long), lambda e: e.upload_window(win["K"], win["cumrot"], win["time_idx"]),
         lambda: _engine(win, time_idx=t_long)),
        (lambda e: e.set_integrator(1), lambda e: e.set_integrator(0), lambda: _engine(win)),
        (lambda e: e.set_accumulate_lanes(16), lambda e: e.set_accumulate_lanes(0), lambda: _engine(win)),
    ]
    a = _engine(win)
    base = _run(a, win["st0"])
    _same(_run(a, win["st0"]), base, "replay")
    for k, (change, restore, fresh) in enumerate(changes):
        captures = a.schedule_graph_stats()[0]
        change(a)
        got = _run(a, win["st0"])
        assert a.schedule_graph_stats()[0] == captures + 1, k
        f = fresh()
        if k:
            change(f)
        want = _run(f, win["st0"])
        f.close()
        _same(got, want, k)
        _same(_run(a, win["st0"]), want, (k, "replay"))
        restore(a)
        # the handle's generation has moved, but the views it yields are those of the base graph again: found by key and view
        # bytes (no capture), which refreshes the graph's identity -- the schedule after it is matched by identity alone
        captures, replays = a.schedule_graph_stats()
        _same(_run(a, win["st0"]), base, (k, "restored"))
        assert a.schedule_graph_stats() == (captures, replays + 1), (k, "restored")
        _same(_run(a, win["st0"]), base, (k, "restored, replay"))
        assert a.schedule_graph_stats() == (captures, replays + 2), (k, "restored, replay")
    a.close()


def test_the_ninth_schedule_evicts_the_least_recently_used_graph(win):
    """A handle keeps eight graphs, most recently used first, and a ninth evicts the one at the back.  Even-length prefixes of the
    driver's schedule (the call parity stays 0, and parity is part of a graph's identity); after every schedule the handle
    holds what a handle with the graph switched off holds."""
    a, b = _engine(win), _engine(win, graph=False)

    def run(ncalls, want):
        _same(_run(a, win["st0"], iters=ITERS[:ncalls], inits=INITS[:ncalls]),
              _run(b, win["st0"], iters=ITERS[:ncalls], inits=INITS[:ncalls]), (ncalls, want))
        assert a.schedule_graph_stats() == want, (ncalls, want)

    for k, ncalls in enumerate(range(20, 2, -2)):       # nine graphs: the last one evicts the 20-call graph
        run(ncalls, (k + 1, 0))
    for k, ncalls in enumerate(range(18, 2, -2)):       # the other eight are there; the 18-call graph is now the least recently used
        run(ncalls, (9, k + 1))
    run(20, (10, 8))                                    # captured again, evicts the 18-call graph
    run(18, (11, 8))                                    # ... which evicts the 16-call graph, used right after it
    run(16, (12, 8))                                    # ... which evicts the 14-call graph
    run(20, (12, 9))                                    # still there
    assert b.schedule_graph_stats() == (0, 0)
    a.close()
    b.close()


@pytest.mark.parametrize("step", [1, 2, 3], ids=["end-capture", "instantiate", "first-launch"])
def test_a_failed_capture_uploads_the_staged_states_exactly_once(step):
    """VBA_GRAPH_FAIL_INJECT (read once per process: a child process): the pass whose capture failed is enqueued again for real,
    entry kernel included -- the bits of a handle that never tries a graph, for two schedules from different states."""
    code = (
        "import numpy as np, sys\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests')\n"
        "import test_gpu_schedule_entry as T\n"
        "for name in sorted(T.WINDOWS):\n"
        "    w = T.WINDOWS[name]()\n"
        "    a, b = T._engine(w), T._engine(w, graph=False)\n"
        "    for k in range(2):\n"
        "        st = T._perturbed(w['st0'], k)\n"
        "        T._same(T._run(a, st), T._run(b, st), (name, k))\n"
        "    assert a.schedule_graph_stats() == (0, 0), a.schedule_graph_stats()\n"
        "    a.close(); b.close()\n"
        "print('fallback ok')\n" % (ROOT, ROOT))
    env = dict(os.environ, VBA_GRAPH_FAIL_INJECT=str(step))
    p = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "fallback ok" in p.stdout, p.stderr[-2000:]


def test_a_schedule_that_stalls_has_the_bits_of_call_by_call_steps():
    """The window of the REJ fixture rejects trials (up to nine per call): the host finishes the stalled calls and re-issues the
    chain from a later call, without the entry kernel -- on the captured pass and on the replayed one."""
    w = _rej()
    assert max(w["n_trials"]) >= 3          # the window does reject trials
    b = _engine(w)
    b.set_states(w["st0"], 1e-4)
    for k, (it, init) in enumerate(zip(w["iters"], w["inits"])):
        b.step(it, init)
        assert b.get_states()[3] == w["n_trials"][k], k
    want = b.get_states()
    b.close()
    a = _engine(w)
    for rep in range(2):
        _same(_run(a, w["st0"], iters=w["iters"], inits=w["inits"])[:5], want, rep)
    assert a.schedule_graph_stats() == (1, 1)
    a.close()
