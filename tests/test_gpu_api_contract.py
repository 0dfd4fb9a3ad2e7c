"""What the C ABI promises around the compute calls, pinned entry point by entry point: which arguments vba_create_mode refuses, that a
handle works at the shapes where the layout of its device arena rounds differently, what the setters reject and that a rejection
leaves the handle as it was, that states come back as they went up, that a new window forgets the old one, and the sizes and
refusals of vba_debug_fetch.  Every refused call is refused on the host.

(The argument checks of vba_create_mode that need no GPU, and the null-handle checks of the setters, are in test_cabi_symbols.py.)"""
import ctypes

import numpy as np
import pytest

from vinsat_amd import _lib, od_pipe, synth
from vinsat_amd._lib import VbaError
from vinsat_amd.engine import DBG, BAEngine

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 4


def _raises(code):
    return pytest.raises(VbaError, match=rf"error {code}:")


def _window(n, m, seed=0):
    """A synthetic window of n poses cut down to exactly m rows (every pose keeps most of its rows), and start states off the truth."""
    per = -(-m // n) + 2
    win = od_pipe.prepare_window(*synth.make_sequence(synth.WindowConfig("api", n, per, 5), seed=seed))
    assert win.ii.size >= m
    keep = np.sort(np.random.default_rng(seed).permutation(win.ii.size)[:m])
    st = win.states_gt.copy()
    st[:, :3] += 0.5
    return dict(n=n, m=m, xyz=win.landmarks_xyz[keep], uv=win.landmarks_uv[keep], conf=win.confidences[keep], ii=win.ii[keep],
                K=win.intrinsics, cumrot=win.cumrot_last, t=win.time_idx, st=st)


def _upload(eng, w, window=0):
    eng.upload_observations(w["xyz"], w["uv"], w["conf"], w["ii"], w["n"], window=window)
    eng.upload_window(w["K"], w["cumrot"], w["t"], window=window)


def _oracle_args(w):
    return (w["cumrot"], w["uv"], w["xyz"], w["ii"], w["t"], w["K"], w["conf"])


@pytest.fixture(scope="module")
def win8():
    return _window(8, 300)


@pytest.fixture()
def eng8(win8):
    e = BAEngine(8, 300)
    _upload(e, win8)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------ 1. arguments that need a device
def test_create_refuses_a_device_index_out_of_range():
    lib = _lib.load()
    cnt = ctypes.c_int()
    assert lib.vba_device_count(ctypes.byref(cnt)) == 0 and cnt.value >= 1
    for device in (-1, cnt.value):
        h = ctypes.c_void_p(1)
        assert lib.vba_create_mode(device, 1, 8, 300, -1, ctypes.byref(h)) == EINVAL, device
        assert not h.value
        assert b"device index" in lib.vba_last_error()


# ------------------------------------------------------------------------------------------------ 2. shapes at the layout's edges
class _SteppedWindow:
    """Window w of a batched handle behind the iterate() of a one-window engine, which is what test_gpu_parity._oracle_vs_gpu drives:
    the states go up, the handle steps (every window), the window's result comes back."""

    def __init__(self, eng, w):
        self.eng, self.w = eng, w

    def iterate(self, it, init, lam, st):
        self.eng.set_states(st, lam, window=self.w)
        self.eng.step(it, init)
        return self.eng.get_states(self.w)


# (W, n_max, m_max, mode, [(n, m) per window]): the smallest shapes at which m_pad, obs_stride, the observation and pose-chain block
# counts and the odd (n_max + 2) / 2 term of the observation block each round differently.  (The API's minimum, n_max = 2, is
# test_gpu_parity.py::test_minimum_window_two_poses_one_observation_each.)
SHAPES = [(1, 8, 300, 1, [(8, 300)]),
          (1, 8, 300, 0, [(8, 300)]),
          (3, 8, 300, -1, [(5, 187), (8, 300), (6, 225)]),
          (1, 33, 257, 1, [(33, 257)])]


@pytest.mark.parametrize("W,n_max,m_max,mode,sizes", SHAPES, ids=[f"W{s[0]}-n{s[1]}-m{s[2]}-mode{s[3]}" for s in SHAPES])
def test_one_call_at_the_edges_of_the_arena_layout(W, n_max, m_max, mode, sizes):
    from test_gpu_parity import _oracle_vs_gpu
    wins = [_window(n, m, seed=k) for k, (n, m) in enumerate(sizes)]
    eng = BAEngine(n_max, m_max, windows=W, mode=mode)
    assert eng.mode()[0] == (1 if mode != 0 else 0)
    for k, w in enumerate(wins):
        _upload(eng, w, window=k)
        eng.set_states(w["st"], 1e-3, window=k)
    for k, w in enumerate(wins):
        _oracle_vs_gpu(_SteppedWindow(eng, k), _oracle_args(w), 12, False, 1e-3, w["st"], tol=1e-7)
        for j, v in enumerate(wins):        # (the step moved every window: back to the start for the next one)
            eng.set_states(v["st"], 1e-3, window=j)
    eng.close()


# ------------------------------------------------------------------------------------------------ 3. buckets follow the mode
def test_bucket_presence_follows_the_mode():
    lat, bw = BAEngine(8, 300, mode=1), BAEngine(8, 300, mode=0)
    lat.set_bucket_cap(0)
    with _raises(ESTATE):
        bw.set_bucket_cap(0)
    lat.close()
    bw.close()


# ------------------------------------------------------------------------------------------------ 4. rejected option values
REJECTED = [("accumulate_lanes", 3), ("trial_tiles", 3), ("fusion", 128), ("chunk_waves", 3), ("warm_shift", 41), ("bucket_cap", 7),
            ("jacobian_f32", 2)]


def _schedule_bits(eng, w):
    eng.set_states(w["st"], 1e-4)
    eng.run_schedule([0, 1, 10], [True, True, False])
    return eng.get_states()


def test_rejected_option_values(eng8, win8):
    lib = eng8.lib
    for name, value in REJECTED:
        assert lib.vba_set_option(eng8.h, _lib.OPT[name], value) == EINVAL, name
    assert lib.vba_set_option(eng8.h, 999, 0) == EINVAL


def test_rejected_solver_values(eng8):
    lib = eng8.lib
    assert lib.vba_set_solver(eng8.h, 1) == EINVAL
    assert lib.vba_set_solver(eng8.h, 61) == EINVAL
    assert lib.vba_set_solver2(eng8.h, 8, 1) == EINVAL


def test_a_handle_that_rejected_values_computes_what_a_fresh_one_does(eng8, win8):
    """Every rejection above but those of vba_set_solver: that one has cleared the second-level chunk size by the time it looks at
    its argument, so a handle whose default is cyclic reduction solves with one level after it (same results to rounding, other bits)."""
    lib = eng8.lib
    for name, value in REJECTED:
        assert lib.vba_set_option(eng8.h, _lib.OPT[name], value) == EINVAL, name
    assert lib.vba_set_option(eng8.h, 999, 0) == EINVAL
    assert lib.vba_set_solver2(eng8.h, 8, 1) == EINVAL
    got = _schedule_bits(eng8, win8)
    fresh = BAEngine(8, 300)
    _upload(fresh, win8)
    ref = _schedule_bits(fresh, win8)
    fresh.close()
    assert np.array_equal(got[0], ref[0]) and got[1] == ref[1] and np.array_equal(got[2], ref[2]) and got[3:] == ref[3:]


# ------------------------------------------------------------------------------------------------ 5. states round trip
def test_states_round_trip_on_a_batched_handle():
    sizes = [(5, 187), (8, 300), (6, 225)]
    wins = [_window(n, m, seed=k) for k, (n, m) in enumerate(sizes)]
    eng = BAEngine(8, 300, windows=3)
    with _raises(ESTATE):
        eng.get_states(0)                       # nothing uploaded, no states
    for k, w in enumerate(wins):
        _upload(eng, w, window=k)
    with _raises(ESTATE):
        eng.get_states(1)                       # a window, but no states yet
    with _raises(EINVAL):
        eng.set_states(wins[0]["st"], 1e-3, window=-1)      # one set of states for all: needs equal pose counts
    for k, w in enumerate(wins):
        eng.set_states(w["st"], 1e-3 * (k + 1), window=k)
    for k, w in enumerate(wins):
        st, lam = eng.get_states(k)[:2]
        assert st.tobytes() == w["st"].tobytes() and lam == 1e-3 * (k + 1), k
    rng = np.random.default_rng(0)
    all_in, lam_in = rng.standard_normal((3, 8, 10)), np.array([1e-2, 2e-2, 3e-2])
    eng.set_states_all(all_in, lam_in)
    all_out, lam_out = eng.get_states_all()[:2]
    assert all_out.tobytes() == all_in.tobytes() and np.array_equal(lam_out, lam_in)
    eng.close()


def test_states_round_trip_through_the_staged_path(eng8, win8):
    """One window in latency mode: vba_set_states only stages the states in mapped host memory; vba_get_states right behind it makes
    them go up first (flush_states)."""
    assert eng8.mode()[0] == 1
    eng8.set_states(win8["st"], 3e-3)
    st, lam = eng8.get_states()[:2]
    assert st.tobytes() == win8["st"].tobytes() and lam == 3e-3


# ------------------------------------------------------------------------------------------------ 6. a new window forgets the old one
def test_a_new_window_forgets_the_old_one(eng8, win8):
    eng8.set_states(win8["st"], 1e-3)
    eng8.step(12, False)
    w5 = _window(5, 187, seed=1)
    eng8.upload_observations(w5["xyz"], w5["uv"], w5["conf"], w5["ii"], 5)
    with _raises(ESTATE) as e:
        eng8.step(12, False)
    assert "window 0 is missing observations, pose constants or states" in str(e.value)


def test_upload_refusals(win8):
    eng, w = BAEngine(8, 300), win8
    with _raises(ESTATE):
        eng.upload_prior(w["st"], np.zeros((8, 6, 6)))       # before any upload
    t = w["t"].copy()
    t[4] = t[3]
    with _raises(EINVAL):
        eng.upload_window(w["K"], w["cumrot"], t)
    ii = w["ii"].copy()
    ii[17] = 8
    with _raises(EINVAL) as e:
        eng.upload_observations(w["xyz"], w["uv"], w["conf"], ii, 8)
    assert "ii[17]" in str(e.value)
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. debug fetch
def _fetch(eng, what, capacity):
    out = np.empty(max(capacity, 1))
    cnt = ctypes.c_int64(-1)
    rc = eng.lib.vba_debug_fetch(eng.h, 0, what, out.ctypes.data_as(_lib.PD), capacity, ctypes.byref(cnt))
    return rc, cnt.value


def test_debug_fetch_sizes_and_refusals(eng8, win8):
    n, m = 8, 300
    assert _fetch(eng8, DBG["scalars"], 8)[0] == ESTATE          # no step has run
    eng8.set_states(win8["st"], 1e-3)
    eng8.step(12, False)
    sizes = dict(est=2 * m, weight=m, Jg=12 * m, H=36 * n, b=6 * n, Phi=36 * n, r_pred=7 * (n - 1), qgrad=3 * n, Hq=27 * n,
                 bands=243 * n, rhs=9 * n, dpose=9 * n, scalars=8,
                 # what the trial left for the next call: 2 observation tiles, 1 pose-chain block, 64 slots of long edges behind a
                 # header of 8; a warm histogram behind a header of 4; 2048 buckets of 256 keys behind their capacity
                 next_keys=2 * m, next_hist=4 + 2048, next_buckets=1 + 2048 * 256, part_trial=8 + 2 + 1 + 64, part_next=2)
    assert sorted(sizes) == sorted(DBG)
    for name, size in sizes.items():
        assert _fetch(eng8, DBG[name], size - 1)[0] == EINVAL, name
        assert b"debug buffer too small" in eng8.lib.vba_last_error(), name
        assert _fetch(eng8, DBG[name], size) == (0, size), name
    assert _fetch(eng8, 99, 4096)[0] == EINVAL
    assert b"unknown debug selector" in eng8.lib.vba_last_error()


def test_debug_fetch_refuses_what_was_not_carried(win8):
    """The selectors of what a trial leaves for the next call: refused with VBA_ESTATE and a message on a handle without bin buckets,
    behind a call that emitted nothing or an exponent histogram, and once the states were replaced; part_trial is always there."""
    big = 1 + 2048 * 256
    carried = ("next_keys", "next_hist", "next_buckets", "part_next")

    def stepped(mode=-1, **options):
        e = BAEngine(8, 300, mode=mode)
        _upload(e, win8)
        for k, v in options.items():
            getattr(e, f"set_{k}")(v)
        e.set_states(win8["st"], 1e-3)
        e.step(12, False)
        return e

    e = stepped(mode=0)                             # bandwidth mode: keys and a warm histogram, no buckets
    assert _fetch(e, DBG["next_buckets"], big)[0] == ESTATE and b"no bin buckets" in e.lib.vba_last_error()
    for name in ("next_keys", "next_hist", "part_next", "part_trial"):
        assert _fetch(e, DBG[name], big)[0] == 0, name
    e.close()
    e = stepped(key_carry=False)                    # nothing emitted
    for name in carried:
        assert _fetch(e, DBG[name], big)[0] == ESTATE and b"carried nothing" in e.lib.vba_last_error(), name
    assert _fetch(e, DBG["part_trial"], big)[0] == 0
    e.close()
    e = stepped(warm_select=False)                  # the exponent histogram: 1024 bins, no buckets behind it
    assert _fetch(e, DBG["next_hist"], big) == (0, 4 + 1024)
    assert _fetch(e, DBG["next_buckets"], big)[0] == ESTATE and b"exponent histogram" in e.lib.vba_last_error()
    e.close()
    e = stepped()
    assert _fetch(e, DBG["next_keys"], big)[0] == 0
    e.set_states(win8["st"], 1e-3)                  # the keys on the device belong to states that are gone
    for name in carried:
        assert _fetch(e, DBG[name], big)[0] == ESTATE and b"carried nothing" in e.lib.vba_last_error(), name
    e.close()


def test_debug_fetch_refuses_after_a_pipelined_call(eng8, win8):
    eng8.iterate(0, True, 1e-4, win8["st"])
    eng8.iterate_resident(1, True)
    assert _fetch(eng8, DBG["rhs"], 9 * 8)[0] == ESTATE
    assert b"pipelined" in eng8.lib.vba_last_error()
