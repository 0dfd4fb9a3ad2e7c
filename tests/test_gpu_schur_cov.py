"""``vba_schur_covariance`` / ``SchurBA.covariance`` on the GPU against the CPU reference of tests/schur_cov_cases.py.

Bars: ``max(100 x floor of the case, 1e-11)`` relative to the largest entry of the family (pose / pairs / landmark); the floor is
the disagreement of the reference's two NumPy routes (tests/test_schur_cov_host.py holds it below 1e-10 everywhere but in the
clamp case).  Every figure is printed before it is asserted.  Shapes: "12" is one panel; "43" two panels with 254 padding rows
(three tiles of nothing but padding, and 58 padding rows inside the last used tile); "128" three panels without padding; "129"
four; "wide" has tile bandwidth 12 of 12, so k_trinv_step skips nothing (the synthetic tracks alone give 2).

Device against reference, measured on an MI355X: see DESIGN section 9.
"""
import ctypes

import numpy as np
import pytest

import schur_cases as C
import schur_cov_cases as V

pytestmark = pytest.mark.gpu


def _open(name, d=None):
    from vinsat_amd.schur import SchurBA
    d = V.case(name) if d is None else d
    e = SchurBA(d["states0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], sigma_prior=d["sigma"])
    e.set_state(d["states0"], d["Xs"])
    return d, e


def _matches(e, name, lam, label=""):
    r = V.reference(name, lam)
    c = e.covariance(lam, pairs=True)
    assert c["info"] == 0
    bi, bj, blocks = c["pairs"]
    assert np.array_equal(bi, r.blk_i) and np.array_equal(bj, r.blk_j)
    got = dict(pose=c["pose"], pairs=blocks, landmark=c["landmark"])
    fig = {k: V.rel(got[k], getattr(r, k)) for k in V.FAMILIES}
    print(f"FIGURES cov {name} {label} lam={lam:g} " + " ".join(f"{k}={fig[k]:.2e} (floor {r.floor[k]:.1e}, bar {V.bar(r, k):.1e})" for k in V.FAMILIES))
    for k in V.FAMILIES:
        assert np.all(np.isfinite(got[k]))
        assert fig[k] <= V.bar(r, k), k
    return c, r


def test_one_panel_matches_the_reference():
    d, e = _open("12")
    assert C.padded_shape(12)[2] == 1
    for lam in (0.0, 1e-3):
        _matches(e, "12", lam)
    assert e.last_covariance_ms() > 0.0
    e.close()


@pytest.mark.parametrize("name,lam,panels", [("43", 1e-3, 2), ("43", 0.0, 2), ("128", 1e-3, 3), ("129", 1e-3, 4), ("wide", 1e-3, 4)])
def test_multi_panel_matches_the_reference(name, lam, panels):
    d, e = _open(name)
    N, Npad, p = C.padded_shape(d["states0"].shape[0])
    assert p == panels and C.kernel_constants() == (64, 4)
    bw, nbu = C.tile_bandwidth(e.structure), (N + 63) // 64
    if name == "wide":
        assert bw == nbu - 1 == 12                  # nothing skipped
    else:
        assert bw == 2 < nbu - 1                    # most products of the triangular inverse skipped
    if name == "43":
        assert Npad - N == 254 and Npad // 64 - nbu == 3 and N % 64 == 2        # whole padding tiles, and a padded tail in the last used one
    if name == "128":
        assert Npad == N
    _matches(e, name, lam)
    e.close()


def test_pose_without_rows_is_held_by_the_damping_alone():
    d, e = _open("pose_without_rows")
    lam, i = 1e-3, d["empty_pose"]
    c, r = _matches(e, "pose_without_rows", lam)
    err = np.abs(c["pose"][i] - np.eye(6) / lam).max() / np.abs(r.pose).max()
    print("FIGURES empty pose against I / lam", err)
    assert err <= V.bar(r, "pose")
    e.close()


@pytest.mark.parametrize("lam", [0.0, 1e-3])
def test_unobserved_landmarks_keep_their_prior_bitwise(lam):
    d, e = _open("more_landmarks_than_rows")
    c, _ = _matches(e, "more_landmarks_than_rows", lam)
    closed = 1.0 / (1.0 / (d["sigma"] * d["sigma"]) + lam)         # the rounding order include/vinsat_ba.h states
    u = d["unobserved"]
    assert u.size > 200
    assert np.array_equal(c["landmark"][u], np.broadcast_to(closed * np.eye(3), (u.size, 3, 3)))
    e.close()


def test_more_poses_than_landmarks():
    d, e = _open("more_poses_than_landmarks")
    assert d["X0"].shape[0] == 8 < d["states0"].shape[0]
    _matches(e, "more_poses_than_landmarks", 1e-3)
    e.close()


def test_landmarks_behind_the_camera():
    d, e = _open("behind_the_camera")
    _matches(e, "behind_the_camera", 1e4)
    e.close()


@pytest.mark.parametrize("mode", ["1", "2"])
def test_comparison_factorisations_serve_the_query(mode, monkeypatch):
    monkeypatch.setenv("VBA_SCHUR_CLASSIC", mode)                   # read in vba_schur_create
    d, e = _open("129")
    _matches(e, "129", 1e-3, label=f"classic={mode}")
    e.close()


def _raw(e, lam, pose=True, pairs=True, lm=True):
    """The C entry itself: (rc, info, pose, pairs, landmark), outputs not asked for are None (NULL)."""
    from vinsat_amd._lib import PD
    nblk = e.structure["blk_i"].size
    bufs = [np.full(s, 7.0) if on else None for s, on in (((e.n, 6, 6), pose), ((nblk, 6, 6), pairs), ((e.L, 3, 3), lm))]
    info = ctypes.c_int(-1)
    rc = e.lib.vba_schur_covariance(e.h, float(lam), *[b.ctypes.data_as(PD) if b is not None else None for b in bufs], ctypes.byref(info))
    return (rc, info.value, *bufs)


@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_failed_factorisation_gives_nan_and_the_row(mode, monkeypatch):
    _, row, _ = C.late_failure_reference()
    monkeypatch.setenv("VBA_SCHUR_CLASSIC", mode)
    d, e = _open("late_failure")
    rc, info, pose, pairs, lm = _raw(e, 0.0)
    print(f"FIGURES cov late_failure classic={mode} info={info} expected={row + 1}")
    assert rc == 0 and info == row + 1 == 595
    assert np.all(np.isnan(pose)) and np.all(np.isnan(pairs)) and np.all(np.isnan(lm))
    assert e.last_info() == 0                       # the handle's own record belongs to its iterates
    e.iterate(0.0)
    assert e.last_info() == info
    from vinsat_amd._lib import VbaError
    with pytest.raises(VbaError, match=f"row {row}"):
        e.covariance(0.0)
    c = e.covariance(0.0, pairs=True, strict=False)
    assert c["info"] == info and np.all(np.isnan(c["pose"])) and np.all(np.isnan(c["landmark"])) and np.all(np.isnan(c["pairs"][2]))
    e.close()


def _snapshot(e):
    st, X = e.get_state()
    dc, dl = e.last_step()
    ms = e.last_ms()
    return [st, X, dc.copy(), dl.copy(), e.cholesky_factor(), np.array([e.last_info(), ms["build"], ms["factor"], ms["solve"]])]


def test_query_changes_nothing_the_handle_shows():
    d, e = _open("43")
    e.iterate(1e-3)
    before = _snapshot(e)
    e.covariance(0.0, pairs=True)
    e.covariance(1e-2)
    after = _snapshot(e)
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    e.close()


def test_iterates_return_the_same_bits_with_queries_between_them():
    d, e = _open("43")
    _, f = _open("43")
    runs = []
    for eng, ask in ((e, True), (f, False)):
        out = []
        for lam in (1e-3, 1e-4, 1e-5):
            if ask:
                eng.covariance(0.0)
            out.append(eng.iterate(lam))
            if ask:
                eng.covariance(lam, pairs=True)
        runs.append((out, *eng.get_state()))
    assert runs[0][0] == runs[1][0] and any(ok for _, _, ok in runs[0][0])
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
    e.close()
    f.close()


def test_queries_repeat_bit_for_bit_on_one_handle_and_across_handles():
    d, e = _open("43")
    _, f = _open("43")
    a, b, c = e.covariance(0.0, pairs=True), e.covariance(0.0, pairs=True), f.covariance(0.0, pairs=True)
    e.covariance(1e-3)                              # (another damping through the same scratch in between)
    g = e.covariance(0.0, pairs=True)
    for o in (b, c, g):
        assert np.array_equal(a["pose"], o["pose"]) and np.array_equal(a["landmark"], o["landmark"]) and np.array_equal(a["pairs"][2], o["pairs"][2])
    e.close()
    f.close()


def test_null_outputs_in_every_combination():
    d, e = _open("12")
    full = _raw(e, 1e-3)
    assert full[0] == 0 and full[1] == 0
    for mask in range(8):
        on = [bool(mask & 1), bool(mask & 2), bool(mask & 4)]
        rc, info, *bufs = _raw(e, 1e-3, *on)
        assert rc == 0 and info == 0
        for k in range(3):
            assert (bufs[k] is None) == (not on[k])
            if on[k]:
                assert np.array_equal(bufs[k], full[2 + k])
    e.close()


def test_argument_and_state_errors():
    from vinsat_amd._lib import PD, load
    lib = load()
    d, e = _open("12")
    info = ctypes.c_int()
    assert lib.vba_schur_covariance(None, 0.0, None, None, None, ctypes.byref(info)) == 1           # VBA_EINVAL
    assert lib.vba_schur_covariance(e.h, 0.0, None, None, None, None) == 1
    assert lib.vba_schur_covariance(e.h, -1.0, None, None, None, ctypes.byref(info)) == 1
    assert lib.vba_schur_covariance(e.h, float("nan"), None, None, None, ctypes.byref(info)) == 1
    assert lib.vba_schur_last_covariance_ms(None, None) == 1
    # before upload / before a state
    s = e.structure
    h = ctypes.c_void_p()
    assert lib.vba_schur_create(0, e.n, e.m, e.L, int(s["blk_i"].size), int(s["pair_k"].size), ctypes.byref(h)) == 0
    rc = lib.vba_schur_covariance(h, 0.0, None, None, None, ctypes.byref(info))
    assert rc != 0 and rc == lib.vba_schur_iterate(h, 0.0, ctypes.byref(ctypes.c_double()), ctypes.byref(ctypes.c_double()), ctypes.byref(ctypes.c_int()))
    lib.vba_schur_destroy(h)
    e.close()


def test_orderings_and_symmetry_from_the_device():
    d, e = _open("43")
    c, r = _matches(e, "43", 0.0)
    m = V.definiteness(c["pose"], c["landmark"], r)
    print("FIGURES orderings from the device " + " ".join(f"{k}={v:.2e}" for k, v in m.items()))
    assert m["below_prior"] >= -1e-9 and m["above_conditional"] >= -1e-9 and m["pose_above_frozen"] >= -1e-9
    assert np.array_equal(c["pose"], np.swapaxes(c["pose"], 1, 2)) and np.array_equal(c["landmark"], np.swapaxes(c["landmark"], 1, 2))
    bi, bj, blocks = c["pairs"]
    dg = bi == bj
    assert np.array_equal(bi[dg], np.arange(e.n)) and np.array_equal(blocks[dg], c["pose"])
    e.close()


def test_landmarks_come_back_in_the_callers_order_and_sigma_helpers():
    from vinsat_amd import schur
    d = V.case("12")
    L = d["X0"].shape[0]
    perm = np.random.default_rng(3).permutation(L)             # new id of landmark l: perm[l]
    p = dict(d)
    p["landmark_of_row"] = perm[d["landmark_of_row"]]
    p["X0"] = np.empty_like(d["X0"])
    p["X0"][perm] = d["X0"]
    p["Xs"] = p["X0"]
    _, e = _open("12", p)
    r = V.reference("12", 0.0)
    c = e.covariance(0.0)
    fig = V.rel(c["landmark"][perm], r.landmark), V.rel(c["pose"], r.pose)
    print("FIGURES permuted landmarks", fig)
    assert fig[0] <= V.bar(r, "landmark") and fig[1] <= V.bar(r, "pose")
    pos, att = schur.pose_sigmas(c)
    dgp = np.diagonal(r.pose, axis1=1, axis2=2)
    assert V.rel(pos, np.sqrt(dgp[:, :3])) <= V.bar(r, "pose") * np.abs(r.pose).max() / dgp[:, :3].min()
    assert V.rel(att, 2.0 * np.sqrt(dgp[:, 3:])) <= V.bar(r, "pose") * np.abs(r.pose).max() / dgp[:, 3:].min()
    dgl = np.diagonal(r.landmark, axis1=1, axis2=2)
    assert V.rel(schur.landmark_sigmas(c)[perm], np.sqrt(dgl)) <= V.bar(r, "landmark") * np.abs(r.landmark).max() / dgl.min()
    e.close()
