"""The free-landmark Schur add-on is PARITY UNPINNED (the reference has no such mode): these tests check this repository's
own CPU restatement against itself -- the eliminated system gives the step of the full one, the step descends, LM converges
back to the truth from a perturbed start -- and the host-side index structure the GPU kernels trust."""
import numpy as np
import pytest

import schur_cases as C
from oracle import schur_oracle as S
from vinsat_amd import synth
from vinsat_amd.schur import build_structure


@pytest.fixture(scope="module")
def prob():
    d = synth.make_tracked_landmarks(n_poses=12, n_landmarks=150, seed=1)
    rng = np.random.default_rng(2)
    st = d["states_gt"].copy()
    st[:, :3] += rng.normal(0, 2.0, (st.shape[0], 3))
    dq = np.concatenate([rng.normal(0, 2e-3, (st.shape[0], 3)), np.ones((st.shape[0], 1))], 1)
    from oracle import ba_oracle as O
    st[:, 3:7] = O.qmul(st[:, 3:7], dq / np.linalg.norm(dq, axis=1, keepdims=True))
    d["states0"] = st
    d["w"] = np.full(d["uv"].shape[0], 0.95)
    return d


def test_schur_step_equals_the_step_of_the_full_system(prob):
    d = prob
    B, C, E, v, wl = S.normal_equations(d["states0"], d["X0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"],
                                        d["intrinsics"], d["sigma"], 1e-3)
    dc_f, dl_f = S.step_full(B, C, E, v, wl)
    dc_s, dl_s, Sm, Lc = S.step_schur(B, C, E, v, wl)
    assert np.abs(dc_s - dc_f).max() / np.abs(dc_f).max() < 1e-8
    assert np.abs(dl_s - dl_f).max() / np.abs(dl_f).max() < 1e-8
    assert np.allclose(Lc @ Lc.T, Sm, rtol=0, atol=1e-9 * np.abs(Sm).max())
    assert np.linalg.eigvalsh(Sm).min() > 0


def test_lm_on_the_oracle_recovers_poses_and_landmarks(prob):
    d = prob
    st, X, lam = d["states0"], d["X0"].copy(), 1e-4
    costs = []
    for _ in range(12):
        c0, c1, ok, st, X, _, _ = S.lm_trial(st, X, d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"],
                                             d["sigma"], lam)
        costs.append(c0)
        lam = lam * 0.1 if ok else lam * 10
    # the minimum is at least as good as the truth itself (1 px noise), from a start 2 km / 2 mrad off; convergence is linear
    # because the reference's rotation Jacobian carries a factor 2 against its retraction, kept as is
    at_truth = S.cost(d["states_gt"], d["X_true"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], d["sigma"])
    assert costs[-1] < at_truth < 1e-2 * costs[0]
    # (along-track position and pitch are nearly interchangeable for a nadir camera without a dynamics factor: the pose
    # error itself is not the test) -- freeing the landmarks moves them towards the truth, away from the noisy catalogue
    assert np.linalg.norm(X - d["X_true"]) < 0.9 * np.linalg.norm(d["X0"] - d["X_true"])


def test_index_structure_covers_every_pair_once(prob):
    for name in ("base", "wide", "pose_without_rows", "more_landmarks_than_rows"):
        _check_index_structure(prob if name == "base" else C.case(name), name)
    with pytest.raises(ValueError):
        build_structure(np.array([0, 0]), np.array([1, 1]), 2, 2)      # one landmark twice from one pose


def _check_index_structure(d, name):
    n, L = d["states_gt"].shape[0], d["X0"].shape[0]
    order, s = build_structure(d["pose_of_row"], d["landmark_of_row"], n, L)
    rp, rl = d["pose_of_row"][order], d["landmark_of_row"][order]
    assert np.array_equal(s["row_pose"], rp) and np.array_equal(s["row_lm"], rl)
    assert np.all(np.diff(rl) >= 0) and s["lm_ptr"][-1] == rp.size and s["pose_ptr"][-1] == rp.size
    assert np.array_equal(np.sort(s["pose_rows"]), np.arange(rp.size))
    assert np.all(np.diff(rp[s["pose_rows"]]) >= 0)
    # blocks: unique, lower triangle, all diagonal blocks present; pairs of a block belong to it and share a landmark
    key = s["blk_i"].astype(np.int64) * n + s["blk_j"]
    assert np.all(np.diff(key) > 0) and np.all(s["blk_j"] <= s["blk_i"])
    assert set(range(n)) <= set(s["blk_i"][s["blk_i"] == s["blk_j"]].tolist())
    for b in range(s["blk_i"].size):
        k, k2 = s["pair_k"][s["blk_ptr"][b]:s["blk_ptr"][b + 1]], s["pair_k2"][s["blk_ptr"][b]:s["blk_ptr"][b + 1]]
        assert np.all(rp[k] == s["blk_i"][b]) and np.all(rp[k2] == s["blk_j"][b]) and np.all(rl[k] == rl[k2])
    # every unordered pair of rows of a landmark (and every row with itself) appears exactly once
    cnt = np.diff(s["lm_ptr"]).astype(np.int64)
    assert s["pair_k"].size == int((cnt * (cnt + 1) // 2).sum())
    # ... by brute force: the pair list of every block is exactly the set of row pairs that share a landmark
    want = C.pairs_by_brute_force(rp, rl, L)
    for b in range(s["blk_i"].size):
        lo, hi = s["blk_ptr"][b], s["blk_ptr"][b + 1]
        got = list(zip(s["pair_k"][lo:hi].tolist(), s["pair_k2"][lo:hi].tolist()))
        assert len(got) == len(set(got)) and set(got) == want.pop((int(s["blk_i"][b]), int(s["blk_j"][b])), set())
    assert not want
    # CSR of the rows of a landmark / of a pose: exactly the rows that name it (empty for a pose without rows, for an unobserved landmark)
    assert np.array_equal(np.diff(s["lm_ptr"]), np.bincount(rl, minlength=L)) and np.array_equal(np.diff(s["pose_ptr"]), np.bincount(rp, minlength=n))
    if name == "pose_without_rows":
        i = d["empty_pose"]
        assert s["pose_ptr"][i] == s["pose_ptr"][i + 1] and not np.any((s["blk_i"] == i) ^ (s["blk_j"] == i))
    if name == "more_landmarks_than_rows":
        assert L > rp.size and np.all(np.diff(s["lm_ptr"])[d["unobserved"]] == 0)
    if name == "wide":
        assert C.tile_bandwidth(s) == (6 * n + 63) // 64 - 1


FLOOR_CASES = [(n, lam) for n in C.NARROW for lam in (1e-3, 1e-6)] + [("wide", 1e-3)] + [(n, 1e-3) for n in C.EDGES[:3]] + [(C.EDGES[3], 1e4)]


@pytest.mark.parametrize("name,lam", FLOOR_CASES)
def test_the_two_routes_agree_on_every_problem_of_the_gpu_tests(name, lam):
    """The noise floor of the reference the GPU tests compare with (bars 1e-7 on dc and dl): its two routes agree to a tenth of
    the bar on every problem, at the damping used there.  On the narrow-band problems the factor keeps the band exactly."""
    r = C.reference(name, lam, True)
    print(f"FLOOR {name} lam={lam:g} dc={r.floor_dc:.2e} dl={r.floor_dl:.2e}")
    assert r.floor_dc < 1e-8 and r.floor_dl < 1e-8
    assert np.linalg.eigvalsh(r.Sm).min() > 0
    if name in C.NARROW:
        bw = C.tile_bandwidth(C.structure(C.case(name)))
        skipped, zero = C.tiles_beyond_band_are_zero(r.Lc, bw)
        assert bw == 2 and skipped > 0 and zero


def test_clamped_rows_are_clamped_and_a_minor_part_of_the_cost():
    from oracle import ba_oracle as O
    d = C.case("behind_the_camera")
    k = d["clamped_rows"]
    ii, X = d["pose_of_row"][k], d["Xs"][d["landmark_of_row"][k]]
    # behind the camera: the projection is the clamped one and does not depend on the depth
    est = O.landmark_project(d["states0"], X, d["intrinsics"], ii, jacobian=False)
    q = d["states0"][ii, 3:7]
    axis = O.rotation_matrix(q / np.linalg.norm(q, axis=1, keepdims=True))[:, :, 2]
    assert np.all(np.einsum("kj,kj->k", X - d["states0"][ii, :3], axis) < -0.9)
    assert np.abs(O.landmark_project(d["states0"], X - 0.5 * axis, d["intrinsics"], ii, jacobian=False) - est).max() < 1e-6
    keep = np.ones(d["uv"].shape[0], dtype=bool)
    keep[k] = False
    others = S.cost(d["states0"], d["Xs"], d["X0"], d["uv"][keep], d["w"][keep], d["pose_of_row"][keep], d["landmark_of_row"][keep],
                    d["intrinsics"], d["sigma"])
    c0 = C.reference("behind_the_camera", 1e4, True).c0
    assert 0 < c0 - others < 0.5 * c0


def test_late_failure_is_unambiguous():
    """The case behind tests/test_schur_gpu.py::test_last_info_tells_the_first_failing_row: the first bad pivot is in the
    third panel, at the first row of the first pose with negative weights, and no rounding decides it.

    The margin first proposed for this -- every pivot further than 1e-6 max|diag S| from zero -- cannot hold for this geometry
    at lam = 0, with any seed: the rotation diagonals are 1.4e10 .. 3.5e10 (a 500 km lever arm, squared) and the position
    pivots 1e2 .. 1e3, which is 3e-3 .. 1e-2 of that margin; the failing pivot is -0.04 .. -0.1 of it (seeds 1 .. 5).  What is
    asserted instead: a symmetric perturbation of S by 1e-9 of every entry -- a hundred times the 1e-11 to which the device's
    Lg Lg^T agrees with the oracle's S wherever the two can be compared -- moves no pivot up to the failing one by 1 % and
    leaves the failing row where it is; and the failing pivot is larger in size than the smallest pivot before it."""
    Sm, row, piv = C.late_failure_reference()
    assert 512 <= row < 768 and row == 6 * (129 - 30)
    assert piv[-1] < 0 and abs(piv[-1]) > piv[:-1].min() > 0
    rng = np.random.default_rng(0)
    for _ in range(3):
        P = np.tril(rng.uniform(-1e-9, 1e-9, Sm.shape))
        row2, piv2 = C.first_bad_pivot(Sm * (1.0 + P + np.tril(P, -1).T))
        assert row2 == row and np.all(np.abs(piv2 / piv - 1.0) < 1e-2)
