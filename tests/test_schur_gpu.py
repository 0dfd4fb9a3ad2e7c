"""Free-landmark Schur add-on on the GPU against this repository's own CPU restatement (oracle/schur_oracle.py).
PARITY UNPINNED: the reference keeps its landmarks fixed and has no counterpart of this mode.

Shapes (``Npad`` is ``N = 6 n`` rounded up to whole panels of ``kPanel * kT = 256`` columns).  The first two tests below run
one panel only (12, 23, 40 poses: ``Npad = 256``), where the panel loop leaves before its first trailing update.  The tests
from ``test_multi_panel_trial...`` on reach the rest of ``vba_schur_iterate``:

  43 / 450    N = 258 -> 512    2 panels: one k_syrk_panel launch of grid (2, 2), nothing on the second stream, 254 padding rows
  128 / 1300  N = 768 -> 768    3 panels, no padding (k_pad_identity not launched), one bulk update on the second stream
  129 / 1300  N = 774 -> 1024   4 panels, two successive bulk updates, a 250-row identity tail in the last panel
  "wide"      129 / 1300 + 20 rows from the last ten poses to landmarks of the first ten: tile bandwidth 12 = all 13 used tiles
              (the synthetic tracks alone give bandwidth 2, where k_trsv_step skips most tiles)

Bars (relative to the largest entry of the reference, unchanged from the one-panel tests): c0 1e-10, c1 1e-7, dc / dl 1e-7,
Lg Lg^T against S 1e-11, Lg 1e-8, states 1e-9, X 1e-10.  Noise floor of the reference = disagreement of the oracle's own two
routes (step_full against step_schur), measured on the CPU (tests/test_schur_oracle.py asserts each below a tenth of the bar):

  case                          lam    floor dc   floor dl
  43 / 450                      1e-3   8.9e-10    3.3e-10
  43 / 450                      1e-6   5.0e-10    1.6e-10
  128 / 1300                    1e-3   1.1e-09    2.5e-10
  128 / 1300                    1e-6   2.1e-09    6.5e-10
  129 / 1300                    1e-3   2.0e-09    4.1e-10
  129 / 1300                    1e-6   2.4e-09    3.2e-10
  wide                          1e-3   2.7e-09    2.6e-10
  pose_without_rows             1e-3   6.5e-10    2.9e-10
  more_landmarks_than_rows      1e-3   1.1e-11    4.0e-12
  more_poses_than_landmarks     1e-3   7.0e-09    2.9e-10
  behind_the_camera             1e+4   2.3e-10    2.5e-09

behind_the_camera runs at lam = 1e4, not 1e-3: a clamped row has a Jacobian of 4e4 px / km (depth clamped to 0.1 km), its
landmark block is 1.5e9 against a prior of 400, and forming S = B - E C^-1 E^T cancels those nine digits.  At lam = 1e-3 .. 1e3
the Schur ROUTE of the oracle itself is then 1e-8 .. 6e-8 (dc) and 1e-7 .. 1e-6 (dl) from an iteratively refined solution of
the full system, whatever the seed (the full route stays at 1e-11 / 1e-9): above a tenth of the bar, so the damping was
raised until the floor is under it.  The clamped blocks (1.5e9) still dominate lam there.

Device against oracle, measured on an MI355X (worst over the cases of a row; default factorisation unless named):

  case                          lam    c1        dc        dl        states    X         Lg Lg^T   Lg
  43 / 450                      1e-3   7.3e-11   1.2e-09   3.9e-10   1.1e-12   6.8e-15   7.2e-16   2.5e-14
  43 / 450                      1e-6   7.3e-11   6.4e-10   2.1e-10   6.1e-13   3.5e-15   7.2e-16   2.8e-14
  128 / 1300                    1e-3   2.9e-11   1.1e-09   2.5e-10   9.7e-13   4.7e-15   8.9e-16   2.9e-14
  128 / 1300                    1e-6   1.1e-10   2.1e-09   6.5e-10   1.9e-12   1.2e-14   7.6e-16   2.9e-14
  129 / 1300                    1e-3   5.5e-11   1.2e-09   2.6e-10   1.0e-12   5.2e-15   9.1e-16   3.9e-14
  129 / 1300                    1e-6   1.8e-12   2.6e-09   2.7e-10   2.3e-12   5.5e-15   7.8e-16   3.4e-14
  129 / 1300, classic 1 and 2   1e-3   5.5e-11   1.2e-09   2.6e-10   1.0e-12   5.2e-15   1.3e-15   3.2e-14
  wide                          1e-3   2.6e-11   1.6e-09   2.9e-10   1.4e-12   5.8e-15   7.0e-16   3.9e-14
  pose_without_rows             1e-3   6.1e-11   6.5e-10   2.9e-10   4.0e-13   4.2e-15   1.1e-15   3.5e-14
  more_landmarks_than_rows      1e-3   2.1e-12   1.1e-11   4.2e-12   1.0e-14   1.4e-16   5.1e-16   3.6e-14
  more_poses_than_landmarks     1e-3   4.7e-10   7.0e-09   2.8e-10   1.1e-11   2.6e-15   2.7e-16   5.4e-13
  behind_the_camera             1e+4   3.2e-12   3.7e-10   4.1e-09   5.0e-15   5.0e-15   6.9e-14   4.4e-10

c0 agrees to 3e-16 .. 2.6e-15 everywhere.  In dc and dl the device is as far from the oracle's Schur route as that route is from
the full system: the figures are the reference's floor, not the device's error.  Unobserved landmarks against their closed form:
1.4e-16.  late_failure: last_info = 595 = 1 + row 594 in all three factorisation modes.
"""
import numpy as np
import pytest

import schur_cases as C
from oracle import ba_oracle as O
from oracle import schur_oracle as S
from vinsat_amd import synth

pytestmark = pytest.mark.gpu


_problem = C.problem


def _engine(d):
    from vinsat_amd.schur import SchurBA
    return SchurBA(d["states0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], sigma_prior=d["sigma"])


@pytest.mark.parametrize("n_poses,n_landmarks", [(12, 150), (23, 400)])      # 72 and 138 unknowns: both padded to one panel of 256 (4 tiles of 64)
def test_one_trial_matches_the_cpu_restatement(n_poses, n_landmarks):
    d = _problem(n_poses, n_landmarks, 1)
    e = _engine(d)
    for lam in (1e-3, 1e-6):
        e.set_state(d["states0"], d["X0"])
        c0, c1, ok = e.iterate(lam)
        r0, r1, rok, st_ref, X_ref, dc_ref, dl_ref = S.lm_trial(d["states0"], d["X0"], d["X0"], d["uv"], d["w"], d["pose_of_row"],
                                                                d["landmark_of_row"], d["intrinsics"], d["sigma"], lam)
        assert abs(c0 - r0) <= 1e-10 * r0 and abs(c1 - r1) <= 1e-7 * r1 and ok == rok
        dc, dl = e.last_step()
        assert np.abs(dc - dc_ref).max() / np.abs(dc_ref).max() < 1e-7
        assert np.abs(dl - dl_ref).max() / np.abs(dl_ref).max() < 1e-7
        st, X = e.get_state()
        assert np.abs(st - st_ref).max() / np.abs(st_ref).max() < 1e-9 and np.abs(X - X_ref).max() / np.abs(X_ref).max() < 1e-10
        # the factor the matrix cores produced is the Cholesky factor of the reduced camera matrix
        B, C, E, v, wl = S.normal_equations(d["states0"], d["X0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"],
                                            d["intrinsics"], d["sigma"], lam)
        _, _, Sm, Lc = S.step_schur(B, C, E, v, wl)
        Lg = e.cholesky_factor()
        assert np.abs(Lg @ Lg.T - Sm).max() / np.abs(Sm).max() < 1e-11
        assert np.abs(Lg - Lc).max() / np.abs(Lc).max() < 1e-8
    e.close()


def test_lm_converges_like_the_cpu_restatement_and_is_repeatable():
    d = _problem(40, 600, 3)
    e = _engine(d)
    hist = e.solve(lamda0=1e-4, max_iters=10)
    st, X, lam = d["states0"], d["X0"].copy(), 1e-4
    for k in range(len(hist)):
        c0, c1, ok, st, X, _, _ = S.lm_trial(st, X, d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"],
                                             d["sigma"], lam)
        assert hist[k][2] == ok and abs(hist[k][1] - c1) <= 1e-6 * c1, k
        lam = max(lam * 0.1, 1e-9) if ok else lam * 10
    at_truth = S.cost(d["states_gt"], d["X_true"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], d["sigma"])
    assert hist[-1][1] < 1.05 * at_truth
    gs, gX = e.get_state()
    assert np.abs(gs - st).max() / np.abs(st).max() < 1e-8
    assert np.linalg.norm(gX - d["X_true"]) < 0.9 * np.linalg.norm(d["X0"] - d["X_true"])
    # fixed-order reductions: a second run gives the same bits
    e2 = _engine(d)
    hist2 = e2.solve(lamda0=1e-4, max_iters=10)
    assert hist2 == hist and np.array_equal(e2.get_state()[0], gs) and np.array_equal(e2.get_state()[1], gX)
    e.close()
    e2.close()


def test_indefinite_system_is_a_rejected_trial_not_an_error():
    """A reduced camera system that is not positive definite at the given damping fails its Cholesky factorisation: the
    ordinary LM response is a rejected trial (the caller raises lamda), with the failing row on record -- not an abort."""
    d = _problem(12, 150, 5)
    d["w"] = -d["w"]                    # negative weights: the reduced system is not positive definite
    e = _engine(d)
    before = e.get_state()
    c0, c1, ok = e.iterate(0.0)
    assert not ok and c1 == c0 and e.last_info() > 0
    after = e.get_state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])      # the state is untouched
    hist = e.solve(lamda0=1e-4, max_iters=4)            # the driver keeps going (and keeps rejecting: nothing to gain here)
    assert all(not h[2] for h in hist) and hist[-1][3] > hist[0][3]
    e.close()


@pytest.mark.parametrize("name", ["c1", "c2"])
def test_frozen_landmarks_limit_reproduces_the_reference_pose_step(name):
    """The one anchor this add-on has in the REFERENCE (everything else about it is pinned to this repository's own
    restatement only: parity unpinned).  With sigma_prior -> 0 the landmarks cannot move, the Schur complement
    S = B - E C^-1 E^T collapses to the pose blocks B, and one trial at the reference's first call -- iter = 0, i.e.
    alpha = 2 and w = confidence (BA_filtering.py:22-25), landmark-only phase, damping float32(1e-4) on the diagonal
    (:54) -- must give the reference's own step: rows [:, :6] of dpose_0 in tests/golden/c1.npz / c2.npz, captured from
    torch.linalg.solve inside the reference's BA (:55).  That pins k_lm_blocks / k_pose_blocks (the same reprojection
    Jacobian and weights), the Schur build and the blocked Cholesky + substitutions to a reference-made fixture."""
    from conftest import golden_inputs, load_golden
    from vinsat_amd.schur import SchurBA
    g = load_golden(name)
    inp = golden_inputs(g)
    n, m = inp["K"].shape[0], inp["xyz"].shape[0]
    assert g["iters"][0] == 0 and bool(g["initialize"][0])
    e = SchurBA(g["states0"][0], inp["xyz"], inp["uv"], inp["conf"], inp["ii"], np.arange(m), inp["K"], sigma_prior=1e-6)
    lam32 = float(np.float32(g["lamda_in"][0]))
    c0, c1, ok = e.iterate(lam32)
    dc, dl = e.last_step()
    ref = g["dpose_0"][0].reshape(n, 9)[:, :6]
    assert np.abs(dc - ref).max() / np.abs(ref).max() < 1e-6
    assert np.abs(dl).max() < 1e-6 * np.abs(ref[:, :3]).max()        # the landmarks stayed where the catalogue has them
    e.close()


# ------------------------------------------------------------------------------------------------ beyond one panel
def _open(name):
    from vinsat_amd.schur import SchurBA
    d = C.case(name)
    e = SchurBA(d["states0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], sigma_prior=d["sigma"])
    e.set_state(d["states0"], d["Xs"])
    return d, e


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _trial_matches(e, name, lam, label=""):
    """One trial from the case's start against the oracle: the per-trial assertions of
    test_one_trial_matches_the_cpu_restatement, each figure printed before it is asserted.  Returns the device's factor."""
    d, r = C.case(name), C.reference(name, lam)
    e.set_state(d["states0"], d["Xs"])
    c0, c1, ok = e.iterate(lam)
    dc, dl = e.last_step()
    st, X = e.get_state()
    Lg = e.cholesky_factor()
    fig = dict(c0=abs(c0 - r.c0) / r.c0, c1=abs(c1 - r.c1) / r.c1, dc=_rel(dc, r.dc), dl=_rel(dl, r.dl), st=_rel(st, r.st), X=_rel(X, r.X),
               LLt=_rel(Lg @ Lg.T, r.Sm), L=_rel(Lg, r.Lc))
    print(f"FIGURES {name} {label} lam={lam:g} info={e.last_info()} ok={ok}/{r.ok} " + " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    assert e.last_info() == 0
    assert abs(c0 - r.c0) <= 1e-10 * r.c0 and abs(c1 - r.c1) <= 1e-7 * r.c1 and ok == r.ok
    assert fig["dc"] < 1e-7
    assert fig["dl"] < 1e-7
    assert fig["st"] < 1e-9 and fig["X"] < 1e-10
    assert fig["LLt"] < 1e-11
    assert fig["L"] < 1e-8
    return Lg


@pytest.mark.parametrize("name,N,Npad,panels", [("43", 258, 512, 2), ("128", 768, 768, 3), ("129", 774, 1024, 4)])
def test_multi_panel_trial_matches_the_cpu_restatement(name, N, Npad, panels):
    """Two, three and four panels: the panel update, the bulk update on the second stream and the ordering between them, on
    matrices with fill; with 254, 0 and 250 padding rows."""
    d, e = _open(name)
    n = d["states0"].shape[0]
    assert C.kernel_constants() == (64, 4)              # the shapes of this module reach their branches for these only
    assert (N, Npad, panels) == C.padded_shape(n) and (6 * n + 255) // 256 == panels
    assert e.cholesky_factor().shape == (N, N)
    # the band k_trsv_step relies on: narrow here (most tiles skipped), and the reference's factor is exactly zero beyond it
    bw = C.tile_bandwidth(e.structure)
    assert bw == 2 < (N + 63) // 64 - 1
    skipped, zero = C.tiles_beyond_band_are_zero(C.reference(name, 1e-3).Lc, bw)
    assert skipped > 0 and zero
    for lam in (1e-3, 1e-6):
        _trial_matches(e, name, lam)
    e.close()


def test_two_streams_give_the_same_bits_every_time():
    """Four panels: the same trial from the same state twice on one handle and once on another.  Every reduction runs in a
    fixed order, so factor, step and costs repeat bit for bit; an unordered pair of launches on the two streams would not."""
    d, e = _open("129")
    e2 = _open("129")[1]
    runs = []
    for eng in (e, e, e2):
        eng.set_state(d["states0"], d["Xs"])
        c = eng.iterate(1e-3)
        runs.append((c, eng.cholesky_factor(), *eng.last_step()))
    for c, Lg, dc, dl in runs[1:]:
        assert c == runs[0][0]
        assert np.array_equal(Lg, runs[0][1]) and np.array_equal(dc, runs[0][2]) and np.array_equal(dl, runs[0][3])
    e.close()
    e2.close()


def test_wide_band_trial_matches_the_cpu_restatement():
    """A reduced system that is NOT banded: no tile is skipped by the substitutions, and every tile of every panel is full."""
    d, e = _open("wide")
    added = np.stack([d["pose_of_row"][-20:], d["landmark_of_row"][-20:]], 1)
    assert np.unique(added, axis=0).shape[0] == 20
    N = 6 * d["states0"].shape[0]
    nb_used = (N + 63) // 64
    assert C.tile_bandwidth(e.structure) == nb_used - 1 == 12
    assert np.any(C.reference("wide", 1e-3).Sm[64 * (nb_used - 1):, :64] != 0.0)
    _trial_matches(e, "wide", 1e-3)
    e.close()


def test_comparison_factorisations_match_the_cpu_restatement_and_each_other(monkeypatch):
    """VBA_SCHUR_CLASSIC=1 (tile by tile, k_potrf64 and the K = 64 trailing update) and =2 (panels with k_potrf64)."""
    Ls = {}
    for mode in ("0", "1", "2"):
        monkeypatch.setenv("VBA_SCHUR_CLASSIC", mode)           # read in vba_schur_create
        e = _open("129")[1]
        Ls[mode] = _trial_matches(e, "129", 1e-3, label=f"classic={mode}")
        e.close()
    assert not np.array_equal(Ls["0"], Ls["1"])                 # (the variable took effect: another order of operations)
    scale = np.abs(C.reference("129", 1e-3).Lc).max()
    for a, b in (("0", "1"), ("0", "2"), ("1", "2")):
        assert np.abs(Ls[a] - Ls[b]).max() / scale < 1e-8


@pytest.mark.parametrize("mode", ["0", "1", "2"])
def test_last_info_tells_the_first_failing_row(mode, monkeypatch):
    """include/vinsat_ba.h: "1 + the row of the reduced system at which it met a non-positive pivot" -- the FIRST such row (the
    only one a CPU factorisation can be compared with: the device replaces a bad pivot by 1 and goes on), in a later panel, in
    at the start of neither a tile nor a 16-row block, and kept although tiles after it fail too.  That the row is beyond the
    reach of rounding is checked on the CPU (tests/test_schur_oracle.py::test_late_failure_is_unambiguous)."""
    _, row, _ = C.late_failure_reference()
    assert row % 64 != 0 and row % 16 != 0
    monkeypatch.setenv("VBA_SCHUR_CLASSIC", mode)
    d, e = _open("late_failure")
    before = e.get_state()
    c0, c1, ok = e.iterate(0.0)
    print(f"FIGURES late_failure classic={mode} info={e.last_info()} expected={row + 1}")
    assert e.last_info() == row + 1
    assert not ok and c1 == c0
    after = e.get_state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    e.close()


# ------------------------------------------------------------------------------------------------ edges of the build kernels
def test_pose_without_rows_keeps_its_place():
    d, e = _open("pose_without_rows")
    lam, i = 1e-3, d["empty_pose"]
    assert not np.any(d["pose_of_row"] == i) and 0 < i < d["states0"].shape[0] - 1
    Lg = _trial_matches(e, "pose_without_rows", lam)
    dc, _ = e.last_step()
    assert np.all(dc[i] == 0.0)
    # its block of S is lam I and nothing couples it: the factor's rows are sqrt(lam) on the diagonal (lam - 0 is exact, the
    # square root correctly rounded up to the last bit), exactly zero elsewhere
    rows = Lg[6 * i:6 * i + 6]
    off = rows.copy()
    off[:, 6 * i:6 * i + 6] -= np.diag(np.diag(rows[:, 6 * i:6 * i + 6]))
    assert not off.any() and not Lg[6 * i + 6:, 6 * i:6 * i + 6].any()
    assert np.all(np.abs(np.diag(rows[:, 6 * i:6 * i + 6]) - np.sqrt(lam)) <= 2.0 ** -52 * np.sqrt(lam))
    e.close()


def test_more_landmarks_than_rows_and_unobserved_landmarks_follow_their_prior():
    """L = 400 > m: k_cost's grid is sized by the landmarks.  An unobserved landmark is held by its prior alone."""
    d, e = _open("more_landmarks_than_rows")
    lam = 1e-3
    assert d["X0"].shape[0] > d["uv"].shape[0] and d["unobserved"].size > 200
    _trial_matches(e, "more_landmarks_than_rows", lam)
    _, dl = e.last_step()
    u, inv_sigma2 = d["unobserved"], 1.0 / d["sigma"] ** 2
    closed = -(d["Xs"][u] - d["X0"][u]) * inv_sigma2 / (inv_sigma2 + lam)
    assert np.abs(closed).min() > 0
    print("FIGURES unobserved landmarks against the closed form", _rel(dl[u], closed))
    assert _rel(dl[u], closed) < 1e-12
    e.close()


def test_more_poses_than_landmarks():
    """L = 8 < n = 12: k_lm_update's grid is sized by the poses."""
    d, e = _open("more_poses_than_landmarks")
    assert d["X0"].shape[0] == 8 < d["states0"].shape[0] and np.unique(d["landmark_of_row"]).size == 8
    _trial_matches(e, "more_poses_than_landmarks", 1e-3)
    e.close()


def test_landmarks_behind_the_camera_are_clamped_as_in_the_oracle():
    """Depth below Z_MIN: clamped in the projection, no derivative along the axis -- in cost, blocks and step alike.  At
    lam = 1e4 (see the module docstring: at smaller damping the oracle's own Schur route is not good to a tenth of the bar)."""
    d, e = _open("behind_the_camera")
    k = d["clamped_rows"]
    pc = np.einsum("kji,kj->ki", O.rotation_matrix(d["states0"][d["pose_of_row"][k], 3:7] / np.linalg.norm(d["states0"][d["pose_of_row"][k], 3:7], axis=1, keepdims=True)),
                   d["Xs"][d["landmark_of_row"][k]] - d["states0"][d["pose_of_row"][k], :3])
    assert np.all(np.abs(pc[:, 2] + 1.0) < 1e-9) and np.all(np.hypot(pc[:, 0], pc[:, 1]) <= 0.005)
    keep = np.ones(d["uv"].shape[0], dtype=bool)
    keep[k] = False
    others = S.cost(d["states0"], d["Xs"], d["X0"], d["uv"][keep], d["w"][keep], d["pose_of_row"][keep], d["landmark_of_row"][keep],
                    d["intrinsics"], d["sigma"])
    c0 = C.reference("behind_the_camera", 1e4).c0
    assert 0 < c0 - others < 0.5 * c0               # the other rows still count in the relative bars
    _trial_matches(e, "behind_the_camera", 1e4)
    e.close()
