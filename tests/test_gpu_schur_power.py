"""``vba_schur_outlier_power`` / ``vba_schur_outlier_power_dyn`` (``SchurBA.outlier_power``, ``state_outlier_power``) on the GPU against
the CPU reference of tests/schur_power_cases.py.

Bars: ``max(100 x floor of the case, 1e-11)`` relative to the largest entry of the family (mdb, ext_pos, ext_att, ext_lm, del_pos,
del_lm, lm_mdb, lm_ext, lm_del_pos); the floor is the disagreement of the reference's two NumPy routes
(tests/test_schur_power_host.py holds it below 1e-8 and lists it).  Every figure is printed before it is asserted.  Rows whose
``I - P_k`` has a smallest eigenvalue below 1e-3 in the REFERENCE and rows of weight 0 are compared on nothing that divides by it
(5 of 1474 rows in ``behind_the_camera``, none elsewhere); landmarks with reference ``q < 1e-9`` and landmarks without rows likewise
(37 of ``more_landmarks_than_rows``, 2 of the dynamics case 29 / 300 at ``lamda = 0``).  Every test here needs the entry point and
fails where it does not exist.

Linearisation sanity (the two last tests): the margin is the oracle's own.  On the CPU, tests/schur_power_cases.py settles 12 / 150
with the planted row (``schur_rel_cases.planted_outlier``) by Gauss-Newton steps, zeroes the row's weight and settles again: the
pose moves 1.215637 km where the reference's ``del_pos`` says 1.214967 km, a linearisation error of 5.5e-4 (``del_lm``: 3e-5).  With
the displaced catalogue entry (``displaced_landmark``) and its prior released (``release_prior``, 14 rounds) the worst-hit pose
moves 0.103131 km where ``lm_del_pos`` says 0.103339 km: 2.0e-3, of which the rounds' remainder (the entry still 0.19 m from the
estimate) is a part.  The device is held to about three times those: 2e-3 and 6e-3 (tests/test_schur_power_host.py
recomputes the oracle's figures).
"""
import ctypes

import numpy as np
import pytest

import schur_cases as C
import schur_dyn_cases as DC
import schur_power_cases as PW
import schur_query_harness as H
import schur_rel_cases as R

pytestmark = pytest.mark.gpu
ROW, LM = PW.ROW_FAMILIES, PW.LM_FAMILIES
OUTPUTS = PW.FAMILIES + ("pose_fit", "fit")
NCP, CRIT = PW.NCP, 3.29


def _open(name=None, d=None, state=None, dyn=False):
    d = (DC.case(name) if dyn else R.problem(name)) if d is None else d
    return d, H.engine(d, dynamics=dyn, state=state)


def _ask(e, dyn, *a, **k):
    return (e.state_outlier_power if dyn else e.outlier_power)(*a, **k)


def _rel(e, dyn, lam):
    return (e.state_reliability if dyn else e.reliability)(lam)


def _bits(a):
    return [np.asarray(a[k]).tobytes() for k in OUTPUTS[:-1]] + [np.array(list(a["fit"].values())).tobytes(), a["info"]]


_fin_max = H.fin_max


def _consistent(d, e, got, rel, crit, dyn):
    """Summaries against the device's own arrays: counts and maxima exactly, the leading slots and the leverage sums bit for bit."""
    lead = 10 if dyn else 8
    fit, rfit = list(got["fit"].values()), list(rel["fit"].values())
    assert len(fit) == lead + 4 and np.array(fit[:lead]).tobytes() == np.array(rfit).tobytes()
    assert got["pose_fit"][:, 1].tobytes() == np.ascontiguousarray(rel["pose_stats"][:, 0]).tobytes()
    with np.errstate(invalid="ignore"):
        over, lm_over = rel["wtest"] > crit, rel["lm_wtest"] > crit
    assert fit[lead] == float(over.sum()) and fit[lead + 2] == float(lm_over.sum())
    assert fit[lead + 1] == _fin_max(got["ext_pos"]) and fit[lead + 3] == _fin_max(got["lm_del_pos"])
    pr = d["pose_of_row"]
    assert np.array_equal(got["pose_fit"][:, 3], np.bincount(pr, weights=over.astype(float), minlength=e.n))
    mx = np.zeros(e.n)
    np.maximum.at(mx, pr, np.where(np.isfinite(got["ext_pos"]), got["ext_pos"], 0.0))
    assert np.array_equal(got["pose_fit"][:, 2], mx)
    res = _residual_cost(d, e)
    om = np.bincount(pr, weights=res, minlength=e.n)
    assert np.abs(got["pose_fit"][:, 0] - om).max() <= 1e-10 * max(om.max(), 1e-300)


def _residual_cost(d, e):
    from oracle import schur_oracle as S
    st, X = e.get_state()
    r, _, _ = S.linearise(st, X, d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"])
    return d["w"] * (r * r).sum(1)


def _matches(name, lam, dyn=False, crit=CRIT):
    r = PW.reference(name, lam, dyn)
    d, e = _open(name, dyn=dyn)
    got = _ask(e, dyn, lam, NCP, crit)
    assert got["info"] == 0
    fig = PW.figures(got, r)
    print(f"FIGURES power {'dynamics ' if dyn else ''}{name} lam={lam:g} " + " ".join(f"{k}={fig[k]:.2e} (bar {PW.bar(r, k):.1e})" for k in PW.FAMILIES) +
          f" rows left out {r.left_out} of {r.kept.size}, landmarks {r.lm_left_out} of {r.lm_kept.size}")
    assert r.left_out <= PW.MAX_LEFT_OUT * r.kept.size
    for k in ROW:
        assert np.all(np.isfinite(got[k][r.kept])), k
    for k in LM:
        assert np.all(np.isfinite(got[k][r.lm_kept])), k
    for k in PW.FAMILIES:
        assert fig[k] <= PW.bar(r, k), k
    _consistent(d, e, got, _rel(e, dyn, lam), crit, dyn)
    assert (e.last_state_outlier_power_ms() if dyn else e.last_outlier_power_ms()) > 0.0
    return d, e, got, r


@pytest.mark.parametrize("name,lam", [c for c in PW.CASES if c[0] not in ("more_landmarks_than_rows", "zero_weights")])
def test_matches_the_reference(name, lam):
    d, e, got, r = _matches(name, lam, crit=1.0 if name == "12" else CRIT)
    if name != "behind_the_camera":
        assert r.left_out == 0 and r.lm_left_out == 0
    e.close()


@pytest.mark.parametrize("name,lam", PW.DYN_CASES)
def test_matches_the_reference_with_the_dynamics_factor(name, lam):
    d, e, got, r = _matches(name, lam, dyn=True, crit=1.0)
    assert list(got["fit"])[8:10] == ["t_edges", "omega_edges"] and got["fit"]["t_edges"] > 0.0
    e.close()


def test_zero_weights_give_inf_and_zeros():
    d, e, got, r = _matches("zero_weights", 1e-3)
    off = d["w"] == 0.0
    assert off.sum() == (e.m + 6) // 7 and np.all(np.isposinf(got["mdb"][off]))
    for k in ROW[1:]:
        assert np.array_equal(got[k][off], np.zeros(off.sum())), k
    e.close()


def test_landmarks_without_rows_and_singular_priors():
    d, e, got, r = _matches("more_landmarks_than_rows", 0.0)
    u = d["unobserved"]
    assert u.size > 200
    assert np.all(np.isposinf(got["lm_mdb"][u])) and np.array_equal(got["lm_ext"][u], np.zeros(u.size)) and np.array_equal(got["lm_del_pos"][u], np.zeros(u.size))
    sing = r.seen & ~r.lm_kept          # the tracks of one row: I - P_l exactly singular, q is rounding of either sign
    assert sing.sum() == 37
    for k in ("lm_mdb", "lm_ext"):      # NaN (q <= 0) or the huge value of a q of a few ulps
        assert np.all(np.isnan(got[k][sing]) | (got[k][sing] > 1e3 * got[k][r.lm_kept].max())), k
    left = got["lm_del_pos"][sing]
    assert np.all(np.isnan(left) | (left >= 0.0))
    g2 = e.outlier_power(1e-3)          # with damping the closed forms of a landmark without rows stay
    assert np.all(np.isposinf(g2["lm_mdb"][u])) and np.array_equal(g2["lm_ext"][u], np.zeros(u.size))
    e.close()


def _raw(e, lam, on=None, ncp=NCP, crit=CRIT, dyn=False):
    """The C entry itself: (rc, info, outputs in the order of OUTPUTS, device row order); outputs not asked for are None (NULL)."""
    return H.raw_query(e, "vba_schur_outlier_power_dyn" if dyn else "vba_schur_outlier_power", lam, on, ncp=ncp, crit=crit)


@pytest.mark.parametrize("dyn", [False, True])
def test_failed_factorisation_gives_nan_and_ok(dyn):
    """The negative-weight recipe of the covariance tests (``late_failure``: the rows of the last 30 poses weigh less than nothing),
    and on a handle with the dynamics factor its failure case (43 / 450 at ``lamda = 0``): NaN everywhere, the row in ``info``, VBA_OK."""
    import schur_dyn_rel_cases as DR
    if dyn:
        name, lam = DR.FAILURE
        d, e = _open(name, dyn=True)
        want = 124
    else:
        lam, want = 0.0, C.late_failure_reference()[1] + 1
        d, e = _open(d=C.case("late_failure"))
    rc, info, *bufs = _raw(e, lam, dyn=dyn)
    print(f"FIGURES power failed factorisation dyn={dyn} rc={rc} info={info} expected={want}")
    assert rc == 0 and info == want
    assert all(np.all(np.isnan(b)) for b in bufs)
    from vinsat_amd._lib import VbaError
    with pytest.raises(VbaError, match="not positive definite"):
        _ask(e, dyn, lam)
    g = _ask(e, dyn, lam, strict=False)
    assert g["info"] == info and all(np.all(np.isnan(g[k])) for k in OUTPUTS[:-1]) and all(np.isnan(v) for v in g["fit"].values())
    e.close()


@pytest.mark.parametrize("dyn", [False, True])
def test_null_outputs_return_the_same_bits(dyn):
    d, e = _open("12", dyn=dyn)
    full = _raw(e, 1e-3, dyn=dyn)
    assert full[0] == 0 and full[1] == 0
    for mask in (0, 1, 0b10000000000, 0b00000111111, 0b11111000000, 0b01010101010, 0b10101010101, 0b00100000100, 0b11111111110):
        on = [bool(mask >> k & 1) for k in range(11)]
        rc, info, *bufs = _raw(e, 1e-3, on, dyn=dyn)
        assert rc == 0 and info == 0
        for k in range(11):
            assert (bufs[k] is None) == (not on[k])
            if on[k]:
                assert np.array_equal(bufs[k], full[2 + k], equal_nan=True), (mask, OUTPUTS[k])
    e.close()


@pytest.mark.parametrize("dyn", [False, True])
def test_queries_repeat_bit_for_bit_on_one_handle_and_across_handles(dyn):
    name = "29" if dyn else "43"
    d, e = _open(name, dyn=dyn)
    _, f = _open(name, dyn=dyn)
    a, b, c = _ask(e, dyn, 0.0 if not dyn else 1e-3), _ask(e, dyn, 0.0 if not dyn else 1e-3), _ask(f, dyn, 0.0 if not dyn else 1e-3)
    _ask(e, dyn, 1e-2, 10.0, 2.0)                   # (another damping, ncp and crit through the same scratch in between)
    _rel(e, dyn, 1e-2)
    g = _ask(e, dyn, 0.0 if not dyn else 1e-3)
    for o in (b, c, g):
        assert _bits(a) == _bits(o)
    e.close()
    f.close()


@pytest.mark.parametrize("dyn", [False, True])
def test_query_changes_nothing_and_later_calls_keep_their_bits(dyn):
    """Handle e asks for the power around every call (first, before any other query: its first query allocates every scratch);
    handle f never does."""
    name = "29" if dyn else "43"
    d, e = _open(name, dyn=dyn)
    _, f = _open(name, dyn=dyn)
    runs = []
    for eng, ask in ((e, True), (f, False)):
        out = []
        for lam in (1e-3, 1e-4):
            if ask:
                assert _ask(eng, dyn, lam)["info"] == 0
            out.append(eng.iterate(lam))
            if ask:
                _ask(eng, dyn, 0.0 if not dyn else 1e-3)
            c = (eng.state_covariance if dyn else eng.covariance)(lam, pairs=True)
            out.append((c["state" if dyn else "pose"].tobytes(), c["landmark"].tobytes(), c["pairs"][2].tobytes()))
            if ask:
                _ask(eng, dyn, lam)
            rl = _rel(eng, dyn, lam)
            out.append(tuple(np.asarray(rl[k]).tobytes() for k in ("leverage", "wtest", "lm_leverage", "lm_wtest", "lm_stats", "pose_stats")) +
                       (tuple(rl["fit"].values()),))
        dc, dl = eng.last_step()
        runs.append((out, *eng.get_state(), dc.copy(), dl.copy(), eng.cholesky_factor()))
    assert runs[0][0] == runs[1][0] and any(o[2] for o in runs[0][0][::3])
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert a.tobytes() == b.tobytes()
    e.close()
    f.close()


def test_rows_come_back_in_the_callers_order():
    d = R.problem("12")
    perm = np.random.default_rng(3).permutation(d["uv"].shape[0])
    p = dict(d)
    for k in ("uv", "w", "pose_of_row", "landmark_of_row"):
        p[k] = d[k][perm]
    _, e = _open(d=p)
    r = PW.reference("12", 0.0)
    got = e.outlier_power(0.0)
    back = dict(got)
    for k in ROW:
        back[k] = np.empty(e.m)
        back[k][perm] = got[k]
    fig = PW.figures(back, r)
    print("FIGURES power permuted rows", fig)
    assert all(fig[k] <= PW.bar(r, k) for k in PW.FAMILIES)
    e.close()


def test_scaled_power_scales_the_detection_figures_only():
    from vinsat_amd.schur import scaled_power
    d, e = _open("12")
    got = e.outlier_power(0.0)
    sc = scaled_power(got)
    s0 = np.sqrt(got["fit"]["s0sq"])
    assert sc["s0"] == s0 and s0 > 0.0
    for k in ("mdb", "ext_pos", "ext_att", "ext_lm", "lm_mdb", "lm_ext"):
        assert np.array_equal(sc[k], got[k] * s0)
    for k in ("del_pos", "del_lm", "lm_del_pos", "pose_fit"):
        assert sc[k] is got[k]
    e.close()


def test_argument_and_state_errors():
    from vinsat_amd._lib import load
    lib = load()
    EINVAL, ESTATE = 1, 4                           # VBA_EINVAL, VBA_ESTATE of include/vinsat_ba.h
    d, e = _open("12")
    _, f = _open("12", dyn=True)
    info = ctypes.c_int()
    nul = [None] * 11
    plain, dynq = lib.vba_schur_outlier_power, lib.vba_schur_outlier_power_dyn
    assert ESTATE not in (0, EINVAL)
    assert plain(f.h, 0.0, NCP, CRIT, *nul, ctypes.byref(info)) == ESTATE           # the plain entry refuses a dynamics handle
    assert dynq(e.h, 0.0, NCP, CRIT, *nul, ctypes.byref(info)) == ESTATE            # and the other way round
    for entry, h in ((plain, e.h), (dynq, f.h)):
        assert entry(None, 0.0, NCP, CRIT, *nul, ctypes.byref(info)) == EINVAL
        assert entry(h, 0.0, NCP, CRIT, *nul, None) == EINVAL
        assert entry(h, -1.0, NCP, CRIT, *nul, ctypes.byref(info)) == EINVAL
        for ncp in (0.0, -1.0, float("nan"), float("inf")):
            assert entry(h, 0.0, ncp, CRIT, *nul, ctypes.byref(info)) == EINVAL
        for crit in (0.0, -1.0, float("nan")):
            assert entry(h, 0.0, NCP, crit, *nul, ctypes.byref(info)) == EINVAL
        assert entry(h, 0.0, NCP, float("inf"), *nul, ctypes.byref(info)) == 0 and info.value == 0
    assert lib.vba_schur_last_outlier_power_ms(None, None) == EINVAL and lib.vba_schur_last_outlier_power_dyn_ms(None, None) == EINVAL
    g = e.outlier_power(0.0, crit=float("inf"))
    assert g["fit"]["n_rows_over_crit"] == 0.0 and g["fit"]["n_lm_over_crit"] == 0.0 and not g["pose_fit"][:, 3].any()
    s = e.structure
    h = ctypes.c_void_p()
    assert lib.vba_schur_create(0, e.n, e.m, e.L, int(s["blk_i"].size), int(s["pair_k"].size), ctypes.byref(h)) == 0
    assert plain(h, 0.0, NCP, CRIT, *nul, ctypes.byref(info)) == lib.vba_schur_covariance(h, 0.0, None, None, None, ctypes.byref(info)) != 0
    lib.vba_schur_destroy(h)
    e.close()
    f.close()


# ------------------------------------------------------------------------------------------------ linearisation sanity
def _device_step(e):
    def step(st, X):
        e.set_state(st, X)
        e.iterate(0.0)
        dc, dl = e.last_step()
        return dc.copy(), dl.copy()
    return step


def _settled(d, steps=PW.GN_STEPS, state=None):
    dd, e = _open(d=d, state=state)
    if state is None:
        hist = e.solve()
        assert any(ok for _, _, ok, _ in hist)
    st, X = PW.settle(_device_step(e), *e.get_state(), steps=steps)
    e.set_state(st, X)
    return e, st, X


def test_del_pos_predicts_the_move_of_the_pose_when_the_row_is_deleted():
    d = R.planted_outlier()
    row, i, l = d["planted_row"], d["pose_of_row"][d["planted_row"]], d["landmark_of_row"][d["planted_row"]]
    e, st, X = _settled(d)
    got = e.outlier_power(0.0)
    e.close()
    f, st2, X2 = _settled(PW.without_row(d, row), state=(st, X))
    f.close()
    move, lm_move = np.linalg.norm(st2[i, :3] - st[i, :3]), np.linalg.norm(X2[l] - X[l])
    print(f"FIGURES power planted row {row}: del_pos {got['del_pos'][row]!r} moved {move!r} ({abs(move / got['del_pos'][row] - 1):.1e}); "
          f"del_lm {got['del_lm'][row]!r} moved {lm_move!r} ({abs(lm_move / got['del_lm'][row] - 1):.1e}); mdb {got['mdb'][row]:.3f} px")
    assert abs(move / got["del_pos"][row] - 1.0) <= 2e-3 and abs(lm_move / got["del_lm"][row] - 1.0) <= 2e-3
    assert got["del_pos"][row] == got["del_pos"].max()          # the planted row is the one whose deletion moves a pose most


def test_lm_del_pos_predicts_the_move_of_the_worst_hit_pose_when_the_prior_is_released():
    d = R.displaced_landmark()
    l = d["displaced_lm"]
    e, st, X = _settled(d)
    got = e.outlier_power(0.0)
    e.close()

    def converge(p, s, x):
        f, s2, x2 = _settled(p, steps=6, state=(s, x))
        f.close()
        return s2, x2

    st2, X2, left = PW.release_prior(d, l, st, X, converge)
    poses = d["pose_of_row"][d["landmark_of_row"] == l]
    move = np.linalg.norm(st2[poses, :3] - st[poses, :3], axis=1).max()
    print(f"FIGURES power displaced landmark {l}: lm_del_pos {got['lm_del_pos'][l]!r} moved {move!r} ({abs(move / got['lm_del_pos'][l] - 1):.1e}), "
          f"entry {left:.2e} km from the estimate; lm_mdb {got['lm_mdb'][l]:.4f} km")
    assert abs(move / got["lm_del_pos"][l] - 1.0) <= 6e-3
