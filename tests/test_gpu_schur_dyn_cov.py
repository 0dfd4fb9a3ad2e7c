"""``vba_schur_covariance_dyn`` / ``SchurBA.state_covariance`` on the GPU: the state covariances of a handle with the dynamics factor
against the CPU reference of tests/schur_dyn_cov_cases.py (cases and why each is there: that module).  PARITY UNPINNED as the rest
of the add-on.

Bars: ``max(100 x floor of the case, 1e-11)`` per family (state / edges / pairs / landmark), every entry scaled by the reference
sigmas of its own row and column; the floor is the disagreement of the reference's two NumPy routes
(tests/test_schur_dyn_cov_host.py holds it below 1e-8).  Every figure is printed before it is asserted.  Device against
reference, measured on an MI355X: DESIGN 9.6.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import schur_cases as SC
import schur_dyn_cov_cases as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTPUTS = ("state", "edges", "landmark")


def engine(d, dynamics=True, sigma_dyn=None):
    from vinsat_amd.schur import SchurBA
    kw = dict(time_idx=d["time_idx"], sigma_dyn=d["sigma_dyn"] if sigma_dyn is None else sigma_dyn) if dynamics else {}
    e = SchurBA(d["states0"], d["X0"], d["uv"], d["w"], d["pose_of_row"], d["landmark_of_row"], d["intrinsics"], sigma_prior=d["sigma"], **kw)
    e.set_state(d["states0"], d["Xs"])
    return e


def _matches(e, name, lam, label=""):
    r = V.reference(name, lam)
    c = e.state_covariance(lam, pairs=True)
    assert c["info"] == 0
    bi, bj, blocks = c["pairs"]
    assert np.array_equal(bi, r.blk_i) and np.array_equal(bj, r.blk_j)
    got = dict(state=c["state"], edges=c["edges"], pairs=blocks, landmark=c["landmark"])
    for k in V.FAMILIES:
        assert got[k].shape == getattr(r, k).shape and np.all(np.isfinite(got[k])), k
    fig = V.scaled(got, r)
    print(f"FIGURES state cov {name} {label} lam={lam:g} " + " ".join(f"{k}={fig[k]:.2e} (floor {r.floor[k]:.1e}, bar {V.bar(r, k):.1e})" for k in V.FAMILIES))
    for k in V.FAMILIES:
        assert fig[k] <= V.bar(r, k), k
    return c, r


def _same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in OUTPUTS) and np.array_equal(a["pairs"][2], b["pairs"][2])


# ------------------------------------------------------------------------------------------------ 1. accuracy
@pytest.mark.parametrize("name,lam", V.CASES)
def test_matches_the_reference(name, lam):
    e = engine(V.case(name))
    _matches(e, name, lam)
    assert e.last_state_covariance_ms() > 0.0
    e.close()


# ------------------------------------------------------------------------------------------------ 2. bit relations
@pytest.mark.parametrize("name", ("12", "29", "86"))
def test_bit_relations_on_one_handle_and_across_handles(name):
    d = V.case(name)
    e, f = engine(d), engine(d)
    a = e.state_covariance(1e-3, pairs=True)
    bi, bj, blocks = a["pairs"]
    dg = bi == bj
    assert np.array_equal(bi[dg], np.arange(e.n)) and np.array_equal(blocks[dg], a["state"][:, :6, :6])
    assert np.array_equal(a["state"], np.swapaxes(a["state"], 1, 2))
    assert np.array_equal(a["landmark"], np.swapaxes(a["landmark"], 1, 2))
    e.state_covariance(0.0)                         # (another damping through the same scratch in between)
    assert _same_bits(a, e.state_covariance(1e-3, pairs=True)) and _same_bits(a, f.state_covariance(1e-3, pairs=True))
    e.close(), f.close()


_CHILD = """
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np
import schur_dyn_cov_cases as V
from test_gpu_schur_dyn_cov import engine
out = {{}}
for name in ("29", "86"):
    e = engine(V.case(name))
    c = e.state_covariance(1e-3, pairs=True)
    e.close()
    out.update({{name + "_" + k: c[k] for k in ("state", "edges", "landmark")}})
    out[name + "_pairs"] = c["pairs"][2]
np.savez({path!r}, **out)
"""


def test_full_product_gives_the_bits_of_the_selected_product(tmp_path):
    """A child process with VBA_SCHUR_COV_FULL=1 (read when the handle is created) forms every tile of S9^-1 by k_syrk_wtw; this
    process forms the listed tiles by k_syrk_wtw_sel.  Every output has the same bits on 29 / 300 and 86 / 900."""
    assert not os.environ.get("VBA_SCHUR_COV_FULL")
    path = str(tmp_path / "full.npz")
    code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), path=path)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, VBA_SCHUR_COV_FULL="1"), cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    full = np.load(path)
    for name in ("29", "86"):
        e = engine(V.case(name))
        c = e.state_covariance(1e-3, pairs=True)
        e.close()
        for k in OUTPUTS:
            assert np.array_equal(c[k], full[f"{name}_{k}"]), (name, k)
        assert np.array_equal(c["pairs"][2], full[f"{name}_pairs"]), name


# ------------------------------------------------------------------------------------------------ 3. failure path
def test_failed_factorisation_gives_nan_and_the_row():
    from vinsat_amd._lib import VbaError
    name, lam = V.FAILURE
    _, _, _, S9 = V.failure_system()
    row, _ = SC.first_bad_pivot(S9)                 # the unpivoted Cholesky of the oracle's S9, not a figure taken on trust
    assert row == 6 * 20 + 3
    e = engine(V.case(name))
    c = e.state_covariance(lam, pairs=True, strict=False)
    print(f"FIGURES state cov failure info={c['info']} expected={row + 1}")
    assert c["info"] == row + 1 == 124
    for k in OUTPUTS:
        assert np.all(np.isnan(c[k])), k
    assert np.all(np.isnan(c["pairs"][2]))
    assert e.last_info() == 0                       # the handle's own record belongs to its iterates
    with pytest.raises(VbaError, match=f"row {row}\\b"):
        e.state_covariance(lam)
    _matches(e, name, 1e-3, label="after the failure")
    e.close()


# ------------------------------------------------------------------------------------------------ 4. the query changes nothing
def _snapshot(e):
    st, X = e.get_state()
    dc, dl = e.last_step()
    return [e.dynamics_residual(), e.dynamics_jacobian(), e.dynamics_edge_cost(), dc.copy(), dl.copy(), e.last_velocity_step(),
            e.cholesky_factor(), st, X, np.array([e.last_info()])]


def test_query_changes_nothing_the_handle_shows():
    """After an accepted trial the resident state is not the state the handle's r, D Phi and edge costs were built at: a query that
    built into the handle's arrays would change what the fetches return."""
    d = V.case("29")
    e, f = engine(d), engine(d)
    for eng in (e, f):
        for _ in range(6):
            if eng.iterate(1e-3)[2]:
                break
        else:
            raise AssertionError("no trial was accepted")
    st0, _ = e.get_state()
    assert not np.array_equal(st0, d["states0"])
    c0 = e.state_covariance(0.0)
    c1 = e.state_covariance(1e-3, pairs=True)
    assert c0["info"] == 0 and c1["info"] == 0
    for a, b in zip(_snapshot(e), _snapshot(f)):
        assert a.tobytes() == b.tobytes()
    assert e.iterate(1e-4) == f.iterate(1e-4)
    for a, b in zip(e.get_state(), f.get_state()):
        assert np.array_equal(a, b)
    e.close(), f.close()


# ------------------------------------------------------------------------------------------------ 5. contract
def test_contract_and_refusals():
    import ctypes
    from vinsat_amd._lib import PD, VbaError
    d = V.case("12")
    p = engine(d, dynamics=False)
    with pytest.raises(VbaError, match="dynamics factor is not enabled"):
        p.state_covariance()
    assert p.covariance()["info"] == 0
    p.close()
    e = engine(d)
    with pytest.raises(VbaError, match="not available on a handle with the dynamics factor"):
        e.covariance()
    with pytest.raises(VbaError, match="lamda must be >= 0"):
        e.state_covariance(-1.0)
    with pytest.raises(VbaError, match="lamda must be >= 0"):
        e.state_covariance(float("nan"))
    lib, info = e.lib, ctypes.c_int()
    st, ed = np.empty((e.n, 9, 9)), np.empty((e.n - 1, 9, 9))
    ps, pe = st.ctypes.data_as(PD), ed.ctypes.data_as(PD)
    assert lib.vba_schur_covariance_dyn(None, 0.0, ps, pe, None, None, ctypes.byref(info)) == 1        # VBA_EINVAL
    assert lib.vba_schur_covariance_dyn(e.h, 0.0, None, pe, None, None, ctypes.byref(info)) == 1
    assert lib.vba_schur_covariance_dyn(e.h, 0.0, ps, None, None, None, ctypes.byref(info)) == 1
    assert lib.vba_schur_covariance_dyn(e.h, 0.0, ps, pe, None, None, None) == 1
    assert lib.vba_schur_last_covariance_dyn_ms(None, None) == 1
    # pair_cov and lm_cov may be NULL: the required outputs keep their bits
    full = e.state_covariance(1e-3)
    assert lib.vba_schur_covariance_dyn(e.h, 1e-3, ps, pe, None, None, ctypes.byref(info)) == 0 and info.value == 0
    assert np.array_equal(st, full["state"]) and np.array_equal(ed, full["edges"])
    # before a state is set: the answer of vba_schur_iterate
    s = e.structure
    h = ctypes.c_void_p()
    assert lib.vba_schur_create(0, e.n, e.m, e.L, int(s["blk_i"].size), int(s["pair_k"].size), ctypes.byref(h)) == 0
    rc = lib.vba_schur_covariance_dyn(h, 0.0, ps, pe, None, None, ctypes.byref(info))
    assert rc != 0 and rc == lib.vba_schur_iterate(h, 0.0, ctypes.byref(ctypes.c_double()), ctypes.byref(ctypes.c_double()), ctypes.byref(ctypes.c_int()))
    lib.vba_schur_destroy(h)
    e.close()


# ------------------------------------------------------------------------------------------------ 6. consistency with the plain mode
def _scaled_by(got, ref):
    sd = np.sqrt(np.diagonal(ref, axis1=1, axis2=2))
    return float((np.abs(got - ref) / (sd[:, :, None] * sd[:, None, :])).max())


def _min_eig_rel(M):
    w = np.linalg.eigvalsh(0.5 * (M + np.swapaxes(M, -1, -2)))
    return float((w[..., 0] / np.abs(w).max(axis=-1)).min())


@pytest.mark.parametrize("name", ("29", "86"))
def test_consistency_with_the_plain_mode(name):
    d = V.case(name)
    p, t, e = engine(d, dynamics=False), engine(d, sigma_dyn=1e-30), engine(d)
    plain, tiny, c = p.covariance(1e-3), t.state_covariance(1e-3), e.state_covariance(1e-3)
    p.close(), t.close(), e.close()
    # without weight the factor is not there: the pose and landmark marginals of the plain handle
    fig = _scaled_by(tiny["state"][:, :6, :6], plain["pose"]), _scaled_by(tiny["landmark"], plain["landmark"])
    print(f"FIGURES state cov {name} sigma_dyn=1e-30 against the plain handle: pose {fig[0]:.2e} landmark {fig[1]:.2e}")
    assert fig[0] <= 1e-9 and fig[1] <= 1e-9
    # the factor adds information: no pose marginal widens
    gain = _min_eig_rel(plain["pose"] - c["state"][:, :6, :6])
    # every state block and every pair of consecutive states is a covariance
    joint = np.block([[c["state"][:-1], c["edges"]], [np.swapaxes(c["edges"], 1, 2), c["state"][1:]]])
    psd = _min_eig_rel(c["state"]), _min_eig_rel(joint)
    print(f"FIGURES state cov {name} smallest eigenvalue over largest: plain - dynamics {gain:.2e}, state {psd[0]:.2e}, joint {psd[1]:.2e}")
    assert gain >= -1e-9 and psd[0] >= -1e-9 and psd[1] >= -1e-9


# ------------------------------------------------------------------------------------------------ 7. Python surface
def test_sigmas_and_landmarks_in_the_callers_order():
    from vinsat_amd import schur
    d = V.case("12")
    L = d["X0"].shape[0]
    perm = np.random.default_rng(3).permutation(L)             # new id of landmark l: perm[l]
    q = dict(d)
    q["landmark_of_row"] = perm[d["landmark_of_row"]]
    for k in ("X0", "Xs"):
        q[k] = np.empty_like(d[k])
        q[k][perm] = d[k]
    e = engine(q)
    r = V.reference("12", 0.0)
    c = e.state_covariance(0.0, pairs=True)
    e.close()
    fig = V.scaled(dict(state=c["state"], edges=c["edges"], pairs=c["pairs"][2], landmark=c["landmark"][perm]), r)
    print("FIGURES state cov permuted landmarks " + " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    assert fig["landmark"] <= V.bar(r, "landmark") and fig["state"] <= V.bar(r, "state")
    pos, att, vel = schur.state_sigmas(c)
    dg = np.diagonal(c["state"], axis1=1, axis2=2)
    assert np.array_equal(pos, np.sqrt(dg[:, :3])) and np.array_equal(att, 2.0 * np.sqrt(dg[:, 3:6])) and np.array_equal(vel, np.sqrt(dg[:, 6:]))
    # a variance within the bar is a sigma within half of it
    dr = np.diagonal(r.state, axis1=1, axis2=2)
    for got, ref in ((pos, np.sqrt(dr[:, :3])), (att, 2.0 * np.sqrt(dr[:, 3:6])), (vel, np.sqrt(dr[:, 6:]))):
        assert np.abs(got / ref - 1.0).max() <= V.bar(r, "state")
    assert np.array_equal(schur.landmark_sigmas(c), np.sqrt(np.diagonal(c["landmark"], axis1=1, axis2=2)))
