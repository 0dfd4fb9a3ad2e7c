"""The NumPy block recurrence of the covariance query (tests/cov_oracle.py: the helper the GPU tests use for windows too big for a
dense inverse) against dense inverses of the oracle's system, and the Python helpers that need no device."""
import numpy as np
import pytest

import cov_oracle as C
from oracle import ba_oracle as O


def _resident(cfg):
    from vinsat_amd import od_pipe, synth
    det, orb = synth.make_sequence(cfg)
    win = od_pipe.prepare_window(det, orb)
    st, lam = od_pipe.initial_guess(win), 1e-4
    for it in range(20):
        st, lam, _, _ = O.ba_iteration(it, st, win.cumrot_last, win.landmarks_uv, win.landmarks_xyz, win.ii, win.time_idx,
                                       win.intrinsics, win.confidences, lam, initialize=it < 10)
    d = {}
    O.ba_iteration(19, st, win.cumrot_last, win.landmarks_uv, win.landmarks_xyz, win.ii, win.time_idx, win.intrinsics,
                   win.confidences, lam, initialize=False, debug=d)
    return d["bands"], lam


@pytest.mark.parametrize("cfg", ["C1", "C2"])
def test_block_recurrence_against_the_dense_inverse(cfg):
    """Measured spread of the dense references among themselves after the 20-call schedule (condition ~1e11 on C1, ~6e10 on C2):
    LU inverse vs Cholesky on identity columns 1.6e-9 / 2.1e-9 (C1 undamped / damped) and 7.8e-11 / 2.2e-11 (C2) per-pose block
    error; the recurrence itself 1.0e-9 / 4.0e-10 (C1) and 2.8e-10 / 2.3e-10 (C2).  Bar: 1e-8 (blocks), 1e-8 (sigmas)."""
    bands, lam = _resident(cfg)
    n = bands.shape[0]
    for lam32 in (0.0, float(np.float32(lam))):
        ref = C.marginal_dense(bands, lam32)
        got = C.marginal_blocks(bands, lam32)
        assert C.block_rel_err(got[0], ref[0]) < 1e-8
        assert C.block_rel_err(got[1][:n - 1], ref[1][:n - 1]) < 1e-8
        assert C.sigma_rel_err(got[0], ref[0]) < 1e-8
        assert np.array_equal(got[0], got[0].transpose(0, 2, 1))


def test_symmetrised_matrix_is_symmetric_and_blocks_agree():
    rng = np.random.default_rng(3)
    n = 6
    bands = rng.normal(size=(n, 3, 9, 9))
    A = C.symmetrised_dense(bands, 0.5)
    assert np.array_equal(A, A.T)
    d, s = C.blocks_of(A, n)
    assert np.array_equal(d[2], A[18:27, 18:27]) and np.array_equal(s[4], A[36:45, 45:54]) and not s[n - 1].any()


def test_pose_sigmas_shapes_and_attitude_factor():
    import torch
    from vinsat_amd.ba import pose_sigmas
    cov = np.zeros((2, 5, 9, 9))
    idx = np.arange(9)
    cov[..., idx, idx] = np.arange(1.0, 10.0) ** 2
    pos, vel, att = pose_sigmas(cov)
    assert pos.shape == vel.shape == att.shape == (2, 5, 3)
    assert np.allclose(pos[0, 0], [1, 2, 3]) and np.allclose(att[0, 0], [8, 10, 12]) and np.allclose(vel[0, 0], [7, 8, 9])
    tp, tv, ta = pose_sigmas(torch.from_numpy(cov[:1]))
    assert isinstance(tp, torch.Tensor) and tuple(ta.shape) == (1, 5, 3)
    lst = pose_sigmas([torch.from_numpy(cov[:1, :3]), torch.from_numpy(cov[1:, :2])])
    assert len(lst) == 2 and tuple(lst[1][0].shape) == (1, 2, 3)


def test_covariance_without_a_call_is_an_error():
    from vinsat_amd import ba
    saved = ba._cache.pop("last_query", None)
    try:
        with pytest.raises(RuntimeError):
            ba.covariance()
    finally:
        if saved is not None:
            ba._cache["last_query"] = saved
