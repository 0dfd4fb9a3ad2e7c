"""tests/state_metrics.py: the per-component state bars resolve what the norm-wise rel_err and the arccos angle cannot."""
import numpy as np
import pytest

from conftest import load_golden, rel_err
from state_metrics import assert_states, state_errors


def _states():
    return load_golden("c2")["states_out_19"][0].copy()


def _rotated(st, angle, axis=(0.3, -0.5, 0.8)):
    """Every quaternion of `st` followed by a rotation of `angle` rad about `axis` (q (x) dq)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    dv, dw = a * np.sin(angle / 2), np.cos(angle / 2)
    out = st.copy()
    v, w = st[:, 3:6], st[:, 6]
    out[:, 3:6] = w[:, None] * dv + dw * v + np.cross(v, dv)
    out[:, 6] = w * dw - v @ dv
    return out


@pytest.mark.parametrize("angle", [1e-12, 1e-9, 1e-6])
def test_small_rotations_are_measured(angle):
    st = _states()
    rot = _rotated(st, angle)
    e = state_errors(rot, st)
    assert abs(e[2] - angle) <= 0.01 * angle, e
    assert e[0] == 0.0 and e[1] == 0.0
    # the arccos form the parity tests used cannot see 1e-12 rad: it gives 0 or >= 2e-8
    q, qr = rot[:, 3:7], st[:, 3:7]
    if angle == 1e-12:
        acos = (2 * np.arccos(np.clip(np.abs((q * qr).sum(-1)), 0, 1))).max()
        assert acos == 0.0 or acos >= 2e-8


def test_sign_of_the_quaternion_is_no_rotation():
    st = _states()
    neg = st.copy()
    neg[:, 3:7] *= -1
    assert state_errors(neg, st)[2] == 0.0
    assert_states(neg, st, 0.0, 0.0, 0.0, "q vs -q")


def test_velocity_error_that_rel_err_lets_through_fails_the_velocity_bar():
    st = _states()
    bad = st.copy()
    bad[:, 7:] *= 1 + 1e-5
    assert rel_err(bad, st) < 1e-6                  # hidden behind max|ref| ~ 7000 km
    e = state_errors(bad, st)
    assert 0.9e-5 < e[1] < 1.1e-5 and e[0] == 0.0
    with pytest.raises(AssertionError):
        assert_states(bad, st, 1e-6, 1e-6, 1e-6, "velocity 1e-5")


def test_position_error_is_relative_to_the_positions():
    st = _states()
    bad = st.copy()
    bad[3, 1] += 1e-3 * np.abs(st[:, :3]).max()
    e = state_errors(bad, st)
    assert abs(e[0] - 1e-3) < 1e-9 and e[1] == 0.0 and e[2] == 0.0
