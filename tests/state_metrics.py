"""Per-component distance of a state array [n, 10] (pos 0:3, quat xyzw 3:7, vel 7:10) from a reference.

``conftest.rel_err`` takes max|d| / max|ref| over the whole 10-vector, and max|ref| is a position of ~7000 km: a bar of 1e-6
on it lets a velocity be off by 7e-3 km/s and a quaternion by 7e-3.  Here every component answers to its own scale, and the
attitude error is the angle of q^-1 (x) q_ref taken with atan2, which resolves angles far below the sqrt(eps) ~ 3e-8 rad that
2 arccos(|q . q_ref|) bottoms out at.

STATE_METRICS_LOG (environment): a file that every ``assert_states`` appends its three numbers to (what the suite observed)."""
import os

import numpy as np


def state_errors(st, ref):
    """(position max-rel, velocity max-rel, attitude angle in rad), each the worst over the window."""
    st = np.asarray(st, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    pos = np.abs(st[:, :3] - ref[:, :3]).max() / np.abs(ref[:, :3]).max()
    vel = np.abs(st[:, 7:] - ref[:, 7:]).max() / np.abs(ref[:, 7:]).max()
    q, qr = st[:, 3:7], ref[:, 3:7]     # (x, y, z, w)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    qr = qr / np.linalg.norm(qr, axis=1, keepdims=True)
    # q^-1 (x) q_ref: vector part and scalar part
    w1, v1 = q[:, 3], -q[:, :3]
    w2, v2 = qr[:, 3], qr[:, :3]
    w = w1 * w2 - (v1 * v2).sum(1)
    v = w1[:, None] * v2 + w2[:, None] * v1 + np.cross(v1, v2)
    ang = 2 * np.arctan2(np.linalg.norm(v, axis=1), np.abs(w))
    return float(pos), float(vel), float(ang.max())


def assert_states(st, ref, pos, vel, att, what=None):
    """Position and velocity max-rel within `pos` / `vel`, attitude angle within `att` rad; returns the three errors."""
    e = state_errors(st, ref)
    log = os.environ.get("STATE_METRICS_LOG")
    if log:
        with open(log, "a") as f:
            f.write(f"{e[0]:.3e} {e[1]:.3e} {e[2]:.3e} {what!r}\n")
    assert e[0] <= pos and e[1] <= vel and e[2] <= att, (what, e, (pos, vel, att))
    return e
