"""Free-landmark bundle adjustment with a Schur-complement solve on the GPU -- ADD-ON, PARITY UNPINNED.

The reference (CMUAbstract/VINSat) keeps its landmarks fixed (``estimation/BA/BA_filtering.py:32-37``): there is nothing to
marginalise and no counterpart of this module in it.  This is the variant BASELINE.json's north_star describes on top of the
reference's reprojection model: the landmarks become unknowns (3 each, held by a catalogue prior ``N(X0, sigma^2 I)``), the
landmark blocks are eliminated (3x3 inversions), and the dense reduced camera system is factorised on the matrix cores
(``vinsat_amd/csrc/vba_schur*.hip``, one unit per stage; ``vba_schur.hip`` heads them with the map).  It is validated against ``oracle/schur_oracle.py`` -- this repository's own CPU
restatement -- only, and it never runs inside :func:`vinsat_amd.ba.BA`.  Opt-in per handle (``time_idx=``, ``sigma_dyn=``) the
reference's J2 orbit factor ties consecutive poses and the velocities become unknowns (``vinsat_amd/csrc/vba_schur_dyn.hip``,
DESIGN 9.5).  On top of that, opt-in too (``cumrot=``, ``sigma_att=``), a Gauss-Newton statement of the reference's attitude term
ties consecutive attitudes through the gyro's gap rotations (``vinsat_amd/csrc/vba_schur_att.hip``).

Host side (this file): the static structure of a window -- rows sorted by landmark, the rows of each pose, and for every
6x6 block of the reduced system the list of row pairs that share a landmark -- is built once with NumPy and uploaded.
"""
from __future__ import annotations

import ctypes
from ctypes import byref, c_double, c_float, c_int, c_void_p

import numpy as np

from . import _lib
from ._lib import PD


# fit[8] of vba_schur_reliability, in its order
FIT_NAMES = ("omega", "m_eff", "t_rows", "t_prior", "rho", "s0sq", "max_wtest", "max_lm_wtest")
# fit[10] of vba_schur_reliability_dyn: the same eight, then the edges' share of the traces and of the cost
FIT_NAMES_DYN = FIT_NAMES + ("t_edges", "omega_edges")
# fit[13] of vba_schur_reliability_att: the same ten, then the attitude edges' share of the traces and of the cost and their largest test
FIT_NAMES_ATT = FIT_NAMES_DYN + ("t_att", "omega_att", "max_att_wtest")
# the four slots vba_schur_outlier_power(_dyn, _att) puts behind the fit of the reliability query, and its arrays in the order of the entry
POWER_FIT_NAMES = ("n_rows_over_crit", "max_ext_pos", "n_lm_over_crit", "max_lm_del_pos")
POWER_ROW_KEYS = ("mdb", "ext_pos", "ext_att", "ext_lm", "del_pos", "del_lm")
POWER_LM_KEYS = ("lm_mdb", "lm_ext", "lm_del_pos")


def alpha_schedule(it):
    """The reference's robustness schedule (``BA_filtering.py:22``): 2 for the first calls, 1 from the fifth on."""
    return min(max(1 - (2 * (it / 5) - 1), 1), 2)


def median(keys, device=0):
    """``vba_schur_median``: the lower median (rank ``(count - 1) // 2``) of non-negative float64 keys by the select kernels of
    :meth:`SchurBA.reweight`, bit for bit ``numpy.sort(keys)[(count - 1) // 2]``."""
    lib = _lib.load()
    k = np.ascontiguousarray(keys, dtype=np.float64).reshape(-1)
    out = c_double()
    rc = lib.vba_schur_median(int(device), k.ctypes.data_as(PD), k.size, byref(out))
    if rc != 0:
        msg = lib.vba_schur_last_error()
        raise _lib.VbaError(f"libvinsat_ba (schur) error {rc}: {msg.decode() if msg else ''}")
    return out.value


def build_structure(pose_of_row, landmark_of_row, n, L):
    """Static index structure of a window (see ``include/vinsat_ba.h``, ``vba_schur_upload``).

    Returns ``(order, s)``: ``order`` sorts the caller's rows by (landmark, pose); ``s`` holds the int32 arrays ``lm_ptr,
    row_pose, row_lm, pose_ptr, pose_rows, blk_i, blk_j, blk_ptr, pair_k, pair_k2`` over the SORTED rows.
    """
    pose_of_row = np.asarray(pose_of_row, dtype=np.int64)
    landmark_of_row = np.asarray(landmark_of_row, dtype=np.int64)
    m = pose_of_row.size
    if landmark_of_row.size != m:
        raise ValueError("pose_of_row and landmark_of_row disagree on the number of rows")
    if m == 0 or pose_of_row.min() < 0 or pose_of_row.max() >= n or landmark_of_row.min() < 0 or landmark_of_row.max() >= L:
        raise ValueError("row indices out of range")
    order = np.lexsort((pose_of_row, landmark_of_row))
    rp, rl = pose_of_row[order], landmark_of_row[order]
    if np.any((rp[1:] == rp[:-1]) & (rl[1:] == rl[:-1])):
        raise ValueError("a landmark is observed twice from one pose")
    lm_ptr = np.zeros(L + 1, dtype=np.int64)
    np.add.at(lm_ptr, rl + 1, 1)
    lm_ptr = np.cumsum(lm_ptr)
    pose_rows = np.argsort(rp, kind="stable")
    pose_ptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(pose_ptr, rp + 1, 1)
    pose_ptr = np.cumsum(pose_ptr)
    # row pairs (k, k') of one landmark with pose(k) >= pose(k'): rows of a landmark are sorted by pose, so k >= k'
    cnt = np.diff(lm_ptr)
    npairs = int((cnt * (cnt + 1) // 2).sum())
    if npairs > 400_000_000:
        raise ValueError(f"{npairs} row pairs: tracks this long are not a bundle-adjustment window (check the visibility model)")
    ks, k2s = [], []
    for t in np.unique(cnt):
        if t == 0:
            continue
        starts = lm_ptr[:-1][cnt == t]
        a, b = np.tril_indices(int(t))
        ks.append((starts[:, None] + a[None, :]).ravel())
        k2s.append((starts[:, None] + b[None, :]).ravel())
    pk, pk2 = np.concatenate(ks), np.concatenate(k2s)
    bi, bj = rp[pk], rp[pk2]
    # every diagonal block exists (it holds B_i) even for a pose without rows
    key = bi * n + bj
    diag = np.arange(n, dtype=np.int64) * (n + 1)
    blocks = np.unique(np.concatenate([key, diag]))
    srt = np.argsort(key, kind="stable")            # pairs grouped by block, fixed order inside a block
    pk, pk2, key = pk[srt], pk2[srt], key[srt]
    blk_ptr = np.searchsorted(key, np.concatenate([blocks, [blocks[-1] + 1]]), side="left")
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    s = dict(lm_ptr=i32(lm_ptr), row_pose=i32(rp), row_lm=i32(rl), pose_ptr=i32(pose_ptr), pose_rows=i32(pose_rows),
             blk_i=i32(blocks // n), blk_j=i32(blocks % n), blk_ptr=i32(blk_ptr), pair_k=i32(pk), pair_k2=i32(pk2))
    return order, s


class SchurBA:
    """Device-resident free-landmark BA problem: ``n`` poses, ``L`` landmarks, ``m`` observation rows."""

    def __init__(self, states, landmarks0, uv, weights, pose_of_row, landmark_of_row, intrinsics, sigma_prior=0.05, device=0,
                 time_idx=None, sigma_dyn=None, cumrot=None, sigma_att=None, long_gaps=False, state_prior=None):
        """``time_idx [n]`` (the second of every pose) and ``sigma_dyn`` together switch on the orbit-dynamics factor with the
        velocities as unknowns (``vba_schur_enable_dynamics`` in ``include/vinsat_ba.h``: gaps of 1 .. 64 s); with neither the
        handle is the purely visual bundle adjustment.  ``long_gaps=True`` (with both) switches it on through
        ``vba_schur_enable_dynamics_long`` instead: gaps up to ``VBA_MAX_GAP`` seconds, the window of a later pass of a sequence;
        edges of more than 64 s are propagated parallel in time (:meth:`long_edges` names them), everything else is as it was.  ``cumrot [n,4]`` (the rotation accumulated over the gap after every pose,
        scalar last, as ``od_pipe.gap_rotations`` gives it; the last row is ignored) and ``sigma_att`` together add the
        Gauss-Newton attitude factor on such a handle (``vba_schur_enable_attitude``); ``sigma_att = sigma_dyn * QUAT_COEFF / 2``
        weights the attitude as the reference does near the solution.  ``state_prior = (pose_idx [count], anchors [count,10],
        infos [count,9,9])`` puts a Gaussian prior on the 9-DoF state ``[dp, dtheta, dv]`` of the chosen poses of a handle with the
        dynamics factor (``vba_schur_enable_state_prior``); :func:`prior_for_first_pose` makes one from the
        :meth:`handoff` of the window before."""
        if state_prior is not None and time_idx is None:
            raise ValueError("the state prior is only valid together with time_idx and sigma_dyn")
        if (time_idx is None) != (sigma_dyn is None):
            raise ValueError("time_idx and sigma_dyn switch on the dynamics factor together: give both or neither")
        if (cumrot is None) != (sigma_att is None):
            raise ValueError("cumrot and sigma_att switch on the attitude factor together: give both or neither")
        if long_gaps and time_idx is None:
            raise ValueError("long_gaps is an option of the dynamics factor: give time_idx and sigma_dyn with it")
        if cumrot is not None and time_idx is None:
            raise ValueError("the attitude factor (cumrot, sigma_att) is only valid together with time_idx and sigma_dyn")
        self.lib = _lib.load()
        states = np.ascontiguousarray(states, dtype=np.float64).reshape(-1, 10)
        X0 = np.ascontiguousarray(landmarks0, dtype=np.float64).reshape(-1, 3)
        self.n, self.L = states.shape[0], X0.shape[0]
        self.order, s = build_structure(pose_of_row, landmark_of_row, self.n, self.L)
        self.m = self.order.size
        uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)[self.order]
        w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1)[self.order])
        K = np.ascontiguousarray(intrinsics, dtype=np.float64).reshape(-1, 4)
        if K.shape[0] != self.n:
            raise ValueError("intrinsics need one row per pose")
        self.structure = s
        self.h = c_void_p()
        self._check(self.lib.vba_schur_create(device, self.n, self.m, self.L, int(s["blk_i"].size), int(s["pair_k"].size), byref(self.h)))
        u, v = np.ascontiguousarray(uv[:, 0]), np.ascontiguousarray(uv[:, 1])
        p = lambda a: a.ctypes.data_as(c_void_p)
        self._check(self.lib.vba_schur_upload(self.h, p(s["lm_ptr"]), p(s["row_pose"]), p(s["row_lm"]), p(u), p(v), p(w), p(s["pose_ptr"]),
                                              p(s["pose_rows"]), p(s["blk_i"]), p(s["blk_j"]), p(s["blk_ptr"]), p(s["pair_k"]), p(s["pair_k2"]),
                                              p(K), p(X0), float(sigma_prior)))
        self.dynamics = time_idx is not None
        if self.dynamics:
            t = np.ascontiguousarray(time_idx, dtype=np.int32).reshape(-1)
            try:
                if t.size != self.n:
                    raise ValueError("time_idx needs one entry per pose")
                enable = self.lib.vba_schur_enable_dynamics_long if long_gaps else self.lib.vba_schur_enable_dynamics
                self._check(enable(self.h, t.ctypes.data_as(ctypes.POINTER(c_int)), float(sigma_dyn)))
            except Exception:
                self.close()
                raise
        self.attitude = cumrot is not None
        if self.attitude:
            try:
                c = np.ascontiguousarray(cumrot, dtype=np.float64)
                if c.shape != (self.n, 4):
                    raise ValueError("cumrot needs one quaternion per pose")
                self._check(self.lib.vba_schur_enable_attitude(self.h, c.ctypes.data_as(PD), float(sigma_att)))
            except Exception:
                self.close()
                raise
        self.prior_count = 0
        if state_prior is not None:
            try:
                idx, anchors, infos = state_prior
                idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
                an = np.ascontiguousarray(anchors, dtype=np.float64)
                lam = np.ascontiguousarray(infos, dtype=np.float64)
                if an.shape != (idx.size, 10) or lam.shape != (idx.size, 9, 9):
                    raise ValueError("state_prior needs one anchor [10] and one information matrix [9, 9] per index")
                self._check(self.lib.vba_schur_enable_state_prior(self.h, int(idx.size), idx.ctypes.data_as(ctypes.POINTER(c_int)),
                                                                  an.ctypes.data_as(PD), lam.ctypes.data_as(PD)))
                self.prior_count = int(idx.size)
            except Exception:
                self.close()
                raise
        self.set_state(states, X0)

    def _check(self, rc):
        if rc != 0:
            msg = self.lib.vba_schur_last_error()
            raise _lib.VbaError(f"libvinsat_ba (schur) error {rc}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.vba_schur_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_state(self, states, landmarks):
        s = np.ascontiguousarray(states, dtype=np.float64).reshape(self.n, 10)
        X = np.ascontiguousarray(landmarks, dtype=np.float64).reshape(self.L, 3)
        self._check(self.lib.vba_schur_set_state(self.h, s.ctypes.data_as(PD), X.ctypes.data_as(PD)))

    def get_state(self):
        s, X = np.empty((self.n, 10)), np.empty((self.L, 3))
        self._check(self.lib.vba_schur_get_state(self.h, s.ctypes.data_as(PD), X.ctypes.data_as(PD)))
        return s, X

    def iterate(self, lamda):
        """One LM trial; returns ``(cost_before, cost_after, accepted)``."""
        c0, c1, acc = c_double(), c_double(), c_int()
        self._check(self.lib.vba_schur_iterate(self.h, float(lamda), byref(c0), byref(c1), byref(acc)))
        return c0.value, c1.value, bool(acc.value)

    def last_info(self):
        """0 if the last factorisation went through, else 1 + the row at which it first met a non-positive pivot."""
        v = c_int()
        self._check(self.lib.vba_schur_last_info(self.h, byref(v)))
        return v.value

    def last_ms(self):
        a, b, c = c_float(), c_float(), c_float()
        self._check(self.lib.vba_schur_last_ms(self.h, byref(a), byref(b), byref(c)))
        return dict(build=a.value, factor=b.value, solve=c.value)

    def last_trial_cost_ms(self):
        """Milliseconds of the cost kernels of the last trial (``vba_schur_last_trial_cost_ms``), beside :meth:`last_ms`."""
        v = c_float()
        self._check(self.lib.vba_schur_last_trial_cost_ms(self.h, byref(v)))
        return v.value

    def last_step(self):
        """``(dc [n,6], dl [L,3])`` of the last iterate."""
        out = np.empty(6 * self.n + 3 * self.L)
        self._check(self.lib.vba_schur_debug_fetch(self.h, 0, out.ctypes.data_as(PD), out.size))
        return out[: 6 * self.n].reshape(self.n, 6), out[6 * self.n:].reshape(self.L, 3)

    def _dynamics_fetch(self, what, shape):
        out = np.empty(shape)
        self._check(self.lib.vba_schur_debug_fetch(self.h, what, out.ctypes.data_as(PD), out.size))
        return out

    def last_velocity_step(self):
        """``dv [n,3]`` of the last iterate (a handle with the dynamics factor)."""
        return self._dynamics_fetch(3, (self.n, 3))

    def dynamics_residual(self):
        """``r [n-1,6]`` of the edges at the state the last iterate started from (a handle with the dynamics factor)."""
        return self._dynamics_fetch(4, (self.n - 1, 6))

    def dynamics_jacobian(self):
        """``D Phi [n-1,6,6]`` of the edges at the state the last iterate started from (a handle with the dynamics factor)."""
        return self._dynamics_fetch(5, (self.n - 1, 6, 6))

    def dynamics_edge_cost(self):
        """``sigma_dyn |r|^2 [n-1]``: the edges' shares of the cost at the state the last iterate started from."""
        return self._dynamics_fetch(6, (self.n - 1,))

    def long_edges(self):
        """The poses ``i`` whose edge ``i -> i + 1`` is propagated parallel in time (``vba_schur_long_edges``): the gaps of more than
        64 s of a handle built with ``long_gaps=True``; empty on any other handle with the dynamics factor."""
        cnt = c_int()
        self._check(self.lib.vba_schur_long_edges(self.h, None, 0, byref(cnt)))
        idx = np.zeros(cnt.value, dtype=np.int32)
        if cnt.value:
            self._check(self.lib.vba_schur_long_edges(self.h, idx.ctypes.data_as(ctypes.POINTER(c_int)), cnt.value, byref(cnt)))
        return idx

    def attitude_residual(self):
        """``a [n-1,3]`` of the edges at the state the last iterate started from (a handle with the attitude factor)."""
        return self._dynamics_fetch(7, (self.n - 1, 3))

    def attitude_jacobian(self):
        """``[n-1,2,3,3]``: ``d a_i / d theta_i``, then ``d a_i / d theta_{i+1}``, of the edges at the state the last iterate
        started from (a handle with the attitude factor)."""
        return self._dynamics_fetch(8, (self.n - 1, 2, 3, 3))

    def attitude_edge_cost(self):
        """``sigma_att |a|^2 [n-1]``: the edges' shares of the cost at the state the last iterate started from."""
        return self._dynamics_fetch(9, (self.n - 1,))

    def prior_residual(self):
        """``e [count,9]`` of the state priors at the state the last iterate started from (a handle with the state prior)."""
        return self._dynamics_fetch(10, (self.prior_count, 9))

    def prior_jacobian(self):
        """``J [count,3,3] = d (2 s eps) / d theta`` of the state priors at the state the last iterate started from."""
        return self._dynamics_fetch(11, (self.prior_count, 3, 3))

    def prior_cost(self):
        """``e^T Lambda e [count]``: the priors' shares of the cost at the state the last iterate started from."""
        return self._dynamics_fetch(12, (self.prior_count,))

    def handoff(self, steps, cumrot_gap, process_noise=None, lamda=0.0, strict=True):
        """``vba_schur_handoff`` at the resident state of a handle with the dynamics factor (``include/vinsat_ba.h``): the marginal
        of the last pose propagated over ``steps`` seconds -- ``cumrot_gap [4]`` the rotation accumulated over them, scalar last,
        ``process_noise [3]`` variances per second of position, attitude and velocity -- into what the next window's prior takes.
        Returns ``dict(anchor [10], info [9,9], status)``; ``status``: 0, ``1 +`` the row of a non-positive pivot of the covariance
        query, or -1 if the propagated covariance is not positive definite.  ``strict``: a non-zero status raises ``VbaError``;
        without it the arrays come back filled with NaN.  Nothing on the handle changes."""
        c = np.ascontiguousarray(cumrot_gap, dtype=np.float64).reshape(4)
        q = None if process_noise is None else np.ascontiguousarray(process_noise, dtype=np.float64).reshape(3)
        anchor, info, status = np.empty(10), np.empty((9, 9)), c_int()
        self._check(self.lib.vba_schur_handoff(self.h, float(lamda), int(steps), c.ctypes.data_as(PD), None if q is None else q.ctypes.data_as(PD),
                                               anchor.ctypes.data_as(PD), info.ctypes.data_as(PD), byref(status)))
        if status.value != 0 and strict:
            if status.value < 0:
                raise _lib.VbaError("schur handoff: the propagated covariance is not positive definite")
            raise self._not_positive_definite("handoff", "reduced system", lamda, status.value)
        return dict(anchor=anchor, info=info, status=status.value)

    def last_handoff_ms(self):
        return self._last_ms("vba_schur_last_handoff_ms")

    def cholesky_factor(self):
        """The factor of the last iterate, dense lower triangular: ``[6n, 6n]``, or ``[9n, 9n]`` over ``[pose | velocity]``
        unknowns on a handle with the dynamics factor."""
        N = (9 if self.dynamics else 6) * self.n
        out = np.empty((N, N))
        self._check(self.lib.vba_schur_debug_fetch(self.h, 1, out.ctypes.data_as(PD), out.size))
        return out

    def covariance(self, lamda=0.0, pairs=False, strict=True):
        """``vba_schur_covariance`` at the resident state (``include/vinsat_ba.h``): blocks of the inverse of the system an
        ``iterate(lamda)`` would build there.  Returns a dict: ``pose [n,6,6]`` -- every pose's marginal over all landmarks and
        all other poses, coordinates ``[dp (km), dtheta]`` -- ``landmark [L,3,3]`` in the caller's landmark order, ``info``,
        and with ``pairs`` also ``pairs = (blk_i, blk_j, [nblk,6,6])``: the cross-covariances of the poses that share a
        landmark (``i >= j``, diagonal blocks included).  Up to the variance factor of the weights.  State, step, factor and
        the bits of the following iterates are not changed.

        A system that is not positive definite at this damping raises ``VbaError`` naming the row (``info - 1``); with
        ``strict=False`` the arrays come back filled with NaN instead."""
        pose, lm = np.empty((self.n, 6, 6)), np.empty((self.L, 3, 3))
        blocks = np.empty((self.structure["blk_i"].size, 6, 6)) if pairs else None
        info = c_int()
        self._check(self.lib.vba_schur_covariance(self.h, float(lamda), pose.ctypes.data_as(PD), blocks.ctypes.data_as(PD) if pairs else None,
                                                  lm.ctypes.data_as(PD), byref(info)))
        if info.value != 0 and strict:
            raise _lib.VbaError(f"schur covariance: the reduced camera system is not positive definite at lamda = {lamda:g} "
                                f"(non-positive pivot at row {info.value - 1})")
        out = dict(pose=pose, landmark=lm, info=info.value)
        if pairs:
            out["pairs"] = (self.structure["blk_i"].copy(), self.structure["blk_j"].copy(), blocks)
        return out

    def last_covariance_ms(self):
        return self._last_ms("vba_schur_last_covariance_ms")

    def state_covariance(self, lamda=0.0, pairs=False, strict=True):
        """``vba_schur_covariance_dyn`` at the resident state of a handle with the dynamics factor (``include/vinsat_ba.h``):
        blocks of the inverse of the system an ``iterate(lamda)`` would build there.  Returns a dict: ``state [n,9,9]`` -- every
        pose's marginal, coordinates ``[dp (km), dtheta, dv (km/s)]`` as ``vba_covariance`` orders them -- ``edges [n-1,9,9]`` =
        ``Sigma(x_i, x_{i+1})`` (rows of pose ``i``, columns of pose ``i + 1``), ``landmark [L,3,3]`` in the caller's landmark
        order, ``info``, and with ``pairs`` also ``pairs = (blk_i, blk_j, [nblk,6,6])`` as :meth:`covariance` returns them.  Up to
        the variance factor of the weights.  Nothing on the handle changes: state, step, factor, the dynamics arrays of the last
        iterate and the bits of the following iterates.  On a handle with the attitude factor the system includes it (and a window
        with a pose without rows is positive definite at ``lamda = 0``).

        ``strict`` as in :meth:`covariance`: a system that is not positive definite raises ``VbaError`` naming the row
        (``info - 1``), or gives NaN everywhere.  A handle without the dynamics factor raises: :meth:`covariance` is its query."""
        state, edges, lm = np.empty((self.n, 9, 9)), np.empty((max(self.n - 1, 0), 9, 9)), np.empty((self.L, 3, 3))
        blocks = np.empty((self.structure["blk_i"].size, 6, 6)) if pairs else None
        info = c_int()
        self._check(self.lib.vba_schur_covariance_dyn(self.h, float(lamda), state.ctypes.data_as(PD), edges.ctypes.data_as(PD),
                                                      blocks.ctypes.data_as(PD) if pairs else None, lm.ctypes.data_as(PD), byref(info)))
        if info.value != 0 and strict:
            raise _lib.VbaError(f"schur state covariance: the reduced system is not positive definite at lamda = {lamda:g} "
                                f"(non-positive pivot at row {info.value - 1})")
        out = dict(state=state, edges=edges, landmark=lm, info=info.value)
        if pairs:
            out["pairs"] = (self.structure["blk_i"].copy(), self.structure["blk_j"].copy(), blocks)
        return out

    def last_state_covariance_ms(self):
        return self._last_ms("vba_schur_last_covariance_dyn_ms")

    def reliability(self, lamda=0.0, strict=True):
        """``vba_schur_reliability`` at the resident state (``include/vinsat_ba.h``): which row, and which catalogue position,
        the window contradicts.  Returns a dict: ``leverage [m]`` (trace of the row's 2x2 block of the hat matrix, poses AND
        landmark free) and ``wtest [m]`` in the CALLER's row order; ``lm_leverage [L]`` / ``lm_wtest [L]``, the same for the
        catalogue prior of every landmark taken as an observation; ``lm_stats [L,3]`` and ``pose_stats [n,3]`` = (sum of
        leverage, largest finite wtest, rows with ``w > 0``) per landmark / pose; ``fit``, a dict of :data:`FIT_NAMES`; ``info``.
        Up to the variance factor of the weights (``fit["s0sq"]`` estimates it).  Nothing on the handle changes.

        ``strict`` as in :meth:`covariance`: a system that is not positive definite raises, or gives NaN everywhere."""
        return self._reliability("plain", lamda, strict)

    def last_reliability_ms(self):
        return self._last_ms("vba_schur_last_reliability_ms")

    def snoop(self, lamda=0.0, crit=3.29, scaled=True, min_rows=6, min_track=3, strict=True):
        """``vba_schur_snoop`` at the resident state (``include/vinsat_ba.h`` states the rule): the device part of
        :meth:`reliability`, then at most one rejection per group, on the device.  A rejected row gets weight 0 in place; a
        rejected catalogue entry leaves the window (every weighted row of the landmark gets weight 0; its prior holds it at
        ``X0``).  ``crit`` is in units of the w-test, times ``sqrt(s0sq)`` of the device's own fit with ``scaled``; a pose keeps
        at least ``min_rows`` weighted rows, and a catalogue entry is only tested on tracks of at least ``min_track`` weighted
        rows.  Returns a dict: ``rows`` (rejected by their own test), ``landmarks``, ``rows_via_landmarks`` of THIS call,
        ``crit_used``, ``info``.  :meth:`rejected` gives the cumulative masks, :meth:`restore_rejected` undoes everything.

        ``strict`` as in :meth:`reliability`: a system that is not positive definite raises, or rejects nothing and tells ``info``."""
        return self._snoop("plain", lamda, crit, scaled, min_rows, min_track, strict)

    def rejected(self):
        """``(row_mask [m] bool in the CALLER's row order, landmark_mask [L] bool)``: everything :meth:`snoop` rejected on this
        handle so far (rows of rejected landmarks included in the row mask)."""
        rows, lms = np.zeros(self.m, dtype=np.uint8), np.zeros(self.L, dtype=np.uint8)
        self._check(self.lib.vba_schur_rejected(self.h, rows.ctypes.data_as(c_void_p), lms.ctypes.data_as(c_void_p), None))
        back = np.zeros(self.m, dtype=bool)
        back[self.order] = rows != 0                    # device rows are sorted by landmark
        return back, lms != 0

    def restore_rejected(self):
        """The weights :meth:`snoop` zeroed come back and both masks are cleared: the handle behaves as one that never snooped."""
        self._check(self.lib.vba_schur_snoop_restore(self.h))

    def last_snoop_ms(self):
        return self._last_ms("vba_schur_last_snoop_ms")

    def state_reliability(self, lamda=0.0, strict=True):
        """``vba_schur_reliability_dyn`` at the resident state of a handle with the dynamics factor (``include/vinsat_ba.h``): the
        dict of :meth:`reliability` -- rows in the CALLER's order, every leverage and test from the covariance of the system WITH
        the factor -- plus ``edge_leverage [n-1]`` (trace of the edge's 6x6 block of the hat matrix, in ``(0, 6]``) and
        ``edge_omega [n-1]`` (``sigma_dyn |r|^2``); ``fit`` is a dict of :data:`FIT_NAMES_DYN`, its ``rho`` and ``omega`` count the
        edges.  There is no w-test of an edge (the header says why).  :func:`suspects` reads the dict unchanged.  Nothing on the
        handle changes.

        ``strict`` as in :meth:`state_covariance`.  A handle without the dynamics factor raises: :meth:`reliability` is its query.
        A handle with the attitude factor raises too, as do :meth:`state_snoop` and :meth:`state_outlier_power`: their redundancy
        counts and edge leverages do not know the attitude equations."""
        return self._reliability("state", lamda, strict)

    def last_state_reliability_ms(self):
        return self._last_ms("vba_schur_last_reliability_dyn_ms")

    def state_snoop(self, lamda=0.0, crit=3.29, scaled=True, min_rows=6, min_track=3, strict=True):
        """``vba_schur_snoop_dyn``: :meth:`snoop` on a handle with the dynamics factor -- the same rule, arguments and result, fed
        by the device part of :meth:`state_reliability`.  Edges are never rejected; :meth:`rejected` and :meth:`restore_rejected`
        serve both."""
        return self._snoop("state", lamda, crit, scaled, min_rows, min_track, strict)

    def last_state_snoop_ms(self):
        return self._last_ms("vba_schur_last_snoop_dyn_ms")

    # Kind of handle -- the plain one, one with the dynamics factor, one with the attitude factor too -> what its three uncertainty queries
    # differ in: the fit names of its reliability query, that query's arrays beyond the common six (each [n - 1]), the suffix of its C
    # entries (vba_schur_reliability<suffix>, vba_schur_snoop<suffix>, vba_schur_outlier_power<suffix>), the label of its error messages,
    # and what the messages of its reliability query and its snoop call the system.
    _KINDS = {"plain": (FIT_NAMES, (), "", "", "reduced camera system"),
              "state": (FIT_NAMES_DYN, ("edge_leverage", "edge_omega"), "_dyn", "state ", "reduced system"),
              "attitude": (FIT_NAMES_ATT, ("edge_leverage", "edge_omega", "att_leverage", "att_wtest", "att_omega"), "_att", "attitude ", "reduced system")}

    def _last_ms(self, entry_name):
        """The milliseconds one of the ``vba_schur_last_*_ms`` entries reports."""
        v = c_float()
        self._check(getattr(self.lib, entry_name)(self.h, byref(v)))
        return v.value

    def _not_positive_definite(self, what, system, lamda, info):
        return _lib.VbaError(f"schur {what}: the {system} is not positive definite at lamda = {lamda:g} (non-positive pivot at row {info - 1})")

    def _finish(self, out, row_keys, names, fit, info):
        """Rows back to the caller's order (device rows are sorted by landmark), ``fit`` as a dict of ``names``, ``info``."""
        for key in row_keys:
            back = np.empty(self.m)
            back[self.order] = out[key]
            out[key] = back
        out["fit"] = dict(zip(names, fit.tolist()))
        out["info"] = info
        return out

    def _reliability(self, kind, lamda, strict):
        """``kind``: a key of ``_KINDS``."""
        names, extra, suffix, label, system = self._KINDS[kind]
        out = dict(leverage=np.empty(self.m), wtest=np.empty(self.m), lm_leverage=np.empty(self.L), lm_wtest=np.empty(self.L),
                   lm_stats=np.empty((self.L, 3)), pose_stats=np.empty((self.n, 3)))
        out.update({k: np.empty(max(self.n - 1, 0)) for k in extra})
        fit, info = np.empty(len(names)), c_int()
        entry = getattr(self.lib, "vba_schur_reliability" + suffix)
        self._check(entry(self.h, float(lamda), *[a.ctypes.data_as(PD) for a in out.values()], fit.ctypes.data_as(PD), byref(info)))
        if info.value != 0 and strict:
            raise self._not_positive_definite(label + "reliability", system, lamda, info.value)
        return self._finish(out, ("leverage", "wtest"), names, fit, info.value)

    def _snoop(self, kind, lamda, crit, scaled, min_rows, min_track, strict):
        """``kind``: a key of ``_KINDS``."""
        _, _, suffix, label, system = self._KINDS[kind]
        counts, used, info = (c_int * 3)(), c_double(), c_int()
        entry = getattr(self.lib, "vba_schur_snoop" + suffix)
        self._check(entry(self.h, float(lamda), float(crit), int(bool(scaled)), int(min_rows), int(min_track), counts, byref(used), byref(info)))
        if info.value != 0 and strict:
            raise self._not_positive_definite(label + "snoop", system, lamda, info.value)
        return dict(rows=counts[0], landmarks=counts[1], rows_via_landmarks=counts[2], crit_used=used.value, info=info.value)

    def _outlier_power(self, kind, lamda, ncp, crit, strict):
        """``kind``: a key of ``_KINDS``."""
        lead, _, suffix, label, _ = self._KINDS[kind]
        names = lead + POWER_FIT_NAMES
        out = {k: np.empty(self.m) for k in POWER_ROW_KEYS}
        out.update({k: np.empty(self.L) for k in POWER_LM_KEYS})
        out["pose_fit"] = np.empty((self.n, 4))
        fit, info = np.empty(len(names)), c_int()
        entry = getattr(self.lib, "vba_schur_outlier_power" + suffix)
        self._check(entry(self.h, float(lamda), float(ncp), float(crit), *[a.ctypes.data_as(PD) for a in out.values()], fit.ctypes.data_as(PD),
                          byref(info)))
        if info.value != 0 and strict:
            raise self._not_positive_definite(label + "outlier power", "reduced system", lamda, info.value)
        return self._finish(out, POWER_ROW_KEYS, names, fit, info.value)

    def outlier_power(self, lamda=0.0, ncp=17.075, crit=3.29, strict=True):
        """``vba_schur_outlier_power`` at the resident state (``include/vinsat_ba.h`` defines every figure): how large an error in a
        row or in a catalogue entry passes the w-test of :meth:`reliability` unnoticed, and how far it moves the fit.  Returns a
        dict: per row, in the CALLER's order, ``mdb [m]`` (px), ``ext_pos`` (km), ``ext_att`` (rad), ``ext_lm`` (km) -- the
        detectable bias and what an undetected one does to the pose's position, its attitude and the row's landmark -- and
        ``del_pos``, ``del_lm`` (km), the moves if the row is deleted; per landmark ``lm_mdb [L]``, ``lm_ext``, ``lm_del_pos`` (km):
        the detectable catalogue error, what it does to the landmark's estimate, and how far the worst-hit pose moves if the prior
        is taken away; ``pose_fit [n,4]`` = (cost share, sum of leverage, largest finite ``ext_pos``, rows with ``wtest > crit``);
        ``fit``, a dict of :data:`FIT_NAMES` then :data:`POWER_FIT_NAMES`; ``info``.  ``ncp`` is the non-centrality of the test at
        the chosen power.  Up to the variance factor of the weights (:func:`scaled_power`).  Nothing on the handle changes.

        ``strict`` as in :meth:`reliability`."""
        return self._outlier_power("plain", lamda, ncp, crit, strict)

    def last_outlier_power_ms(self):
        return self._last_ms("vba_schur_last_outlier_power_ms")

    def state_outlier_power(self, lamda=0.0, ncp=17.075, crit=3.29, strict=True):
        """``vba_schur_outlier_power_dyn``: the dict of :meth:`outlier_power` on a handle with the dynamics factor, every figure from
        the covariance of the system WITH the factor; ``fit`` is a dict of :data:`FIT_NAMES_DYN` then :data:`POWER_FIT_NAMES`.  There
        is no figure in velocity and none for an edge (the header says why).  A handle without the factor raises."""
        return self._outlier_power("state", lamda, ncp, crit, strict)

    def last_state_outlier_power_ms(self):
        return self._last_ms("vba_schur_last_outlier_power_dyn_ms")

    def attitude_reliability(self, lamda=0.0, strict=True):
        """``vba_schur_reliability_att`` at the resident state of a handle with the dynamics AND the attitude factor
        (``include/vinsat_ba.h``): the dict of :meth:`state_reliability` -- every leverage and test from the covariance of the system
        with BOTH factors -- plus ``att_leverage [n-1]`` (trace of the attitude edge's 3x3 block of the hat matrix, in ``(0, 3]``),
        ``att_wtest [n-1]`` (the test of the gyro's gap rotation ``i -> i + 1``; NaN where ``I - P_a`` is not positive definite) and
        ``att_omega [n-1]`` (``sigma_att |a|^2``); ``fit`` is a dict of :data:`FIT_NAMES_ATT`, its ``rho`` and ``omega`` count the
        edges of both kinds.  There is still no w-test of an orbit edge.  :func:`suspects` reads the dict unchanged,
        :func:`gyro_suspects` reads ``att_wtest``.  Nothing on the handle changes.

        ``strict`` as in :meth:`state_covariance`.  A handle without the attitude factor raises: :meth:`state_reliability` or
        :meth:`reliability` is its query."""
        return self._reliability("attitude", lamda, strict)

    def last_attitude_reliability_ms(self):
        return self._last_ms("vba_schur_last_reliability_att_ms")

    def attitude_snoop(self, lamda=0.0, crit=3.29, scaled=True, min_rows=6, min_track=3, strict=True):
        """``vba_schur_snoop_att``: :meth:`snoop` on a handle with both factors -- the same rule, arguments and result, fed by the
        device part of :meth:`attitude_reliability` (``scaled`` reads its ``s0sq``, which counts the attitude equations).  Edges of
        either kind are never rejected: a gyro suspect is reported (:func:`gyro_suspects`), not acted on.  :meth:`rejected` and
        :meth:`restore_rejected` serve it too."""
        return self._snoop("attitude", lamda, crit, scaled, min_rows, min_track, strict)

    def last_attitude_snoop_ms(self):
        return self._last_ms("vba_schur_last_snoop_att_ms")

    def attitude_outlier_power(self, lamda=0.0, ncp=17.075, crit=3.29, strict=True):
        """``vba_schur_outlier_power_att``: the dict of :meth:`outlier_power` on a handle with both factors, every figure from the
        covariance of the system with both; ``fit`` is a dict of :data:`FIT_NAMES_ATT` then :data:`POWER_FIT_NAMES`.  There is no
        figure for an edge of either kind.  A handle without the attitude factor raises."""
        return self._outlier_power("attitude", lamda, ncp, crit, strict)

    def last_attitude_outlier_power_ms(self):
        return self._last_ms("vba_schur_last_outlier_power_att_ms")

    def reweight(self, alpha):
        """``vba_schur_reweight`` at the resident state (``include/vinsat_ba.h``): the reference's robust weights
        (``BA_filtering.py:21-25``) times the uploaded weights, written into the handle's weights on the device.  ``alpha`` in
        ``[1, 2]``; 2 puts the uploaded weights back.  Returns a dict: ``c_obs`` (the exact lower median of the ``2 m`` values
        ``|r|``, rows of weight 0 included), ``w_max`` (the largest raw weight) and ``status`` (1: ``c_obs`` is 0 or not finite,
        nothing was changed)."""
        c, wm, st = c_double(), c_double(), c_int()
        self._check(self.lib.vba_schur_reweight(self.h, float(alpha), byref(c), byref(wm), byref(st)))
        return dict(c_obs=c.value, w_max=wm.value, status=st.value)

    def weights(self, base=False):
        """The current weights -- or, with ``base``, the weights as uploaded -- in the CALLER's row order."""
        out = np.empty(self.m)
        self._check(self.lib.vba_schur_get_weights(self.h, None if base else out.ctypes.data_as(PD), out.ctypes.data_as(PD) if base else None))
        back = np.empty(self.m)
        back[self.order] = out                          # device rows are sorted by landmark
        return back

    def reweight_keys(self):
        """The ``2 m`` keys ``|r|`` of the last :meth:`reweight`, ``[m, 2]`` in the device's SORTED row order (``self.order``)."""
        out = np.empty(2 * self.m)
        self._check(self.lib.vba_schur_debug_fetch(self.h, 2, out.ctypes.data_as(PD), out.size))
        return out.reshape(self.m, 2)

    def last_reweight_ms(self):
        return self._last_ms("vba_schur_last_reweight_ms")

    def solve(self, lamda0=1e-4, max_iters=20, tol=1e-10, snoop=None, robust=None, state_snoop=None, attitude_snoop=None):
        """Levenberg-Marquardt driver: damping x10 on a rejected trial, /10 on an accepted one.  Returns the cost history.

        ``robust = dict(outer=8, alpha=None)`` (any subset) replaces the single LM loop by the robust loop: for ``it`` in
        ``range(outer)``, :meth:`reweight` at ``alpha(it)`` (a callable; ``None``: :func:`alpha_schedule`, the reference's) --
        the history gains ``("reweight", dict of reweight)`` -- then the LM loop from the resident state on those weights,
        which stay fixed through its trials as the reference's do through a ``BA()`` call.  A re-weighting with ``status != 0``
        ends the robust loop.  The ``snoop`` rounds, if given, follow on the final weights.

        ``snoop = dict(crit=, scaled=, min_rows=, min_track=, rounds=8)`` (any subset; ``lamda=`` of the query too, 0 by default):
        after the loop ends, at most ``rounds`` rounds of :meth:`snoop`; a round that rejected something is followed by the LM loop again from the
        resident state, one that rejected nothing ends the rounds.  The history gains one entry per round, ``("snoop", dict of
        :meth:`snoop`)``.  ``state_snoop = dict(...)`` is the same with :meth:`state_snoop`, the snoop of a handle with the dynamics
        factor (``snoop=`` on such a handle raises as :meth:`snoop` does), ``attitude_snoop = dict(...)`` the same with
        :meth:`attitude_snoop`, the snoop of a handle with the attitude factor too; give one of the three."""
        given = [(k, o) for k, o in (("snoop", snoop), ("state_snoop", state_snoop), ("attitude_snoop", attitude_snoop)) if o is not None]
        if len(given) > 1:
            raise ValueError("snoop, state_snoop and attitude_snoop are the rounds of three kinds of handle: give one of them")
        if robust is None:
            hist = self._lm_loop(lamda0, max_iters, tol)
        else:
            ropts = dict(robust)
            outer, alpha = int(ropts.pop("outer", 8)), ropts.pop("alpha", None) or alpha_schedule
            if ropts:
                raise ValueError(f"unknown robust options {sorted(ropts)}")
            hist = []
            for it in range(outer):
                res = self.reweight(alpha(it))
                hist.append(("reweight", res))
                if res["status"] != 0:
                    break
                hist += self._lm_loop(lamda0, max_iters, tol)
        if not given:
            return hist
        opts = dict(given[0][1])
        one_round = getattr(self, given[0][0])
        rounds = int(opts.pop("rounds", 8))
        for _ in range(rounds):
            res = one_round(**opts)
            hist.append(("snoop", res))
            if res["rows"] + res["landmarks"] == 0:
                break
            hist += self._lm_loop(lamda0, max_iters, tol)
        return hist

    def _lm_loop(self, lamda0, max_iters, tol):
        lam, hist = float(lamda0), []
        for _ in range(max_iters):
            c0, c1, ok = self.iterate(lam)
            hist.append((c0, c1, ok, lam))
            if ok:
                lam = max(lam * 0.1, 1e-9)
                if c0 - c1 <= tol * max(c0, 1e-300):
                    break
            else:
                lam *= 10.0
                if lam > 1e8:
                    break
        return hist


def suspects(rel, crit, scaled=False):
    """``(rows, landmarks)``: the indices (caller's order, ascending) of the rows whose ``wtest`` and of the landmarks whose
    ``lm_wtest`` exceed ``crit`` in the dict of :meth:`SchurBA.reliability` -- ``crit * sqrt(s0sq)`` with ``scaled`` (weights
    known up to their variance factor).  NaN tests exceed nothing."""
    thr = float(crit) * (np.sqrt(rel["fit"]["s0sq"]) if scaled else 1.0)
    with np.errstate(invalid="ignore"):
        return np.nonzero(rel["wtest"] > thr)[0], np.nonzero(rel["lm_wtest"] > thr)[0]


def gyro_suspects(rel, crit, scaled=False):
    """The indices (ascending) of the attitude edges ``i -> i + 1`` whose ``att_wtest`` exceeds ``crit`` in the dict of
    :meth:`SchurBA.attitude_reliability` -- ``crit * sqrt(s0sq)`` with ``scaled``, i.e. the test divided by ``s0``.  NaN tests exceed
    nothing.  A suspect is a gap whose gyro rotation the window contradicts; the edges next to it absorb part of the fault and rank
    behind it."""
    thr = float(crit) * (np.sqrt(rel["fit"]["s0sq"]) if scaled else 1.0)
    with np.errstate(invalid="ignore"):
        return np.nonzero(rel["att_wtest"] > thr)[0]


def scaled_power(power):
    """The dict of :meth:`SchurBA.outlier_power` with ``mdb``, ``ext_pos``, ``ext_att``, ``ext_lm``, ``lm_mdb`` and ``lm_ext`` times
    ``s0 = sqrt(fit["s0sq"])``, as ``ba.scaled_sigmas`` scales covariances: weights known up to their variance factor.  The
    deletion figures come from the residuals and need no scale.  A copy; ``power`` is left as it is."""
    s0 = float(np.sqrt(power["fit"]["s0sq"]))
    out = dict(power)
    for key in ("mdb", "ext_pos", "ext_att", "ext_lm", "lm_mdb", "lm_ext"):
        out[key] = np.asarray(power[key]) * s0
    out["s0"] = s0
    return out


def prior_for_first_pose(handoff):
    """The ``state_prior`` tuple of :class:`SchurBA` for pose 0 of the next window from the dict of :meth:`SchurBA.handoff`."""
    return (np.zeros(1, dtype=np.int32), np.asarray(handoff["anchor"], dtype=np.float64).reshape(1, 10),
            np.asarray(handoff["info"], dtype=np.float64).reshape(1, 9, 9))


def tile_bandwidth_of(structure, tile=64):
    """Largest distance from the diagonal of a non-zero tile of the reduced system, as ``vba_schur_upload`` derives it: the
    substitutions and the triangular inverse of the covariance query skip the tiles beyond it."""
    return int(((6 * structure["blk_i"].astype(np.int64) + 5) // tile - (6 * structure["blk_j"].astype(np.int64)) // tile).max())


def _blocks(cov, key):
    return np.asarray(cov[key] if isinstance(cov, dict) else cov, dtype=np.float64)


def pose_sigmas(cov):
    """1-sigma per pose from :meth:`SchurBA.covariance` (its dict, or ``[..., 6, 6]`` blocks): ``(position [..., 3] km,
    attitude [..., 3] rad)``.  The step's ``dtheta`` linearises a rotation of angle ``2 dtheta``: attitude = ``2 sqrt(.)``."""
    d = np.diagonal(_blocks(cov, "pose"), axis1=-2, axis2=-1)
    return np.sqrt(d[..., 0:3]), 2.0 * np.sqrt(d[..., 3:6])


def state_sigmas(cov):
    """1-sigma per pose from :meth:`SchurBA.state_covariance` (its dict, or ``[..., 9, 9]`` blocks): ``(position [..., 3] km,
    attitude [..., 3] rad, velocity [..., 3] km/s)``.  Attitude is ``2 sqrt(.)`` as in :func:`pose_sigmas`."""
    d = np.diagonal(_blocks(cov, "state"), axis1=-2, axis2=-1)
    return np.sqrt(d[..., 0:3]), 2.0 * np.sqrt(d[..., 3:6]), np.sqrt(d[..., 6:9])


def landmark_sigmas(cov):
    """1-sigma per landmark and axis, km ``[..., 3]``, from :meth:`SchurBA.covariance` (its dict, or ``[..., 3, 3]`` blocks)."""
    return np.sqrt(np.diagonal(_blocks(cov, "landmark"), axis1=-2, axis2=-1))
