"""``BA``: the reference's bundle-adjustment call surface, executed by the HIP kernels.

Same positional signature and 4-tuple return as the reference's
``estimation/BA/BA_filtering.py:4, 98``::

    states_new, velocities, lamda_init, last_hessian = BA(iter, states, velocities, imu_meas, landmarks,
        landmarks_xyz, ii, time_idx, intrinsics, confidences, Sigma, V, lamda_init, poses_gt_eci, initialize=False)

Behaviour kept from the reference: ``Sigma``/``V`` are ignored (overwritten at :26-27),
``velocities`` is returned untouched, only ``imu_meas[0, :, -1, 6:10]`` is read
(``BA_utils.py:295``), a "lamda too large" outcome keeps the last trial (:75-77).
Inputs may be torch tensors or NumPy arrays; outputs are fp64 torch tensors shaped like
the reference's (``[1,n,10]``, ``[1,9,9]``).

What makes the reference's loop ``for iter in range(20): states, ... = BA(iter, states, ...)``
(``od_pipe.py:1036-1040``) cheap here:

* the window arguments (observations, per-pose constants) are uploaded once: a call whose arguments are the SAME
  buffers with the SAME content as the previous call's skips the upload.  For torch tensors "same" is decided by identity:
  buffer address, shape, strides, dtype and torch's in-place modification counter ``_version`` (a write through a
  ``.numpy()`` alias or ``.data`` does not bump that counter: call :func:`invalidate` after such a write).  NumPy arrays
  carry no such counter, so their CONTENT is compared, byte for byte, with a private copy taken at the upload (``ii`` and
  ``time_idx`` are what the reference passes as ndarrays: 0.4 MB at 500 / 50k, ~8 us of memcmp) -- an in-place edit is
  seen and uploads the window again.  The arguments of the last upload are kept referenced, so an address cannot be
  recycled by another live array;
* a call whose ``states`` IS the tensor the previous call returned (and whose ``lamda_init`` is the value it
  returned) uploads nothing at all: the device already holds both (``vba_iterate_resident``).

Batch dimension.  The reference's ``BA`` carries ``bsz = states.shape[0]`` (``BA_filtering.py:14``) but hard-codes batch index
0 at ``:24`` and ``:37``, and its real batch axis is the loop over sequences (``od_pipe.py:1069-1077``).  Here ``BA`` /
``BA_window`` take a batch in either of two forms and run all its windows with every kernel launch covering the lot (one
ragged handle of ``bsz`` windows, ``vba_step`` / ``vba_run_schedule``):

* dense: ``states [B, n, 10]``, ``imu_meas [B, n, g, 10]``, ``landmarks [B, m, 2]``, ``landmarks_xyz [B, m, 3]``,
  ``intrinsics [B, n, 4]`` (or ``[1, n, 4]``), ``ii`` / ``time_idx`` / ``confidences`` shared (``[m]``, ``[n]``, ``[m]``) or per
  window (``[B, m]`` ...), ``lamda_init`` a float or ``B`` floats; returns ``states_new [B, n, 10]``, ``velocities``, a list of
  ``B`` dampings and ``last_hessian [B, 9, 9]``;
* ragged: every per-window argument a list of ``B`` items shaped as the reference's single-window arguments (windows of
  different ``n``, ``m``); returns lists.

``iter`` and ``initialize`` are per call, as in the reference.  Equal handle settings (:func:`configure`) give a window the
same bits in a batch as alone.

No CPU fallback exists.
"""
from __future__ import annotations

import ctypes

import numpy as np

from .engine import BAEngine

_memcmp = ctypes.CDLL(None).memcmp
_memcmp.argtypes = (ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)
_memcmp.restype = ctypes.c_int

_cache = {}
_WATCH_SLOTS = 8         # vba_set_host_watch: one per array argument of BA()


def _np(x):
    try:
        import torch
        if isinstance(x, torch.Tensor):
            return x.detach().cpu().double().numpy()
    except ImportError:
        pass
    return np.asarray(x, dtype=np.float64)


def _token(x):
    """Identity of an argument's buffer (torch: plus its in-place counter); the content of NumPy arrays is checked
    separately (host watch, see :func:`_engine_for`), see the module docstring."""
    ver = getattr(x, "_version", None)
    if ver is not None:                                    # torch.Tensor
        return (x.data_ptr(), tuple(x.shape), x.stride(), x.dtype, ver)
    if isinstance(x, np.ndarray):
        return (x.__array_interface__["data"][0], x.shape, x.strides, x.dtype.str)
    return ("obj", id(x))


def _same_objects(args):
    """The cheap test that almost every call of a driver loop passes: the very same Python objects as at the upload, torch
    tensors with an unchanged in-place counter (ndarrays: their content is compared by the library while the device
    works, see ``vba_set_host_watch``)."""
    refs = _cache.get("refs")
    if refs is None:
        return False
    vers = _cache["vers"]
    for a, r, v in zip(args, refs, vers):
        if a is not r or getattr(a, "_version", None) != v:
            return False
    return True


def _same_bytes(a, c):
    """Equal content of two ndarrays of equal shape and dtype; contiguous ones by one ``memcmp`` (``np.array_equal`` builds a
    boolean array first: ~5 x the time at 400 kB)."""
    if a.flags.c_contiguous and c.flags.c_contiguous and a.dtype.kind in "iuf":
        if a.dtype.kind != "f":
            return _memcmp(a.ctypes.data, c.ctypes.data, a.nbytes) == 0
        # (floats: equal bytes are equal values; different bytes may still be equal values, -0.0 == 0.0 -- only then look closer)
        return _memcmp(a.ctypes.data, c.ctypes.data, a.nbytes) == 0 or np.array_equal(a, c)
    return np.array_equal(a, c)


def _watchable(a):
    """The host buffer of an argument whose CONTENT is compared with the uploaded copy: an ndarray itself; with
    ``configure(strict=True)`` also a torch CPU tensor (as the ndarray view of its storage: a write through ``.numpy()`` or any
    other alias does not bump ``_version`` and would otherwise go unseen); None for everything else."""
    if isinstance(a, np.ndarray):
        return a
    if _cache.get("strict") and getattr(a, "_version", None) is not None:
        try:
            if a.device.type == "cpu" and not a.requires_grad:
                return a.detach().numpy()
        except (RuntimeError, TypeError):
            pass
    return None


def _numpy_unchanged(args):
    """True if every watchable argument (:func:`_watchable`) still holds the bytes of the private copy taken when it was uploaded."""
    for a, c in zip(args, _cache.get("np_copies", ())):
        if c is None:
            continue
        a = _watchable(a)
        if a is None or not (a.shape == c.shape and a.dtype == c.dtype and _same_bytes(a, c)):
            return False
    return True


def configure(integrator=None, lanes=None, fusion=None, solver=None, mode=None, strict=None, jacobian=None):
    """Settings of the cached engines that the reference's call surface has no argument for.

    ``integrator``: ``"rk4"`` (default) = one-second RK4 steps, the reference's CPU branch ``predict``
    (``BA_utils.py:73-87``) -- the parity target; ``"hop"`` = the <=100 s hops of ``predict_gpu``
    (``BA_utils.py:52-71, 529-602``), which is what the reference itself runs when it sees a GPU
    (``BA_filtering.py:16-17``).  Takes effect from the next call on.

    ``jacobian``: ``"fp64"`` (default) or ``"fp32"`` = the terms of the reprojection Jacobian in fp32, everything else in
    fp64 (``VBA_OPT_JACOBIAN_F32``; ``include/vinsat_ba.h`` states the contract).
    Takes effect from the next call on.

    ``lanes`` / ``fusion`` / ``solver`` / ``mode`` pin what a handle otherwise chooses from its own geometry -- lanes per
    pose of the accumulation (``VBA_OPT_ACCUMULATE_LANES``: the shape of its reduction tree), the kernel-fusion mask
    (``VBA_OPT_FUSION``), the chain partition ``(chunk, chunk2)`` (``vba_set_solver2``; ``0`` = sequential walk) and the kernel
    set (``vba_create_mode``) -- so that a window gets the same bits alone and in a batch of any size.  ``"auto"`` returns
    one of them to the handle's choice.  The cached engines are rebuilt.

    ``strict=True``: torch CPU arguments are content-checked like ndarrays (private copy at the upload, compared by the library
    while the device works) instead of being trusted on address / shape / ``_version`` -- a write through ``tensor.numpy()`` or
    another alias is then seen by itself; costs one more copy of the window's arguments at every upload."""
    if strict is not None and bool(strict) != bool(_cache.get("strict")):
        _cache["strict"] = bool(strict)
        invalidate()
    if integrator is not None:
        if integrator not in ("rk4", "hop"):
            raise ValueError("integrator must be 'rk4' or 'hop'")
        _cache["hop"] = integrator == "hop"
        for key in ("eng", "beng"):
            eng = _cache.get(key)
            if eng is not None:
                eng.set_integrator(_cache["hop"])
        _cache["resident"] = None
        _cache["bresident"] = None
    if jacobian is not None:
        if jacobian not in ("fp64", "fp32"):
            raise ValueError("jacobian must be 'fp64' or 'fp32'")
        _cache["jac_f32"] = jacobian == "fp32"
        for key in ("eng", "beng"):
            eng = _cache.get(key)
            if eng is not None:
                eng.set_jacobian_f32(_cache["jac_f32"])
        _cache["resident"] = None
        _cache["bresident"] = None
    pins = dict(_cache.get("pins", {}))
    changed = False
    for name, val in (("lanes", lanes), ("fusion", fusion), ("solver", solver), ("mode", mode)):
        if val is None:
            continue
        if val == "auto":
            changed |= pins.pop(name, None) is not None
        else:
            changed |= pins.get(name) != val
            pins[name] = val
    if changed:
        _cache["pins"] = pins
        release()


def _new_engine(n_max, m_max, windows, device):
    """An engine with the pinned settings (:func:`configure`) applied."""
    pins = _cache.get("pins", {})
    eng = BAEngine(n_max, m_max, windows=windows, device=device, mode={"lat": 1, "bw": 0}.get(pins.get("mode"), pins.get("mode", -1)))
    eng.set_integrator(bool(_cache.get("hop", False)))
    if _cache.get("jac_f32"):
        eng.set_jacobian_f32(True)
    if "lanes" in pins:
        eng.set_accumulate_lanes(pins["lanes"])
    if "fusion" in pins:
        eng.set_fusion(pins["fusion"])
    if "solver" in pins:
        sv = pins["solver"]
        if isinstance(sv, (tuple, list)):
            eng.set_solver(*sv)
        else:
            eng.set_solver(sv)
    return eng


def invalidate():
    """Forget what is on the device: the next call uploads its window again (needed after a torch argument was written
    through an alias that does not bump its ``_version``; edits of NumPy arguments are seen by themselves)."""
    # the watch slots first: clearing them waits for the library's comparison helper, which may still be reading the live
    # buffers and the copies that are dropped below
    eng = _cache.get("eng")
    if eng is not None and getattr(eng, "h", None):
        for k in range(_WATCH_SLOTS):
            eng.set_host_watch(k)
    _cache.pop("key", None)
    _cache.pop("refs", None)
    _cache.pop("vers", None)
    _cache.pop("nm", None)
    _cache.pop("np_copies", None)
    _cache.pop("views", None)
    _cache.pop("all_watched", None)
    _cache.pop("bkey", None)
    _cache.pop("bleaves", None)
    _cache.pop("brefs", None)
    _cache.pop("bcopies", None)
    _cache.pop("bform", None)
    _cache.pop("bns", None)
    _cache["resident"] = None
    _cache["bresident"] = None


def release():
    """Close the cached engines (device memory, streams) -- e.g. before another handle takes over the device."""
    for key in ("eng", "beng"):
        eng = _cache.pop(key, None)
        if eng is not None:
            eng.close()
    invalidate()


def _engine_for(args, n, m, device, compare_now=False):
    """The cached engine with the window given by ``args`` = (imu_meas, landmarks, landmarks_xyz, ii, time_idx,
    intrinsics, confidences) on the device.  ``compare_now``: the caller's device call does not evaluate the library's host
    watch (``vba_run_schedule``: :func:`BA_window`), so the watched buffers are compared here, before it."""
    eng = _cache.get("eng")
    if eng is None or eng.n_max < n or eng.m_max < m or eng.device != device:
        if eng is not None:
            eng.close()
        eng = _new_engine(max(n, 16), max(m, 256), 1, device)
        _cache["eng"] = eng
        invalidate()
    if _cache.get("nm") == (n, m) and _same_objects(args):
        # ndarray contents: compared by the library while the device works (resident calls) -- if every ndarray has a watch slot
        # (contiguous, at most 8 of them); else here and now
        if (_cache.get("all_watched") and not compare_now) or _numpy_unchanged(args):
            return eng
    key = (n, m) + tuple(_token(a) for a in args)
    if _cache.get("key") != key or not _numpy_unchanged(args):
        imu_meas, landmarks, landmarks_xyz, ii, time_idx, intrinsics, confidences = args
        cum = np.ascontiguousarray(_np(imu_meas)[0, :, -1, 6:10])
        uv = _np(landmarks).reshape(-1, 2)
        xyz = _np(landmarks_xyz).reshape(-1, 3)
        K = _np(intrinsics).reshape(-1, 4)
        conf = _np(confidences).reshape(-1)
        ii_ = np.ascontiguousarray(np.asarray(ii), dtype=np.int64).reshape(-1)
        t = np.ascontiguousarray(np.asarray(time_idx), dtype=np.int64).reshape(-1)
        if not (K.shape[0] == n and cum.shape[0] == n and t.shape[0] == n):
            raise ValueError("intrinsics / imu_meas / time_idx must have one row per pose")
        if xyz.shape[0] != m:
            raise ValueError("landmarks and landmarks_xyz disagree on the number of rows")
        eng.upload_observations(xyz, uv, conf, ii_, n)
        eng.upload_window(K, cum, t)
        _cache["key"] = key
        _cache["np_copies"] = tuple(w.copy() if w is not None else None for w in map(_watchable, args))
        _cache["resident"] = None
    # (also when only the Python objects are new -- fresh slices of the same buffers, as the reference's driver makes them)
    _cache["nm"] = (n, m)
    _cache["refs"] = args               # keeps the buffers alive: their addresses cannot be reused while cached
    _cache["vers"] = tuple(getattr(a, "_version", None) for a in args)
    # the library compares the live ndarrays with the copies that were uploaded during every resident call
    slot, all_watched, views = 0, True, []
    for a, c in zip(args, _cache["np_copies"]):
        if c is None:
            continue
        a = _watchable(a)
        views.append(a)
        if slot < _WATCH_SLOTS and a.flags.c_contiguous and c.flags.c_contiguous:
            eng.set_host_watch(slot, a, c)
            slot += 1
        else:
            all_watched = False         # (a strided view: compared on the Python side before every call instead)
    _cache["views"] = views             # (the ndarray views of watched torch tensors stay alive with the watch)
    for k in range(slot, _WATCH_SLOTS):
        eng.set_host_watch(k)
    _cache["all_watched"] = all_watched
    return eng


def _shape_of(states):
    shp = tuple(states.shape)
    if len(shp) != 3 or shp[0] != 1 or shp[2] != 10:
        raise ValueError("states must be [1, n, 10] here (BA and BA_window also take batches: [B, n, 10] or a list of windows)")
    return shp[1]


def _rows(landmarks):
    shp = landmarks.shape
    if len(shp) == 3:
        return shp[0] * shp[1]
    return int(np.prod(shp[:-1])) if len(shp) > 1 else shp[0] // 2


def _take_resident(states, lamda_init, reg):
    """True if the device holds exactly these states and this damping (the previous call's result).  The record is
    consumed either way: it is valid again only once the next call has returned."""
    r = _cache.get("resident")
    _cache["resident"] = None
    return (r is not None and r[0] is states and getattr(states, "_version", None) == r[1]
            and float(lamda_init) == r[2] and r[3] == reg)


def _wrap(out, lam, hess, reg):
    import torch
    st = torch.from_numpy(out)[None]
    _cache["resident"] = (st, st._version, lam, reg)
    return st, torch.from_numpy(hess)[None]


_HOST_CHANGED = 1 << 30


def _call(eng, reg, iter, initialize, states, lamda_init, reupload):
    """One call on the cached engine: resident if the states are the previous result, else with the states sent up.  A
    resident call during which the library found a watched ndarray edited is repeated on the window as it is now."""
    if _take_resident(states, lamda_init, reg):
        out, lam, hess, n_trials, flags = eng.iterate_resident(iter, initialize)
        if flags & _HOST_CHANGED:
            invalidate()
            eng = reupload()
            out, lam, hess, n_trials, flags = eng.iterate(iter, initialize, float(lamda_init), _np(states)[0])
    else:
        # the first call of a window's loop: the calls that follow feed its result back, so it opens the pipelined chain
        # (vba_iterate_open), and like a resident call it has the library compare the watched ndarrays while the device works;
        # ndarrays without a watch slot are compared here and now
        watched = _cache.get("all_watched")
        if not watched and not _numpy_unchanged(_cache.get("refs", ())):
            invalidate()
            eng = reupload()
        out, lam, hess, n_trials, flags = eng.iterate(iter, initialize, float(lamda_init), _np(states)[0], opening=True)
        if watched and flags & _HOST_CHANGED:
            invalidate()
            eng = reupload()
            out, lam, hess, n_trials, flags = eng.iterate(iter, initialize, float(lamda_init), _np(states)[0])
    return out, lam, hess, n_trials, flags & 7


# ------------------------------------------------------------------------------------------------ batch dimension
def _is_batch(states):
    if isinstance(states, (list, tuple)):
        return True
    shp = getattr(states, "shape", None)
    return shp is not None and len(shp) == 3 and shp[0] > 1


def _item(x, b, B, what):
    """Window ``b`` of a per-window argument given as a list of ``B`` items."""
    if not isinstance(x, (list, tuple)) or len(x) != B:
        raise ValueError(f"ragged batch: {what} must be a list of {B} items (one per window)")
    return x[b]


def _split_batch(states, imu_meas, landmarks, landmarks_xyz, ii, time_idx, intrinsics, confidences, lamda_init):
    """Per-window views of a batch.  Returns (form, windows) with ``form`` "dense" or "ragged" and, per window, a dict of
    NumPy arrays: states [n,10], cum [n,4], uv [m,2], xyz [m,3], ii [m] int64, t [n] int64, K [n,4], conf [m], lam."""
    ragged = isinstance(states, (list, tuple))
    B = len(states) if ragged else states.shape[0]
    if B < 1:
        raise ValueError("empty batch")
    lams = [float(x) for x in lamda_init] if isinstance(lamda_init, (list, tuple, np.ndarray)) else [float(lamda_init)] * B
    if len(lams) != B:
        raise ValueError("lamda_init must be a float or one float per window")
    wins = []
    if ragged:
        for b in range(B):
            st = _np(states[b]).reshape(-1, 10)
            imu = _np(_item(imu_meas, b, B, "imu_meas"))
            imu = imu[0] if imu.ndim == 4 else imu
            wins.append(dict(states=st, cum=np.ascontiguousarray(imu[:, -1, 6:10]),
                             uv=_np(_item(landmarks, b, B, "landmarks")).reshape(-1, 2),
                             xyz=_np(_item(landmarks_xyz, b, B, "landmarks_xyz")).reshape(-1, 3),
                             ii=np.ascontiguousarray(np.asarray(_item(ii, b, B, "ii")), dtype=np.int64).reshape(-1),
                             t=np.ascontiguousarray(np.asarray(_item(time_idx, b, B, "time_idx")), dtype=np.int64).reshape(-1),
                             K=_np(_item(intrinsics, b, B, "intrinsics")).reshape(-1, 4),
                             conf=_np(_item(confidences, b, B, "confidences")).reshape(-1), lam=lams[b]))
    else:
        st_all, imu_all = _np(states), _np(imu_meas)
        uv_all, xyz_all, K_all = _np(landmarks), _np(landmarks_xyz), _np(intrinsics)
        ii_all, t_all, c_all = np.asarray(ii), np.asarray(time_idx), _np(confidences)
        if imu_all.ndim != 4 or imu_all.shape[0] not in (1, B) or uv_all.shape[0] != B or xyz_all.shape[0] != B:
            raise ValueError("dense batch: imu_meas [B,n,g,10], landmarks [B,m,2] and landmarks_xyz [B,m,3] need the batch size of states")
        for b in range(B):
            wins.append(dict(states=st_all[b], cum=np.ascontiguousarray(imu_all[b if imu_all.shape[0] == B else 0][:, -1, 6:10]),
                             uv=uv_all[b].reshape(-1, 2), xyz=xyz_all[b].reshape(-1, 3),
                             ii=np.ascontiguousarray(ii_all[b] if ii_all.ndim == 2 else ii_all, dtype=np.int64).reshape(-1),
                             t=np.ascontiguousarray(t_all[b] if t_all.ndim == 2 else t_all, dtype=np.int64).reshape(-1),
                             K=(K_all[b] if K_all.shape[0] == B else K_all[0]).reshape(-1, 4),
                             conf=(c_all[b] if c_all.ndim == 2 else c_all).reshape(-1), lam=lams[b]))
    for b, w in enumerate(wins):
        n, m = w["states"].shape[0], w["xyz"].shape[0]
        if not (w["K"].shape[0] == n and w["cum"].shape[0] == n and w["t"].shape[0] == n):
            raise ValueError(f"window {b}: intrinsics / imu_meas / time_idx must have one row per pose")
        if not (w["uv"].shape[0] == m and w["ii"].shape[0] == m and w["conf"].shape[0] == m):
            raise ValueError(f"window {b}: landmarks, landmarks_xyz, ii and confidences disagree on the number of rows")
    return ("ragged" if ragged else "dense"), wins


def _flat(x):
    """The leaves of a (possibly list-valued) argument, for identity tokens."""
    return tuple(x) if isinstance(x, (list, tuple)) else (x,)


def _leaves(args):
    return tuple(leaf for a in args for leaf in _flat(a))


def _batch_hit(args, device):
    """The cached batch engine if it holds exactly these windows: same argument buffers (identity tokens) and, for ndarray
    arguments, the bytes that were uploaded (each distinct array compared once)."""
    eng = _cache.get("beng")
    if eng is None or eng.device != device or "bkey" not in _cache:
        return None
    leaves = _leaves(args)
    # the cheap test first (what every call of a driver loop passes): the very same leaf objects as at the upload, torch tensors
    # with an unchanged in-place counter -- 154 leaves at 22 windows, whose tokens cost ~0.25 ms to build
    old = _cache.get("bleaves")
    same = old is not None and len(old[0]) == len(leaves) and all(a is b for a, b in zip(leaves, old[0])) \
        and tuple(getattr(a, "_version", None) for a in leaves) == old[1]
    if not same and _cache["bkey"] != tuple(_token(a) for a in leaves):
        return None
    seen = set()
    for a, c in zip(leaves, _cache.get("bcopies", ())):
        if c is None or id(a) in seen:
            continue
        seen.add(id(a))
        if not (a.shape == c.shape and a.dtype == c.dtype and _same_bytes(a, c)):
            return None
    if not same:        # (fresh objects over the same buffers: remember them for the next call)
        _cache["bleaves"] = (leaves, tuple(getattr(a, "_version", None) for a in leaves))
    return eng


def _batch_engine_for(args, wins, device):
    """A batch engine (one ragged handle of len(wins) windows) with these windows uploaded; becomes the cached one."""
    B = len(wins)
    n_max = max(16, max(w["states"].shape[0] for w in wins))
    m_max = max(256, max(w["xyz"].shape[0] for w in wins))
    eng = _cache.get("beng")
    if eng is None or eng.windows != B or eng.n_max < n_max or eng.m_max < m_max or eng.device != device:
        if eng is not None:
            eng.close()
        eng = _new_engine(n_max, m_max, B, device)
        _cache["beng"] = eng
    for b, w in enumerate(wins):
        eng.upload_observations(w["xyz"], w["uv"], w["conf"], w["ii"], w["states"].shape[0], window=b)
        eng.upload_window(w["K"], w["cum"], w["t"], window=b)
    leaves = _leaves(args)
    _cache["bkey"] = tuple(_token(a) for a in leaves)
    copies, made = [], {}
    for a in leaves:
        if isinstance(a, np.ndarray):
            if id(a) not in made:
                made[id(a)] = a.copy()
            copies.append(made[id(a)])
        else:
            copies.append(None)
    _cache["bcopies"] = tuple(copies)
    _cache["bleaves"] = (leaves, tuple(getattr(a, "_version", None) for a in leaves))
    _cache["brefs"] = args              # keeps the buffers alive: their addresses cannot be reused while cached
    return eng


def _batch_resident(states, lamda_init):
    """True if the device holds exactly these states and dampings: ``states`` IS what the previous batched call returned."""
    r = _cache.get("bresident")
    _cache["bresident"] = None
    if r is None:
        return False
    prev, vers, lams = r
    if isinstance(prev, list):
        same = isinstance(states, (list, tuple)) and len(states) == len(prev) and all(a is b for a, b in zip(states, prev))
        now = tuple(getattr(a, "_version", None) for a in states) if same else None
    else:
        same = states is prev
        now = (getattr(states, "_version", None),) if same else None
    lam_in = [float(x) for x in lamda_init] if isinstance(lamda_init, (list, tuple, np.ndarray)) else None
    return bool(same and now == vers and lam_in is not None and lam_in == lams)


def _batch_result(eng, form, ns):
    import torch
    S, lam, hess, ntr, flags = eng.get_states_all()
    lams = [float(x) for x in lam]
    if form == "dense":
        st = torch.from_numpy(np.ascontiguousarray(S[:, :ns[0]]))
        hs = torch.from_numpy(hess)
        _cache["bresident"] = (st, (st._version,), lams)
    else:
        st = [torch.from_numpy(np.ascontiguousarray(S[b, :n]))[None] for b, n in enumerate(ns)]
        hs = [torch.from_numpy(hess[b].copy())[None] for b in range(len(ns))]
        _cache["bresident"] = (st, tuple(x._version for x in st), lams)
    return st, lams, hs, [int(x) for x in ntr], [int(x) & 7 for x in flags]


def _batch_states_up(eng, states, lamda_init, ns):
    B = len(ns)
    lams = [float(x) for x in lamda_init] if isinstance(lamda_init, (list, tuple, np.ndarray)) else [float(lamda_init)] * B
    if len(lams) != B:
        raise ValueError("lamda_init must be a float or one float per window")
    S = np.zeros((eng.windows, eng.n_max, 10))
    for b, n in enumerate(ns):
        st = _np(states[b]).reshape(-1, 10)
        if st.shape[0] != n:
            raise ValueError(f"window {b}: states have {st.shape[0]} poses, the window {n}")
        S[b, :n] = st
    eng.set_states_all(S, lams)


def _BA_batched(iters, inits, states, velocities, imu_meas, landmarks, landmarks_xyz, ii, time_idx, intrinsics, confidences, lamda_init, device):
    """``len(iters)`` BA() calls on every window of a batch: one ``vba_step`` (a single call) or one chained ``vba_run_schedule``."""
    args = (imu_meas, landmarks, landmarks_xyz, ii, time_idx, intrinsics, confidences)
    resident = _batch_resident(states, lamda_init)
    eng = _batch_hit(args, device)
    B = len(states) if isinstance(states, (list, tuple)) else states.shape[0]
    if eng is not None and _cache.get("bform") is not None and len(_cache["bns"]) == B:
        form, ns = _cache["bform"], _cache["bns"]         # the windows are on the device already
    else:
        form, wins = _split_batch(states, imu_meas, landmarks, landmarks_xyz, ii, time_idx, intrinsics, confidences, lamda_init)
        eng = _batch_engine_for(args, wins, device)
        ns = [w["states"].shape[0] for w in wins]
        _cache["bform"], _cache["bns"] = form, ns
        resident = False
    if not resident:        # (else: the device holds these states and dampings -- the previous call's result)
        _batch_states_up(eng, states, lamda_init, ns)
    if len(iters) == 1:
        eng.step(int(iters[0]), bool(inits[0]))
    else:
        eng.run_schedule([int(x) for x in iters], [bool(x) for x in inits])
    st, lams, hs, ntr, flags = _batch_result(eng, form, ns)
    for f in flags:
        if f & 1:
            print("lamda too large")          # reference BA_filtering.py:76
    return st, lams, hs, ntr, flags


def BA(iter, states, velocities, imu_meas, landmarks, landmarks_xyz, ii, time_idx, intrinsics, confidences, Sigma, V,
       lamda_init, poses_gt_eci, initialize=False, device=0):
    if _is_batch(states):       # bsz > 1 (dense) or a list of windows (ragged): see the module docstring
        st, lams, hs, ntr, flags = _BA_batched([iter], [initialize], states, velocities, imu_meas, landmarks, landmarks_xyz, ii,
                                               time_idx, intrinsics, confidences, lamda_init, device)
        BA.last = dict(n_trials=ntr, flags=flags)
        _cache["last_query"] = dict(eng="beng", iter=int(iter), reg=False, form=_cache["bform"], ns=list(_cache["bns"]))
        return (st, velocities, lams, hs)
    shp = states.shape
    if len(shp) != 3 or shp[0] != 1 or shp[2] != 10:
        _shape_of(states)
    n = shp[1]
    args = (imu_meas, landmarks, landmarks_xyz, ii, time_idx, intrinsics, confidences)
    m = _rows(landmarks)
    eng = _engine_for(args, n, m, device)
    out, lam, hess, n_trials, flags = _call(eng, False, int(iter), bool(initialize), states, lamda_init,
                                            lambda: _engine_for(args, n, m, device))
    if flags & 1:
        print("lamda too large")          # reference BA_filtering.py:76
    BA.last = dict(n_trials=n_trials, flags=flags)
    _cache["last_query"] = dict(eng="eng", iter=int(iter), reg=False, form="single", ns=[n])
    st, hs = _wrap(out, lam, hess, False)
    return (st, velocities, lam, hs)


BA.last = {}


def BA_reg(iter, states, velocities, states_prior, velocity_prior, hessian_state_t, hessian_rot_t, imu_meas, landmarks,
           landmarks_xyz, ii, time_idx, intrinsics, confidences, Sigma, V, lamda_init, poses_gt_eci, initialize=False,
           use_reg=True, device=0):
    """Counterpart of the reference's ``BA_reg`` (``BA_filtering.py:100-210``): ``BA`` with a propagated-covariance
    prior per pose.  Same positional signature and 4-tuple.  As in the reference ``Sigma``, ``V``, ``use_reg`` and
    ``velocity_prior`` are not read (the prior velocity is ``states_prior[..., 7:]``, ``BA_utils.py:614``), and
    ``hessian_rot_t`` has no effect on the result (see ``include/vinsat_ba.h``: the rotation term of ``prior_gpu`` is
    a constant).  The integrator is the reference's CPU branch (``predict``) unless the engine is switched."""
    n = _shape_of(states)
    eng = _engine_for((imu_meas, landmarks, landmarks_xyz, ii, time_idx, intrinsics, confidences), n, _rows(landmarks), device)
    pkey = (_token(states_prior), _token(hessian_state_t))
    pc = _cache.get("prior_copies", (None, None))
    same_bytes = all(c is None or np.array_equal(a, c) for a, c in zip((states_prior, hessian_state_t), pc))
    if _cache.get("prior_key") != pkey or _cache.get("prior_for") != _cache.get("key") or not same_bytes:
        sp = _np(states_prior).reshape(-1, 10)
        Hs = _np(hessian_state_t).reshape(-1, 6, 6)
        if not (sp.shape[0] == n and Hs.shape[0] == n):
            raise ValueError("the prior must have one row per pose")
        eng.upload_prior(sp, Hs)
        _cache["prior_key"], _cache["prior_for"], _cache["prior_refs"] = pkey, _cache.get("key"), (states_prior, hessian_state_t)
        _cache["prior_copies"] = tuple(a.copy() if isinstance(a, np.ndarray) else None for a in (states_prior, hessian_state_t))
        _cache["resident"] = None
    eng.set_prior(True)
    try:
        args = (imu_meas, landmarks, landmarks_xyz, ii, time_idx, intrinsics, confidences)
        out, lam, hess, n_trials, flags = _call(eng, True, int(iter), bool(initialize), states, lamda_init,
                                                lambda: _engine_for(args, n, _rows(landmarks), device))
    finally:
        eng.set_prior(False)
    if flags & 1:
        print("lamda too large")          # reference BA_filtering.py:186
    BA_reg.last = dict(n_trials=n_trials, flags=flags)
    _cache["last_query"] = dict(eng="eng", iter=int(iter), reg=True, form="single", ns=[n])
    st, hs = _wrap(out, lam, hess, True)
    return (st, velocities, lam, hs)


BA_reg.last = {}


def BA_window(iters, initializes, states, velocities, imu_meas, landmarks, landmarks_xyz, ii, time_idx, intrinsics, confidences,
              lamda_init, device=0):
    """The driver's loop ``for iter in range(num_iters): states, ... = BA(iter, states, ...)`` (reference
    ``od_pipe.py:1036-1040``) as ONE call: the states stay on the device between the calls and the calls are chained
    there (``vba_run_schedule``).  Bit-identical to calling :func:`BA` ``len(iters)`` times.

    Returns ``(states_new, velocities, lamda, last_hessian)`` of the last call, shaped like ``BA``'s.  A batch (dense
    ``[B, n, 10]`` or a list of windows, see the module docstring) runs the schedule on every window at once.
    """
    if _is_batch(states):
        st, lams, hs, ntr, flags = _BA_batched(list(iters), list(initializes), states, velocities, imu_meas, landmarks,
                                               landmarks_xyz, ii, time_idx, intrinsics, confidences, lamda_init, device)
        BA_window.last = dict(n_trials=ntr, flags=flags)
        _cache["last_query"] = dict(eng="beng", iter=int(list(iters)[-1]), reg=False, form=_cache["bform"], ns=list(_cache["bns"]))
        return (st, velocities, lams, hs)
    n = _shape_of(states)
    # (vba_run_schedule does not evaluate the host watch: an ndarray edited in place since the upload is looked for here)
    eng = _engine_for((imu_meas, landmarks, landmarks_xyz, ii, time_idx, intrinsics, confidences), n, _rows(landmarks), device, compare_now=True)
    if not _take_resident(states, lamda_init, False):
        eng.set_states(_np(states)[0], float(lamda_init))
    eng.run_schedule(list(iters), list(initializes))
    out, lam, hess, n_trials, flags = eng.get_states()
    if flags & 1:
        print("lamda too large")
    _cache["last_query"] = dict(eng="eng", iter=int(list(iters)[-1]), reg=False, form="single", ns=[n])
    st, hs = _wrap(out, lam, hess, False)
    return (st, velocities, lam, hs)


BA_window.last = {}


# ------------------------------------------------------------------------------------------------ uncertainty
def _query(name, call, iter):
    """``call(eng, it)`` on the engine of the last BA / BA_reg / BA_window call, with the prior on iff that call was ``BA_reg``.
    Returns ``(eng, result, ns, form)``; ``iter`` defaults to that call's."""
    q = _cache.get("last_query")
    eng = _cache.get(q["eng"]) if q is not None else None
    if eng is None or not getattr(eng, "h", None):
        raise RuntimeError(f"{name}() needs a preceding BA / BA_reg / BA_window call")
    it = q["iter"] if iter is None else int(iter)
    if q["reg"]:
        eng.set_prior(True)
    try:
        res = call(eng, it)
    finally:
        if q["reg"]:
            eng.set_prior(False)
    return eng, res, q["ns"], q["form"]


def _shaped(a, counts, form):
    """The used part of a per-window array ``[W, max count, ...]`` in the form of the last call: ``[1, count, ...]``, a dense
    ``[B, count, ...]`` or a list of ``[1, count_b, ...]`` (fp64 torch tensors); None stays None."""
    import torch
    if a is None:
        return None
    if form == "single":
        return torch.from_numpy(np.ascontiguousarray(a[:1, :counts[0]]))
    if form == "dense":
        return torch.from_numpy(np.ascontiguousarray(a[:len(counts), :counts[0]]))
    return [torch.from_numpy(np.ascontiguousarray(a[b:b + 1, :c])) for b, c in enumerate(counts)]


def covariance(iter=None, damped=False, super_diagonal=False):
    """Marginal covariances of the poses at the states the last :func:`BA` / :func:`BA_reg` / :func:`BA_window` call returned
    (``vba_covariance``, ``include/vinsat_ba.h``): the diagonal blocks ``Sigma_ii`` -- and with ``super_diagonal`` the blocks
    ``Sigma_i,i+1`` -- of the inverse of the symmetrised full-phase normal matrix a ``BA(iter)`` call would build there.
    ``iter`` defaults to that call's ``iter`` (its last one for ``BA_window``); the prior is included iff that call was
    ``BA_reg``; ``damped`` adds the damping the next call would start with (the reference's ``JTwJ``).  Coordinates of the
    step: [dp (km), dtheta, dv (km/s)] (attitude sigma = 2 sqrt(Sigma_theta), :func:`pose_sigmas`).  Up to the scale of the
    robust weights, which are normalised by their maximum.

    Shapes follow the last call's form: ``[1, n, 9, 9]`` for one window, ``[B, n, 9, 9]`` for a dense batch, a list of
    ``[1, n_b, 9, 9]`` for a ragged one (fp64 torch tensors).  ``covariance.last["flags"]``: the ``VBA_FLAG_*`` bits per window
    (4: singular -- that window's blocks are NaN; 8: indefinite -- no covariance).  The device states, damping and the bits of
    the following calls are not changed."""
    _, res, ns, form = _query("covariance", lambda eng, it: eng.covariance(it, damped=damped, super_diagonal=super_diagonal), iter)
    diag, sup, flags = res if super_diagonal else (res[0], None, res[1])
    fl = [int(x) for x in flags[:len(ns)]]
    covariance.last = dict(flags=fl[0] if form == "single" else fl)
    return (_shaped(diag, ns, form), _shaped(sup, ns, form)) if super_diagonal else _shaped(diag, ns, form)


covariance.last = {}


def reliability(iter=None, damped=False):
    """Observation reliability at the states the last :func:`BA` / :func:`BA_reg` / :func:`BA_window` call returned
    (``vba_reliability``, ``include/vinsat_ba.h``): per row the leverage ``tr(P_k)``, ``P_k = w_k J_k S_i J_k^T`` with ``S_i`` the
    pose's block of :func:`covariance`, and the standardised residual (w-test) ``sqrt(w_k r_k^T (I - P_k)^-1 r_k)``, both in the
    order of the rows as they were passed in.  ``iter`` defaults to that call's ``iter`` (its last one for ``BA_window``); the
    prior is included iff that call was ``BA_reg``; ``damped`` as in :func:`covariance`.  Up to the same unestimated variance
    factor as :func:`covariance`; a row of weight zero gives 0, 0, a degenerate row or a window without a covariance NaN.

    Returns ``(leverage, wtest)``: ``[1, m]`` tensors for one window, ``[B, m]`` for a dense batch, lists of ``[1, m_b]`` for a ragged
    one (fp64).  ``reliability.last["flags"]``: the ``VBA_FLAG_*`` bits per window as ``covariance.last``; ``["pose_stats"]``: per
    pose the sum of its leverages, its largest finite ``wtest``, its count of rows with non-zero weight (``[1, n, 3]`` / ``[B, n, 3]``
    / a list).  The device states, damping and the bits of the following calls are not changed."""
    eng, (lev, wt, ps, flags), ns, form = _query("reliability", lambda eng, it: eng.reliability(it, damped=damped, pose_stats=True), iter)
    ms = [int(eng.m[b]) for b in range(len(ns))]
    fl = [int(x) for x in flags[:len(ns)]]
    reliability.last = dict(flags=fl[0] if form == "single" else fl, pose_stats=_shaped(ps, ns, form))
    return _shaped(lev, ms, form), _shaped(wt, ms, form)


reliability.last = {}


FIT_FIELDS = ("omega", "m_eff", "leverage_sum", "dof", "s0sq", "wtest_max", "n_flagged", "ext_pos_max")


def outlier_power(iter=None, damped=False, ncp=17.075, crit=None):
    """Outlier power at the states the last :func:`BA` / :func:`BA_reg` / :func:`BA_window` call returned
    (``vba_outlier_power``, ``include/vinsat_ba.h``).  Per row, in the order the rows were passed in: ``mdb``, the minimal
    detectable bias in pixels (the error in the row that the w-test of :func:`reliability` finds with the power ``ncp`` stands
    for -- 17.075: a 0.1 % test, 80 % power -- along the direction it sees worst); ``ext_pos`` (km) and ``ext_att`` (rad), the
    largest displacement of the pose such an undetected error causes; ``del_pos`` (km), how far the pose's position moves if the
    row is removed.  ``iter``, ``damped`` and the prior as in :func:`covariance`.  ``crit``: the critical value rows are
    counted against (``None``: count nothing).  A row of weight zero gives ``inf, 0, 0, 0``, a degenerate row or a window
    without a covariance NaN.

    Returns ``(mdb, ext_pos, ext_att, del_pos, fit)``; the arrays are shaped as :func:`reliability`'s, ``fit`` is one record per
    window (a list for a batch) with the fields ``omega`` (sum of ``w |r|^2``), ``m_eff`` (rows of non-zero weight),
    ``leverage_sum``, ``dof`` (the redundancy ``2 m_eff - leverage_sum``), ``s0sq = omega / dof`` and ``s0 = sqrt(s0sq)``,
    ``wtest_max``, ``n_flagged`` (rows with ``wtest > crit``), ``ext_pos_max`` and ``flags``.  ``s0sq`` is the a-posteriori
    variance factor of the observation class in the units of the normalised weights: ``s0`` scales the sigmas
    (:func:`scaled_sigmas`), ``mdb`` and ``ext_*`` linearly and ``wtest`` inversely; the orbit and attitude factors enter through
    the covariance only.  ``outlier_power.last["pose_fit"]``: per pose ``[.., n, 4]`` the sum of ``w |r|^2``, the sum of
    leverages, the largest finite ``ext_pos``, the rows with ``wtest > crit``.  The device states, damping and the bits of the
    following calls are not changed."""
    import collections
    eng, (*rows, pf, fit, flags), ns, form = _query("outlier_power", lambda eng, it: eng.outlier_power(it, damped=damped, ncp=ncp, crit=crit),
                                                    iter)
    ms = [int(eng.m[b]) for b in range(len(ns))]
    Fit = collections.namedtuple("Fit", FIT_FIELDS + ("s0", "flags"))
    recs = [Fit(*[float(x) for x in fit[b]], s0=float(np.sqrt(fit[b, 4])) if fit[b, 4] >= 0 else float("nan"), flags=int(flags[b]))
            for b in range(len(ns))]
    outlier_power.last = dict(pose_fit=_shaped(pf, ns, form))
    return (*[_shaped(a, ms, form) for a in rows], recs[0] if form == "single" else recs)


outlier_power.last = {}


def snoop(iter=None, damped=False, crit=3.29, scaled=True, mode=0, min_rows=6):
    """Data snooping at the states the last :func:`BA` / :func:`BA_reg` / :func:`BA_window` call returned (``vba_snoop``,
    ``include/vinsat_ba.h``): per pose, the row whose w-test (:func:`reliability`'s) exceeds the critical value by most is rejected
    on the device -- ``mode=1``: every row above it -- as long as the pose keeps ``min_rows`` rows of non-zero weight.  A rejected
    row stays in the window with confidence 0, as if the rows had been passed in so.  ``iter``, ``damped`` and the prior as in
    :func:`covariance`.  ``scaled``: ``crit`` is a quantile of the standard normal distribution (3.29: a 0.1 % test) and is
    multiplied by ``s0`` of :func:`outlier_power`, taken first; a NaN ``s0`` raises, and so does a batch (one critical value per
    call: pass ``scaled=False`` and ``crit`` in the units of ``wtest`` there).

    Returns the cumulative mask of rejected rows shaped as :func:`reliability`'s arrays (bool).  ``snoop.last``: ``counts``
    (``[rejected by this call, in total]`` per window), ``flags`` and the ``crit`` that was used.

    Lifetime: the rejections live on the device until the rows are uploaded again.  A following ``BA`` call with unchanged
    arguments keeps them (and, fed the states the last call returned, stays resident); :func:`invalidate`, changed rows or
    another window lose them.  :func:`rejected` reads them back, :func:`restore_rejected` undoes them."""
    used = float(crit)
    if scaled:
        fit = outlier_power(iter=iter, damped=damped)[-1]
        if isinstance(fit, list):
            raise ValueError("snoop(scaled=True) takes one window: a batch has one s0 per window and a call one critical value")
        if not fit.s0 == fit.s0:
            raise RuntimeError("snoop(scaled=True): s0 of the fit is NaN (no redundancy, or a window without a covariance)")
        used = float(crit) * fit.s0
    eng, (rej, counts, flags), ns, form = _query("snoop", lambda eng, it: eng.snoop(it, used, mode=mode, min_rows=min_rows, damped=damped),
                                                 iter)
    ms = [int(eng.m[b]) for b in range(len(ns))]
    cn = [[int(x) for x in counts[b]] for b in range(len(ns))]
    fl = [int(x) for x in flags[:len(ns)]]
    snoop.last = dict(counts=cn[0] if form == "single" else cn, flags=fl[0] if form == "single" else fl, crit=used)
    return _shaped(rej, ms, form)


snoop.last = {}


def snoop_scaled(iter=None, damped=False, quantile=3.29, mode=0, min_rows=6):
    """:func:`snoop` with ``scaled=True`` in one device call, for one window, a dense batch or a ragged list
    (``vba_snoop_scaled``, ``include/vinsat_ba.h``): every window is tested against ``quantile * s0`` of its own fit (``s0`` of
    :func:`outlier_power`), formed on the device behind one covariance step.  The rule, ``mode``, ``min_rows``, ``iter``,
    ``damped``, the prior and the lifetime of the rejections are :func:`snoop`'s; per window the result is, bit for bit, that of
    ``snoop(crit=quantile, scaled=True)`` on that window alone.

    Returns the cumulative mask of rejected rows shaped as :func:`reliability`'s arrays (bool).  ``snoop_scaled.last``:
    ``counts`` (``[rejected by this call, in total]``), ``flags``, ``crit`` (the critical value used) and ``s0`` -- scalars for
    one window, lists per window for a batch.  A window whose ``s0`` is NaN (no redundancy, no covariance, every confidence zero)
    rejects nothing: for one window that raises, as :func:`snoop` does; in a batch it shows in ``last`` (``crit`` and ``s0`` NaN)."""
    eng, (rej, counts, crit, s0sq, flags), ns, form = _query(
        "snoop_scaled", lambda eng, it: eng.snoop_scaled(it, quantile, mode=mode, min_rows=min_rows, damped=damped), iter)
    B = len(ns)
    ms = [int(eng.m[b]) for b in range(B)]
    cn = [[int(x) for x in counts[b]] for b in range(B)]
    fl = [int(x) for x in flags[:B]]
    cr = [float(x) for x in crit[:B]]
    s0 = [float(np.sqrt(x)) if x >= 0 else float("nan") for x in s0sq[:B]]
    single = form == "single"
    snoop_scaled.last = dict(counts=cn[0] if single else cn, flags=fl[0] if single else fl, crit=cr[0] if single else cr,
                             s0=s0[0] if single else s0)
    if single and not cr[0] == cr[0]:
        raise RuntimeError("snoop_scaled(): s0 of the fit is NaN or zero (no redundancy, or a window without a covariance): "
                           "nothing was rejected")
    return _shaped(rej, ms, form)


snoop_scaled.last = {}


def rejected():
    """The rows :func:`snoop` has rejected since the window's rows were uploaded, shaped as :func:`reliability`'s arrays (bool)."""
    eng, (rej, _), ns, form = _query("rejected", lambda eng, it: eng.rejected(), None)
    return _shaped(rej, [int(eng.m[b]) for b in range(len(ns))], form)


def restore_rejected():
    """Undo every rejection of :func:`snoop` on the engine of the last call: the rows get their confidences back."""
    _query("restore_rejected", lambda eng, it: eng.snoop_restore(-1), None)


def scaled_sigmas(cov, fit):
    """:func:`pose_sigmas` of ``cov`` times ``s0`` of ``fit`` (:func:`outlier_power`): 1-sigma values in km, km/s and rad under the
    a-posteriori variance factor of the observation class.  ``fit``: one record, or a list of records -- one per window of a
    batch (``cov`` a list, or a dense ``[B, n, 9, 9]``)."""
    if isinstance(fit, (list, tuple)) and not hasattr(fit, "s0"):
        if isinstance(cov, (list, tuple)):
            return [scaled_sigmas(c, f) for c, f in zip(cov, fit)]
        per = [scaled_sigmas(cov[b:b + 1], f) for b, f in enumerate(fit)]
        if isinstance(cov, np.ndarray):
            return tuple(np.concatenate([p[k] for p in per]) for k in range(3))
        import torch
        return tuple(torch.cat([p[k] for p in per]) for k in range(3))
    return tuple(x * fit.s0 for x in pose_sigmas(cov))


def pose_sigmas(cov):
    """1-sigma per pose from marginal blocks ``cov [..., n, 9, 9]`` (:func:`covariance`): ``(position [..., n, 3] km,
    velocity [..., n, 3] km/s, attitude [..., n, 3] rad)``.  The step's ``dtheta`` linearises a rotation of angle ``2 dtheta``,
    so the attitude sigma is ``2 sqrt(Sigma_theta)``.  A list (ragged batch) gives a list of tuples; torch in, torch out."""
    if isinstance(cov, (list, tuple)):
        return [pose_sigmas(c) for c in cov]
    is_torch = not isinstance(cov, np.ndarray)
    a = _np(cov) if is_torch else cov
    d = np.diagonal(a, axis1=-2, axis2=-1)
    pos, att, vel = np.sqrt(d[..., 0:3]), 2.0 * np.sqrt(d[..., 3:6]), np.sqrt(d[..., 6:9])
    if is_torch:
        import torch
        return torch.from_numpy(np.ascontiguousarray(pos)), torch.from_numpy(np.ascontiguousarray(vel)), torch.from_numpy(np.ascontiguousarray(att))
    return pos, vel, att
