"""What the GPU tests of the free-landmark queries share (plain module, no tests): a handle of each KIND -- ``plain``, ``dyn`` (the
dynamics factor), ``att`` (the attitude factor too) -- the C entries of the four features called through raw ``ctypes``, the bitwise
comparisons of the reliability dicts, and the statistics-and-totals block of the three reliability test files, parametrised by kind.
tests/test_gpu_schur_rel.py, test_gpu_schur_dyn_rel.py, test_gpu_schur_att_rel.py, test_gpu_schur_snoop.py, test_gpu_schur_power.py and
test_gpu_schur_query_contract.py use it.
"""
import ctypes

import numpy as np

EPS = np.finfo(np.float64).eps
KINDS = ("plain", "dyn", "att")
NCP = 17.075
_SUFFIX = {"plain": "", "dyn": "_dyn", "att": "_att"}
# the output arrays of the reliability entry of a kind in the entry's order, `fit` last; the SchurBA method that wraps it
REL_OUTPUTS = {"plain": ("leverage", "wtest", "lm_leverage", "lm_wtest", "lm_stats", "pose_stats", "fit")}
REL_OUTPUTS["dyn"] = REL_OUTPUTS["plain"][:-1] + ("edge_leverage", "edge_omega", "fit")
REL_OUTPUTS["att"] = REL_OUTPUTS["dyn"][:-1] + ("att_leverage", "att_wtest", "att_omega", "fit")
REL_METHOD = {"plain": "reliability", "dyn": "state_reliability", "att": "attitude_reliability"}
FIT_LEN = {"plain": 8, "dyn": 10, "att": 13}
# the eleven query entries: name -> (feature, kind)
ENTRIES = {"vba_schur_covariance": ("cov", "plain"), "vba_schur_covariance_dyn": ("cov", "dyn")}
ENTRIES.update({f"vba_schur_{name}{_SUFFIX[k]}": (f, k) for f, name in (("rel", "reliability"), ("snoop", "snoop"), ("power", "outlier_power"))
                for k in KINDS})


def engine(d, dynamics=False, attitude=False, sigma_dyn=None, sigma_att=None, state=None, w=None):
    """A handle on case dict ``d`` at ``state`` (the case's start by default): plain, or with the factors asked for."""
    from vinsat_amd.schur import SchurBA
    kw = dict(time_idx=d["time_idx"], sigma_dyn=d["sigma_dyn"] if sigma_dyn is None else sigma_dyn) if dynamics else {}
    if attitude:
        kw.update(cumrot=d["cumrot"], sigma_att=d["sigma_att"] if sigma_att is None else sigma_att)
    e = SchurBA(d["states0"], d["X0"], d["uv"], d["w"] if w is None else w, d["pose_of_row"], d["landmark_of_row"], d["intrinsics"],
                sigma_prior=d["sigma"], **kw)
    e.set_state(*(state or (d["states0"], d["Xs"])))
    return e


def engine_of(kind, d, **kw):
    return engine(d, dynamics=kind != "plain", attitude=kind == "att", **kw)


def _fitv(rel):
    return np.array(list(rel["fit"].values()))


def _same(outputs):
    """``same(a, b)``: bitwise equal dicts of a query with these array outputs, a ``fit`` dict and ``info`` (NaN equal to NaN)."""
    keys = [k for k in outputs if k != "fit"]

    def same(a, b):
        return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys) and np.array_equal(_fitv(a), _fitv(b), equal_nan=True) and \
            a["info"] == b["info"]
    return same


def _same_cov(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("state", "edges", "landmark"))


def shapes_of(e, entry):
    """The shapes of the double outputs of a covariance, reliability or power entry, in the entry's order."""
    feature, kind = ENTRIES[entry]
    ne = e.n - 1
    if feature == "cov":
        nblk = int(e.structure["blk_i"].size)
        return ((e.n, 6, 6), (nblk, 6, 6), (e.L, 3, 3)) if kind == "plain" else ((e.n, 9, 9), (ne, 9, 9), (nblk, 6, 6), (e.L, 3, 3))
    if feature == "rel":
        extra = {"plain": 0, "dyn": 2, "att": 5}[kind]
        return ((e.m,), (e.m,), (e.L,), (e.L,), (e.L, 3), (e.n, 3)) + ((ne,),) * extra + ((FIT_LEN[kind],),)
    assert feature == "power"
    return ((e.m,),) * 6 + ((e.L,),) * 3 + ((e.n, 4), (FIT_LEN[kind] + 4,))


def raw_query(e, entry, lam, on=None, handle=True, info=True, ncp=NCP, crit=None, scaled=1, min_rows=6, min_track=3):
    """The C entry itself on handle ``e``: ``(rc, info, outputs in the entry's order, device row order)``; outputs not asked for
    (``on[k]`` false) are None (NULL), the others start at 7.  A snoop entry gives ``(rc, info, counts [3], crit_used)`` and takes
    ``crit = inf`` (nothing rejected) unless told otherwise; a power entry ``crit = 3.29``.  ``handle=False`` / ``info=False`` pass
    NULL in their place."""
    from vinsat_amd._lib import PD
    feature, _ = ENTRIES[entry]
    fn, h = getattr(e.lib, entry), e.h if handle else None
    word = ctypes.c_int(-1)
    pinfo = ctypes.byref(word) if info else None
    if feature == "snoop":
        counts, used = (ctypes.c_int * 3)(-1, -1, -1), ctypes.c_double(7.0)
        rc = fn(h, float(lam), float("inf") if crit is None else float(crit), int(scaled), int(min_rows), int(min_track), counts,
                ctypes.byref(used), pinfo)
        return rc, word.value, list(counts), used.value
    shapes = shapes_of(e, entry)
    bufs = [np.full(s, 7.0) if o else None for s, o in zip(shapes, on or (True,) * len(shapes))]
    ptrs = [b.ctypes.data_as(PD) if b is not None else None for b in bufs]
    args = (float(ncp), 3.29 if crit is None else float(crit)) if feature == "power" else ()
    rc = fn(h, float(lam), *args, *ptrs, pinfo)
    return (rc, word.value, *bufs)


def _raw(kind, e, lam, on=None):
    """The reliability entry of this kind: ``(rc, info, outputs in the order of REL_OUTPUTS[kind])``."""
    return raw_query(e, "vba_schur_reliability" + _SUFFIX[kind], lam, on)


def last_error(e):
    msg = e.lib.vba_schur_last_error()
    return msg.decode() if msg else ""


def fin_max(a):
    a = np.asarray(a)
    return float(np.max(a[np.isfinite(a)], initial=0.0))


def statistics_and_totals(kind, T, d, e, got, r=None):
    """The statistics and totals of a reliability dict ``got`` of a handle of this kind against the device's own arrays (sums to the
    rounding of another order, maxima and counts exactly) and, with the reference ``r`` of the cases module ``T``, against it: what
    the file of each kind has always asserted, with its tolerances (``lm_stats[:, 2]`` against the reference on ``dyn`` only)."""
    w, fit = d["w"], got["fit"]
    for key, index, size in (("lm_stats", d["landmark_of_row"], e.L), ("pose_stats", d["pose_of_row"], e.n)):
        own = T.stats_of(got["leverage"], got["wtest"], w, index, size)
        # (a sum of t non-negative terms in another order: within t eps of it)
        assert np.abs(got[key][:, 0] - own[:, 0]).max() <= np.bincount(index).max() * EPS * np.abs(own[:, 0]).max()
        assert np.array_equal(got[key][:, 1:], own[:, 1:])
        if r is not None:
            ref = getattr(r, key)
            assert T.rel(got[key][:, 0], ref[:, 0]) <= T.bar(r, "leverage") and T.rel(got[key][:, 1], ref[:, 1]) <= T.bar(r, "wtest")
            if kind == "dyn":
                assert np.array_equal(got[key][:, 2], ref[:, 2])
    assert fit["m_eff"] == float((w > 0).sum()) and fit["max_wtest"] == fin_max(got["wtest"]) and fit["max_lm_wtest"] == fin_max(got["lm_wtest"])
    if r is not None:
        assert fit["m_eff"] == r.fit["m_eff"]
    ne = e.n - 1
    traces = [("t_rows", "leverage", e.m), ("t_prior", "lm_leverage", e.L)]
    sums = []
    rho = 2.0 * fit["m_eff"] + 3.0 * e.L
    if kind != "plain":
        traces.append(("t_edges", "edge_leverage", ne))
        sums.append(("omega_edges", "edge_omega", ne))
        rho = rho + 6.0 * ne
    if kind == "att":
        assert fit["max_att_wtest"] == fin_max(got["att_wtest"])
        traces.append(("t_att", "att_leverage", ne))
        sums.append(("omega_att", "att_omega", ne))
        rho = rho + 3.0 * ne
    for k, own, cnt in traces + sums:
        assert abs(fit[k] - got[own].sum()) <= cnt * EPS * abs(fit[k]), k
    for k, _, _ in traces:
        rho = rho - fit[k]
    assert fit["rho"] == rho
    assert fit["s0sq"] == fit["omega"] / fit["rho"]
    if r is not None:
        # (a trace within the bar of its family, relative to the largest entry, times the number of entries)
        for k, fam, cnt in traces:
            assert abs(fit[k] - r.fit[k]) <= cnt * getattr(r, fam).max() * T.bar(r, fam), k
        assert abs(fit["rho"] - r.fit["rho"]) <= 1e-9 * r.unknowns and abs(fit["s0sq"] - r.fit["s0sq"]) <= 1e-9 * r.fit["s0sq"]
