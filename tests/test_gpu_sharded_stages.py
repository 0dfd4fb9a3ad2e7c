"""The sharded stage kernels (``vba_sh_stage1..4``: vinsat_amd/csrc/vba_sharded_api.hip, vba_shard.hip, the ``abs_all`` branches of
vba_select.hip / vba_select_body.h) layer by layer on emulated ranks: one engine per rank on one GPU, ``torch.cat`` in place of the
all-gathers (tests/emulated_ranks.py).  Behind every stage the ranks' buffers are copied to the host, so each layer answers to a
reference of its own instead of to "the states came out within 1e-9":

  1 keys        ``abs_l[r][:2 m_r]`` EQUALS |uv - est| of the same rows on an unsharded handle at the same states, in the rank's pose-sorted
                order; the rest of the slot is still +inf
  2 select      ``c_obs`` on every rank EQUALS the lower median of all 2 m keys; the branch is predicted from the device's keys
                (``select_reference.predict_gathered``) and, for the select cases, asserted to be the one the case was made for
  3 partial     ``part_l[r]``: 21 n + 6 n sums of w_raw conf J^T J / J^T r against the extended-precision sums of the rank's rows at the
                global median, by the bars of tests/test_gpu_accumulate_paths.py (K x 2^-53, K = max(16, 4 x the oracle's figure on the
                same rows)); exact zeros on poses without rows on that rank; the wmax slot by the bar of the row figure ``w``; the
                sum |r| slot within ``select_reference.sum_bound``
  4 reduction   ``debug("H")``, ``debug("b")`` on every rank EQUAL (((p_0 + p_1) + ...) + p_R-1) / max_q wmax_q in NumPy fp64
  5 decision    ``trial_l[r][1]`` has the same bits on every rank; ``trial_l[r][0]`` against the extended-precision sum of
                ``trial_reference.row_terms`` of the rank's rows (est at the accepted trial states from a second call); ``trial_residual``
                and ``init_residual`` EQUAL ``decide_finish``'s sharded branch evaluated in fp64 in its order (sum_pred from the device's own
                ``r_pred`` in the order of ``dynamics_block``); ``n_trials`` and ``lamda`` equal the unsharded engine's

tests/sharded_stage_cases.py has the windows and the references, tests/test_sharded_stage_cases_host.py their conditions and the
planted faults.  Every test prints its figures (``FIGURES ...``: units of 2^-53 / bar, predicted branch, list length).

Where each test lands:
  test_slices[R-call]       17 poses, 91 rows over 1, 2, 3, 8 ranks: m % R != 0 (padded slots), boundaries inside poses, ranks inside one pose
  test_single_rows[R-call]  R + 1 rows: slices of 2, 1, 1, ...
  test_rejecting[conf]      confidences of 2.2 (four trials rejected, the fifth accepted) and 3 (all nine rejected): ``stage3(None, ...)``
  test_chain[call]          608 poses over 3 ranks: the second trip of k_shard_pack / k_shard_reduce (layers 3, 4; 1, 2 and the exact
                            identities of 5 -- sum_pred over 19 blocks -- ride along)
  test_select[name-mode]    one case per branch of the select over gathered keys (count, digits, overflow-short, overflow-long), +inf
                            padding in the gathered buffer, all keys tied; 8 / 32 keys per thread

What ``overflow-short`` and ``all-tied`` pin: on a sharded handle the compacted list has room for the rank's own 2 m_local keys and is
filled from the keys of all ranks, so a list of 2 m_local < cnt <= 1024 keys has overflowed although it is short enough to be ranked by
counting; only its first 2 m_local entries exist.  ``select_finish_list`` must send it to the digits over all gathered keys (the
counting branch requires cnt <= cap in exact mode); ranking the truncated list gives another key, and not the same one on every rank.

What is NOT compared with a reference: the observation trial sum ``trial_l[r][0]`` of a REJECTED trial.  ``est`` at the trial states
comes from a second call at the states the first one returned, and a rejected trial's states are returned by nobody; so the sum is
judged against ``row_terms`` for the last trial of a call that accepted it (every case but ``rejecting-3``), and the sums of the four
rejected trials of ``rejecting-2.2`` and of all nine of ``rejecting-3`` enter only the exact ``trial_residual`` identity (the last of them)
and the trial counts and damping, which must equal the unsharded engine's.

Measured on the MI355X: the largest figure over the ranks in units of 2^-53 / its bar (layer 3: H over tt, tr, rr; b over t, r; the wmax
and sum |r| slots; layer 5: the observation trial sum of the accepted trial).  Layers 1, 2 and 4 and the two residuals of layer 5 are
exact: every one EQUAL.

  case                      H         b         wmax      sum |r|   trial sum   rounds / trials
  slices R=1 landmark       0.96/16   1.68/16   0.27/16   0.33/29   0.02/16     1 / 1
  slices R=1 full           1.33/16   1.30/16   0.33/16   0.33/29   0.63/16     1 / 1
  slices R=2 landmark       1.25/16   1.68/16   0.27/16   1.71/29   0.91/16     1 / 1
  slices R=2 full           1.23/16   1.00/16   0.33/16   1.71/29   0.21/16     1 / 1
  slices R=3 landmark       1.25/16   1.68/16   0.27/16   0.66/29   0.43/16     1 / 1
  slices R=3 full           1.14/16   1.04/16   0.95/16   0.66/29   1.01/16     1 / 1
  slices R=8 landmark       1.25/16   1.68/16   0.27/16   0.89/29   1.69/16     1 / 1
  slices R=8 full           1.25/16   1.69/16   1.11/16   0.89/29   0.56/16     1 / 1
  head[3] R=2 (both calls)  0.82/16   1.21/16   0.69/16   0.00/29   0.84/16     1 / 1
  head[4] R=3               0.93/16   1.21/16   1.65/16   0.00/29   0.84/16     1 / 1
  head[9] R=8               1.14/16   1.30/16   1.30/16   0.00/29   1.19/16     1 / 1
  rejecting-2.2 R=3         1.12/16   1.40/16   0.27/16   0.66/29   1.04/16     5 / 5 (accepted)
  rejecting-3 R=3           0.94/16   1.01/16   0.27/16   0.66/29   not judged  9 / 9 (none accepted: no states to project at)
  chain R=3 landmark        1.21/16   1.62/16   0.08/16   0.82/29
  chain R=3 full            1.97/16   2.48/16   1.22/16   0.82/29

  select (R = 8, both modes alike)   branch           list   capacity   rank   c_obs = median
  count                              count            512    1024       256    2.699999999674219
  digits                             digits           1032   1040       516    2.6999999980425855
  overflow-short                     overflow-short   200    128        100    2.699999994704285
  overflow-long                      overflow-long    1040   256        520    2.699999998459589
  padded                             count            40     130 / 128  20     2.7000000143486886
  all-tied                           overflow-short   1024   128        511    2.6999999992722223

Nothing comes near a bar.  The carried-keys protocol (``k_sh_front``, ``vba_sh_run_schedule``, ``vba_sh_call``), which needs the
library-issued exchanges and more than one process, is taken exchange by exchange in tests/test_gpu_sharded_carried.py.
"""
import numpy as np
import pytest

import select_cases as SC
import select_reference as S
import sharded_stage_cases as C
import trial_reference as TR

pytestmark = pytest.mark.gpu

_RUNS = {}
MODES = {"latency": 1, "bandwidth": 0}


def run(c, ranks, spec, mode=-1, second=True):
    """One call ``spec`` = (iter, initialize, lamda) on ``c`` over ``ranks`` emulated ranks and on an unsharded handle; every layer's output."""
    key = (c.name, ranks, spec, mode)
    if key in _RUNS:
        return _RUNS[key]
    import torch
    from emulated_ranks import EmulatedRanks
    from vinsat_amd.engine import BAEngine
    it, init, lam = spec
    d = dict(trial=[])

    def after(k, em):
        if k == 1:
            d["abs"] = [a.cpu().numpy().copy() for a in em.abs_l]
        elif k == 2:
            d["part"] = [p.cpu().numpy().copy() for p in em.part_l]
        elif k == 3:
            d["trial"].append([t.cpu().numpy().copy() for t in em.trial_l])

    em = EmulatedRanks(c.n, c.m, ranks, c.xyz, c.uv, c.conf, c.ii, c.K, c.cumrot, c.t, mode=mode, after_stage=after)
    em.set_states(c.states, lam)
    d["rounds"] = em.call(it, init)
    torch.cuda.synchronize()
    d["out"] = em.results()
    what = ("scalars", "H", "b", "est", "Jg", "weight") + (() if init else ("r_pred",))
    d["rank"] = [{w: e.eng.debug(w) for w in what} for e in em.engs]
    d["lat"] = [e.eng.mode()[0] for e in em.engs]
    sc = d["rank"][0]["scalars"]
    d["accepted"] = bool(sc[3] < sc[2])
    if second and d["accepted"]:
        em.after_stage = None
        em.call(it, init)
        d["est2"] = [e.eng.debug("est") for e in em.engs]
    em.close()
    single = BAEngine(c.n, c.m, mode=mode)
    single.upload_observations(c.xyz, c.uv, c.conf, c.ii, c.n)
    single.upload_window(c.K, c.cumrot, c.t)
    single.set_states(c.states, lam)
    single.step(it, init)
    d["single"] = dict(est=single.debug("est"), scalars=single.debug("scalars"), out=single.get_states())
    single.close()
    _RUNS[key] = d
    return d


def sizes(c, ranks):
    return [int(x) for x in np.diff(C.bounds(c.m, ranks))]


def layers_1_2(c, ranks, d, where, branch=None):
    keys = np.abs(c.uv - d["single"]["est"])
    m_pad = -(-c.m // ranks)
    med = S.lower_median(keys)
    bad = []
    for r, m_r in enumerate(sizes(c, ranks)):
        rows = C.rank_rows(c, ranks, r)
        got = d["abs"][r]
        want = SC.device_order(keys[rows], c.ii[rows])
        if got.size != 2 * m_pad or not np.array_equal(S.f64_bits(got[:2 * m_r]), S.f64_bits(want)):
            bad.append(f"{where} rank {r}: the keys of stage 1 are not |uv - est| of its rows in pose-sorted order")
        if not np.all(np.isposinf(got[2 * m_r:])):
            bad.append(f"{where} rank {r}: the padding of its slot is not +inf any more")
        p = S.predict_gathered(keys, m_r)
        c_obs = d["rank"][r]["scalars"][0]
        if r == 0 or c_obs != med:
            print(f"FIGURES {where} rank {r}: {p['branch']}, list {p['cnt']}, capacity {2 * m_r}, rank {p['rank']}, neighbours {p['neighbours']}, "
                  f"{'latency' if d['lat'][r] else 'bandwidth'} set, c_obs {c_obs!r}, median {med!r}")
        if branch is not None and (p["branch"] != branch or p["neighbours"] != 2):
            bad.append(f"{where} rank {r}: made for {branch} with two different neighbours, the device's keys give {p}")
        if c_obs != med:
            bad.append(f"{where} rank {r}: c_obs {c_obs!r}, the lower median of the {2 * c.m} keys is {med!r} ({p['branch']})")
    if d["single"]["scalars"][0] != med:
        bad.append(f"{where}: the unsharded handle's c_obs is not the median of its own keys")
    return bad


def layer_3(c, ranks, d, it, where):
    bad, worst = [], {}
    for r, m_r in enumerate(sizes(c, ranks)):
        rk = d["rank"][r]
        b, figs = C.check_partial(c, C.rank_rows(c, ranks, r), d["part"][r], rk["est"], rk["Jg"], rk["scalars"][0], it,
                                  TR.geometry(c.n, m_r, True)[0], f"{where} rank {r}")
        bad += b
        for k, (f, bar) in figs.items():
            if f >= worst.get(k, (-1.0, 0.0))[0]:
                worst[k] = (f, bar)
    print(f"FIGURES {where} partial: " + " ".join(f"{k}={f:.2f}/{bar:.0f}" for k, (f, bar) in worst.items()))
    return bad


def layer_4(c, ranks, d, where):
    H, b = C.fetched_expected(d["part"], c.n)
    wmax = C.reduce_expected(d["part"], c.n)[2]
    bad = []
    for r in range(ranks):
        rk = d["rank"][r]
        if not (np.array_equal(rk["H"], H) and np.array_equal(rk["b"], b)):
            k = int(np.argmax((rk["H"] != H).any((1, 2)) | (rk["b"] != b).any(1)))
            bad.append(f"{where} rank {r}: H / b behind the reduction are not the rank-ordered fp64 sum of the partials over the largest "
                       f"wmax (first at pose {k}; entry {21 * k} of H, {21 * c.n + 6 * k} of b)")
        if rk["scalars"][1] != wmax:
            bad.append(f"{where} rank {r}: w_max {rk['scalars'][1]!r}, the largest wmax slot is {wmax!r}")
        if not (np.array_equal(rk["H"], d["rank"][0]["H"]) and np.array_equal(rk["b"], d["rank"][0]["b"])):
            bad.append(f"{where} rank {r}: other bits than rank 0")
    print(f"FIGURES {where} reduction: {27 * c.n} entries x {ranks} ranks compared bit for bit")
    return bad


def layer_5(c, ranks, d, spec, where):
    it, init, _lam = spec
    bad = []
    trials = d["trial"][-1]
    if any(S.f64_bits(t[1:2])[0] != S.f64_bits(trials[0][1:2])[0] for t in trials):
        bad.append(f"{where}: the pose-chain part of the trial sum differs between ranks")
    sc0 = d["rank"][0]["scalars"]
    sum_pred = 0.0 if init else C.sum_pred_model(d["rank"][0]["r_pred"], sc0[5])
    want_init, want_trial = C.decide_expected(d["part"], trials, c.n, c.m, init, sum_pred)
    for r in range(ranks):
        sc = d["rank"][r]["scalars"]
        if sc[3] != want_trial:
            bad.append(f"{where} rank {r}: trial_residual {sc[3]!r}, (t[1] + sum_q t[2 q]) / denom is {want_trial!r}")
        if sc[2] != want_init:
            bad.append(f"{where} rank {r}: init_residual {sc[2]!r}, (sum_q sum|r|_q + sum_pred) / denom is {want_init!r}")
    so, ss = d["out"], d["single"]["out"]
    if not (so[3] == ss[3] and so[1] == ss[1] and so[4] == ss[4]):
        bad.append(f"{where}: n_trials / lamda / flags {so[3]}, {so[1]!r}, {so[4]} -- the unsharded engine: {ss[3]}, {ss[1]!r}, {ss[4]}")
    figs = []
    if d["accepted"] and "est2" in d:
        for r in range(ranks):
            rows = C.rank_rows(c, ranks, r)
            f, bar = C.trial_figure(trials[r][0], c.uv[rows], d["est2"][r], d["rank"][r]["weight"], c.ii[rows])
            figs.append((f, bar))
            if not f <= bar:
                bad.append(f"{where} rank {r}: trial sum {trials[r][0]!r} is {f:.3g} x 2^-53 from the sum of its rows' terms (bar {bar:.3g})")
    print(f"FIGURES {where} decision: {d['rounds']} rounds, {so[3]} trials, accepted {d['accepted']}, trial sum "
          + (f"{max(f for f, _ in figs):.2f}/{min(b for _, b in figs):.0f}" if figs else "-")
          + f", init {want_init!r}, trial {want_trial!r}")
    return bad


def all_layers(c, ranks, spec, where, mode=-1):
    d = run(c, ranks, spec, mode)
    bad = layers_1_2(c, ranks, d, where)
    bad += layer_3(c, ranks, d, spec[0], where)
    bad += layer_4(c, ranks, d, where)
    bad += layer_5(c, ranks, d, spec, where)
    return d, bad


# ------------------------------------------------------------------------------------------------ slices
@pytest.mark.parametrize("call", list(C.CALLS))
@pytest.mark.parametrize("ranks", C.SLICE_RANKS)
def test_slices(ranks, call):
    c = C.slices()
    d, bad = all_layers(c, ranks, C.CALLS[call], f"slices R={ranks} {call}")
    assert d["accepted"] and d["rounds"] == 1
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("call", list(C.CALLS))
@pytest.mark.parametrize("ranks", C.SLICE_RANKS[1:])
def test_single_rows(ranks, call):
    c = C.head(ranks + 1)
    assert sizes(c, ranks) == [2] + [1] * (ranks - 1)
    d, bad = all_layers(c, ranks, C.CALLS[call], f"{c.name} R={ranks} {call}")
    assert d["accepted"]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("conf", sorted(C.REJECT_TRIALS))
def test_rejecting(conf):
    c = C.rejecting(conf)
    d, bad = all_layers(c, 3, C.REJECT_CALL, f"{c.name} R=3")
    assert d["out"][3] == C.REJECT_TRIALS[conf] and d["rounds"] >= d["out"][3] and d["accepted"] == (conf == 2.2), (d["out"][3], d["rounds"])
    assert len(d["trial"]) == d["rounds"] > 1, "stage3(None, ...) ran"
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ the long chain
@pytest.mark.parametrize("call", list(C.CALLS))
def test_chain(call):
    c = C.chain()
    spec = C.CALLS[call]
    where = f"chain R={C.CHAIN_RANKS} {call}"
    d = run(c, C.CHAIN_RANKS, spec, second=False)
    bad = layers_1_2(c, C.CHAIN_RANKS, d, where)
    bad += layer_3(c, C.CHAIN_RANKS, d, spec[0], where)
    bad += layer_4(c, C.CHAIN_RANKS, d, where)
    bad += layer_5(c, C.CHAIN_RANKS, d, spec, where)        # (19 blocks of |r_pred|; no second call: the local trial sums are not judged here)
    tail = slice(C.PACK_TRIP, 27 * c.n)
    assert all(np.any(p[tail] != 0.0) for p in d["part"]), "the entries behind the first trip hold sums on every rank"
    assert not bad, "\n".join(bad[:20])


# ------------------------------------------------------------------------------------------------ the select over gathered keys
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(C.SELECT) + ["all-tied"])
def test_select(name, mode):
    c = C.select_case(name)
    R = C.SELECT_RANKS
    where = f"select {name} R={R} {mode}"
    d = run(c, R, (SC.IT, True, SC.LAM), MODES[mode], second=False)
    assert d["lat"] == [MODES[mode]] * R
    bad = layers_1_2(c, R, d, where, branch=C.SELECT_BRANCH[name])
    if name == "padded":
        assert np.isposinf(np.concatenate(d["abs"])).sum() == 2 * 5, "five ranks hold 64 rows in slots of 65: +inf keys were gathered"
    assert not bad, "\n".join(bad)
