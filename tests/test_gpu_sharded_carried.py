"""The carried-keys protocol of the observation-sharded mode (``k_sh_front``, ``vba_sh_run_schedule``, ``vba_sh_call``:
vinsat_amd/csrc/vba_shard.hip, vba_sharded_api.hip) exchange by exchange.  Every layer boundary of this protocol is an all-gather, and
the test double of RCCL (tests/fake_rccl/) stages each one through host memory: its tap records, per all-gather, the element count, the
bytes the rank sent and the bytes it received.  Each rank is one process (``mp.spawn``, a gloo control group, every rank on device 0);
a world size is spawned ONCE per session, every rank runs all scenarios of ``sharded_carried_cases.scenarios(R)`` and writes one
``.npz`` with the tap records next to the debug fetches; the parent judges them.  Every handle is created for exactly ceil(m / R)
rows, and every call first proves from the tap's element counts that the carried path ran (a handle that quietly takes the round-3
protocol gathers 2 doubles per trial on EVERY call and no exchange of lenA: it fails layer a).

Per ``vba_sh_call`` k and rank r:
  a pattern     the tap holds exactly B (lenB), C (27 n + 2), A (lenA) on carried keys; keys (2 m_pad), C, A without; a missed select
                repeats the call (keys, C, A); a stalled call adds 2 doubles per LM trial and A once more -- predicted from the carried
                flag, the front model, ``n_trials`` and the unsharded engine stepped alongside, never read back from the tap
  b exchange A  as sent behind call k: the 2048 histogram words EQUAL the histogram of r's next keys under ``warm_lo`` =
                ``warm_range_start`` of the bits of ``c_obs`` (the same on all ranks) at shift 44; the keys EQUAL |uv - est| at the
                returned states (est of call k + 1); ``part_next`` / ``part_trial`` within K x 2^-53 of the extended-precision sums of
                r's rows, K = max(16, 4 x fp64 NumPy's figure on the same terms) as in tests/test_gpu_trial_paths.py
  c front       bin, in-bin rank, ``in_bin`` and hit / miss follow from the gathered A by ``sharded_carried_cases.front_model``; B as
                sent is [count, keys ...]: count EQUALS r's histogram word of the bin, the keys as a sorted multiset of bit patterns
                EQUAL r's next keys of that bin; every rank received the same bytes (every exchange)
  d median      ``c_obs`` on every rank EQUALS the lower median of all ranks' next keys (hit and miss); a key exchange EQUALS r's keys
                in device order followed by +inf up to 2 m_pad
  e partial     C as sent passes ``sharded_stage_cases.check_partial`` on r's rows at that ``c_obs`` (the bars of layer 3 of the stage
                tests); slot 27 n + 1 is judged on a key exchange only (unused with carried keys), the wmax slot when R > 1 or on a key
                exchange (``V.wmax_ext`` is set for R > 1 only)
  f reduction   R > 1: ``debug("H")`` / ``debug("b")`` EQUAL ``fetched_expected`` of the gathered partials.  R = 1: the received bytes EQUAL
                the sent ones and H / b are NOT fetched -- the sums live in the exchange buffer there (the gathered copy is the sum) and
                ``vba_debug_fetch`` reads the handle's own array
  g decision    ``init_residual`` / ``trial_residual`` EQUAL the model's from the gathered A of the call's trial (a stalled call: from its
                last 2-double exchange, pose-chain part identical on all ranks); ``n_trials``, ``lamda``, flags equal the unsharded
                engine's; the states have the same bits on every rank

The double synchronises the stream at every exchange and all ranks share one GPU: the asynchrony of the real chain is not under test.

Where each test lands:
  test_stepped[R-case]     slices (17 poses, 91 rows: m % R != 0, cuts inside poses) and head (R + 1 rows) at R = 1, 2, 3: two landmark-only
                           calls, two full calls, layers a-g per call
  test_chained[R-kind]     the same calls as one schedule and as two (the second starts from carried keys; accept tests folded into the
                           next front): as many records, the same counts and the same bits in every sent buffer as stepped, same states
  test_stalled[conf-how]   rejecting(2.2) / rejecting(3) at R = 3, stepped and in a chain: 2 doubles per trial, ``fallbacks_lm`` + 1 per call
  test_miss[name]          one window per reason the front can miss for, each with the reason the model predicts, ``fallbacks_miss`` + 1 and
                           layers a-g of the repeated call: forced (``set_warm_select(2)``, R = 1, 2, 3: the reason the older tests
                           already exercised); overflow-one-rank (R = 3, cap 8: 10 / 8 / 4 keys of the median's bin) with its twin
                           (8 / 8 / 4: a hit on a bin of 20 keys, wanted rank 16); long-bin (R = 5, 1500 rows, 205 keys per rank =
                           1025) with its twin (1024 keys: a hit, wanted rank 1019); leaving (R = 3, the median falls from 40 px to
                           under one: bin 0).  The twins are the hit windows with a populated median bin: buckets of several keys per
                           rank in layer c, the median ranked from the gathered buckets far inside the list in layer d
  test_reupload[R]         rows split the other way round on live handles: key exchange with +inf padding, then carried again
  test_every_reason        forced, overflow, long and leaving were each reached on the GPU (``lo == ~0``: unreachable, stays out)

The last call of a scenario has no call behind it whose ``est`` would be the projection at the states it returned; a fresh handle of
the rank's rows is set to those states and stepped once for that ``est`` (the same projection kernel), so layer b holds for every call.

Measured on the MI355X: the largest figure over ranks and calls in units of 2^-53 / its bar.  Every EQUAL held; layers a, c, d, f, g
are exact.  part_obs / part_dyn / part_next: the observation and pose-chain slots of ``part_trial`` and ``part_next`` in exchange A.
  scenario                H tt   tr   rr  /bar  b t    r   /bar  wmax     sum |r|  part_obs part_dyn part_next  front of the carried calls
  slices R=1              2.08 2.00 1.97 /16    2.34 2.18 /16    0.27/16  0.33/29  1.04/16  1.07/16  0.90/16    hit, 1 key in the bin
  slices R=2              1.65 1.46 1.34 /16    1.92 1.81 /16    1.97/16  1.71/29  0.91/16  1.63/16  0.84/16    hit, 1 key
  slices R=3              1.37 1.52 1.60 /16    1.70 1.89 /16    1.50/16  0.66/29  0.91/16  0.75/16  0.96/16    hit, 1 key
  forced R=1              2.08 2.00 1.97 /16    2.34 2.18 /16    1.32/16  0.33/29  0.13/16  0.33/16  0.25/16    predicted forced, observed forced
  forced R=2              1.43 1.46 1.26 /16    1.86 1.81 /16    1.97/16  1.71/29  0.91/16  1.63/16  0.84/16    predicted forced, observed forced
  forced R=3              1.37 1.52 1.60 /16    1.70 1.89 /16    1.50/16  0.96/29  0.73/16  0.75/16  0.96/16    predicted forced, observed forced
  overflow-one-rank R=3   1.15 1.65 1.22 /16    0.78 0.60 /16    0.97/16  0.00/29  0.92/16  0.00/16  0.00/16    predicted overflow (rank 0), observed overflow
  overflow-twin R=3       1.16 1.40 1.11 /16    0.88 0.80 /16    0.85/16  0.00/29  1.17/16  0.00/16  0.00/16    predicted hit, observed hit: rank 16 of 20
  long-bin R=5            1.18 1.13 0.94 /16    0.64 0.86 /16    1.09/16  0.73/29  1.87/16  0.00/16  0.60/16    predicted long (1025 keys), observed long
  long-twin R=5           1.16 1.02 1.18 /16    0.47 0.44 /16    0.76/16  0.94/29  1.79/16  0.00/16  0.62/16    predicted hit, observed hit: rank 1019 of 1024
  leaving R=3             0.91 1.33 1.02 /16    1.33 1.53 /16    0.49/16  1.20/29  1.15/16  0.00/16  0.00/16    predicted leaving (bin 0), observed leaving
  rejecting-2.2 R=3       1.36 1.40 1.95 /16    1.41 1.95 /16    1.71/16  0.66/29  1.13/16  0.00/16  0.82/16    5 and 2 trials; chained: 18 exchanges
  rejecting-3 R=3         0.94 1.11 0.97 /16    1.30 1.78 /16    0.38/16  0.66/29  0.50/16  0.00/16  0.00/16    9 and 3 trials; chained: 23 exchanges
  chain, chain2 R=1,2,3   12 exchanges each, every sent buffer with the bits of the stepped run; the same states and damping
head (R + 1 rows) and reupload print their lines in the same form and stay under 2.2 / 16 throughout.  A pose-chain figure of 0.00 is a
scenario of landmark-only calls (nothing is summed there; the slots must be, and are, exactly 0).  Nothing comes near a bar.
"""
import ctypes
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import select_cases as SC
import select_reference as S
import sharded_carried_cases as K
import sharded_stage_cases as C
import trial_reference as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE_DIR = os.path.join(ROOT, "tests", "fake_rccl")
FAKE = os.path.join(FAKE_DIR, "libfake_rccl.so")
pytestmark = pytest.mark.gpu

_RUNS = {}
REACHED = {}
FETCH = ("scalars", "est", "Jg", "weight")


# ------------------------------------------------------------------------------------------------ the rank process
def _drain(tap, seen, out, key):
    n = tap.fake_rccl_tap_count()
    out[f"{key}.ntap"] = np.array(n - seen)
    for j, i in enumerate(range(seen, n)):
        cnt, el, nr = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_int()
        assert tap.fake_rccl_tap_info(i, ctypes.byref(cnt), ctypes.byref(el), ctypes.byref(nr)) == 0 and el.value == 8
        sent, recv = np.empty(cnt.value), np.empty(cnt.value * nr.value)
        assert tap.fake_rccl_tap_copy(i, sent.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(sent.nbytes),
                                      recv.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(recv.nbytes)) == 0
        out[f"{key}.tap{j}.sent"], out[f"{key}.tap{j}.recv"] = sent, recv
    return n


def _worker(rank, world, port, tmp):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    import sharded_carried_cases as K
    from vinsat_amd.dist import HipStageEngine, ShardedBA
    from vinsat_amd.engine import BAEngine
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        tap = ctypes.CDLL(FAKE)
        tap.fake_rccl_tap_enable(1)
        seen = 0
        out = {}
        for name, ops in K.scenarios(world).items():
            c, cap, forced = K.case_of(name, world)
            m_pad = -(-c.m // world)
            b = K.split_bounds(c.m, world, False)
            lo, hi = int(b[rank]), int(b[rank + 1])
            e = BAEngine(c.n, m_pad)                    # exactly ceil(m / R) rows: the carried-keys protocol
            if forced:
                e.set_warm_select(2)
            if cap:
                e.set_bucket_cap(cap)
            e.upload_observations(c.xyz[lo:hi], c.uv[lo:hi], c.conf[lo:hi], c.ii[lo:hi], c.n)
            e.upload_window(c.K, c.cumrot, c.t)
            stage = HipStageEngine(e, torch_stream=False)
            stage.attach_rccl(dist, None, FAKE)
            sb = ShardedBA(stage, c.n, hi - lo, c.m)
            sb.set_states(c.states, K.lam0_of(name))
            single = None
            if rank == 0:
                single = BAEngine(c.n, c.m)
                single.upload_observations(c.xyz, c.uv, c.conf, c.ii, c.n)
                single.upload_window(c.K, c.cumrot, c.t)
                single.set_states(c.states, K.lam0_of(name))
            for k, op in enumerate(ops):
                key = f"{name}.{k}".replace("/", "__")
                if op[0] == "reupload":
                    b = K.split_bounds(c.m, world, True)
                    lo, hi = int(b[rank]), int(b[rank + 1])
                    e.upload_observations(c.xyz[lo:hi], c.uv[lo:hi], c.conf[lo:hi], c.ii[lo:hi], c.n)
                    sb.m_local = hi - lo
                    sb.set_states(c.states, K.lam0_of(name))
                    if single is not None:
                        single.set_states(c.states, K.lam0_of(name))
                    continue
                calls = [(op[1], op[2])] if op[0] == "step" else list(op[1])
                if op[0] == "step":
                    out[f"{key}.ret"] = np.array(sb.step(op[1], op[2]))
                else:
                    out[f"{key}.ret"] = np.array(sb.run_schedule([q[0] for q in calls], [q[1] for q in calls]))
                seen = _drain(tap, seen, out, key)
                for w in FETCH + (("H", "b") if world > 1 else ()) + (() if calls[-1][1] else ("r_pred",)):
                    out[f"{key}.{w}"] = e.debug(w)
                nx = e.debug_next()
                out[f"{key}.keys"], out[f"{key}.warm_lo"], out[f"{key}.shift"] = nx["keys"], np.array(nx["warm_lo"], dtype=np.uint64), np.array(nx["shift"])
                geo = e.debug_trial()
                out[f"{key}.geo"] = np.array([geo[q] for q in ("nblk_obs", "nblk_dyn", "nblk_long", "cap")] + [geo["part_trial"].size])
                st = sb.get_states()
                out[f"{key}.states"], out[f"{key}.res"] = st[0], np.array([st[1], st[3], st[4]])
                out[f"{key}.stats"] = np.array(stage.stats())
                if single is not None:
                    for it, init in calls:
                        single.step(it, init)
                    ss = single.get_states()
                    out[f"{key}.single"] = np.array([ss[1], ss[3], ss[4]])
                    out[f"{key}.single_sc"] = single.debug("scalars")
            # est at the states the last call returned: the projection kernel of a fresh handle of this rank's rows at those states
            last = f"{name}.{len(ops) - 1}".replace("/", "__")
            e2 = BAEngine(c.n, m_pad)
            e2.upload_observations(c.xyz[lo:hi], c.uv[lo:hi], c.conf[lo:hi], c.ii[lo:hi], c.n)
            e2.upload_window(c.K, c.cumrot, c.t)
            e2.set_states(out[f"{last}.states"], K.lam0_of(name))
            e2.step(0, True)
            out[f"{last}.est_after"] = e2.debug("est")
            e2.close()
            sb.close()
            if single is not None:
                single.close()
        out["overflowed"] = np.array(tap.fake_rccl_tap_overflowed())
        np.savez(os.path.join(tmp, f"rank{rank}.npz"), **out)
    finally:
        dist.destroy_process_group()


def world_run(world, tmp_path_factory):
    """The ``.npz`` of every rank of world size ``world`` (spawned once; a failed spawn is remembered, not repeated)."""
    assert world <= K.MAX_WORLD
    if world not in _RUNS:
        _RUNS[world] = None
        if not os.path.exists(FAKE) or os.path.getmtime(FAKE) < os.path.getmtime(os.path.join(FAKE_DIR, "fake_rccl.cpp")):
            subprocess.check_call(["make", "-C", FAKE_DIR], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        tmp = tmp_path_factory.mktemp(f"carried{world}")
        with socket.socket() as sk:                 # a free port for the gloo rendezvous
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        mp.spawn(_worker, args=(world, port, str(tmp)), nprocs=world, join=True)
        _RUNS[world] = [dict(np.load(tmp / f"rank{r}.npz")) for r in range(world)]
    if _RUNS[world] is None:
        pytest.fail(f"the ranks of world size {world} failed before (not spawned again)")
    assert all(int(d["overflowed"]) == 0 for d in _RUNS[world]), "the tap ran out of room: records are missing"
    return _RUNS[world]


# ------------------------------------------------------------------------------------------------ judging one scenario
class Scenario:
    def __init__(self, data, name, world):
        self.D, self.name, self.R = data, name, world
        self.c, self.cap_set, self.forced = K.case_of(name, world)
        self.ops = K.scenarios(world)[name]
        self.m_pad = -(-self.c.m // world)
        self.figs = {}

    def get(self, r, k, what):
        return self.D[r][f"{self.name}.{k}.{what}".replace("/", "__")]

    def taps(self, r, k):
        n = int(self.get(r, k, "ntap"))
        return [(self.get(r, k, f"tap{j}.sent"), self.get(r, k, f"tap{j}.recv")) for j in range(n)]

    def note(self, k, f, bar):
        cur = self.figs.get(k, (-1.0, 0.0))
        if f >= cur[0]:
            self.figs[k] = (float(f), float(bar))

    def rows(self, b, r):
        return slice(int(b[r]), int(b[r + 1]))


def _bits(a):
    return TR.f64_bits(np.asarray(a, dtype=np.float64).reshape(-1))


def judge(sc, stop_after=None):
    """Layers a-g of every ``step`` operation of scenario ``sc``: ([] or what is wrong, what happened per call)."""
    c, R, n = sc.c, sc.R, sc.c.n
    bad, log = [], []
    bounds = K.split_bounds(c.m, R, False)
    carried, prev, states_in = False, None, c.states
    stats_prev = np.array([0, 0, 0])
    for k, op in enumerate(sc.ops):
        if op[0] == "reupload":
            bounds, carried, prev, states_in = K.split_bounds(c.m, R, True), False, None, c.states
            continue
        assert op[0] == "step"
        it, init = op[1], op[2]
        where = f"{sc.name} R={R} call {k}"
        geo = [int(v) for v in sc.get(0, k, "geo")]
        nbo, nbd, nbl, cap, stride = geo
        lenA, lenB = K.len_a(nbo, stride), K.len_b(cap)
        assert all(np.array_equal(sc.get(r, k, "geo"), sc.get(0, k, "geo")) for r in range(R)), f"{where}: the ranks' geometry differs"
        assert nbo == -(-sc.m_pad // 256) and (sc.cap_set == 0 or cap == sc.cap_set), (where, geo)
        taps = [sc.taps(r, k) for r in range(R)]
        scal = [sc.get(r, k, "scalars") for r in range(R)]
        res = [sc.get(r, k, "res") for r in range(R)]
        stats = sc.get(0, k, "stats")
        single, single_sc = sc.get(0, k, "single"), sc.get(0, k, "single_sc")
        ntr = int(res[0][1])
        # ---- c (first half): what the front must have resolved from the gathered A of the call in front
        fm = None
        if carried:
            slotsA = np.asarray(prev["A_recv"]).reshape(R, -1)
            fm = K.front_resolve(list(slotsA), c.m, cap, prev["warm_lo"], sc.forced)
            fm["sum_in"] = K.front_sums(list(slotsA), nbo, prev["nchain"])[0]
        missed = bool(carried and not fm["hit"])
        stalled_pred = bool(single[1] > 1 or not single_sc[3] < single_sc[2])
        stalled = int(stats[2] - stats_prev[2]) == 1
        if stalled != stalled_pred:
            bad.append(f"{where}: fallbacks_lm rose by {int(stats[2] - stats_prev[2])}, the unsharded engine took {int(single[1])} trials")
        if int(stats[1] - stats_prev[1]) != int(missed):
            bad.append(f"{where}: fallbacks_miss rose by {int(stats[1] - stats_prev[1])}, the model of the front says "
                       f"{'miss (' + str(fm['reasons']) + ')' if missed else 'hit'}")
        # ---- a: the exchange pattern
        want = K.pattern(carried, missed, stalled_pred, ntr, lenA, lenB, n, sc.m_pad)
        for r in range(R):
            got = [t[0].size for t in taps[r]]
            if got != want:
                bad.append(f"{where} rank {r}: all-gathers of {got} elements, the protocol prescribes {want} "
                           f"(carried {carried}, missed {missed}, stalled {stalled_pred}, {ntr} trials)")
        if bad and any("prescribes" in x for x in bad):
            return bad, log                                         # (the records cannot be told apart any further)
        for r in range(1, R):
            for j, (t0, tr) in enumerate(zip(taps[0], taps[r])):
                if not np.array_equal(_bits(t0[1]), _bits(tr[1])):
                    bad.append(f"{where}: rank {r} received other bytes than rank 0 in exchange {j}")
        if R == 1 and any(not np.array_equal(_bits(s), _bits(v)) for s, v in taps[0]):
            bad.append(f"{where}: one rank, and the received bytes are not the sent ones")
        base = 3 if missed else 0
        rec_front, rec_C, rec_A = [[taps[r][base + j] for r in range(R)] for j in range(3)]
        key_exchange = missed or not carried
        if stalled_pred:
            rounds = [[taps[r][base + 3 + j] for r in range(R)] for j in range(ntr)]
            rec_A = [taps[r][base + 3 + ntr] for r in range(R)]
        est = [sc.get(r, k, "est") for r in range(R)]
        uv = [c.uv[sc.rows(bounds, r)] for r in range(R)]
        ii = [c.ii[sc.rows(bounds, r)] for r in range(R)]
        own_keys = [prev["keys"][r] if carried else np.abs(uv[r] - est[r]) for r in range(R)]
        # ---- c: the bucket exchange
        if carried:
            log.append((k, "miss" if missed else "hit", fm["reasons"], fm["bin"], fm["rank"], fm["in_bin"], fm["over"]))
            REACHED.setdefault(fm["reason"], []).append(where)
            print(f"FIGURES {where} front: bin {fm['bin']}, rank {fm['rank']} of {fm['in_bin']} in the bin, cap {cap}, "
                  f"{'MISS ' + str(fm['reasons']) if missed else 'hit'}, over {fm['over']}")
            if not missed:
                for r in range(R):
                    bad += [f"{where} rank {r}: {x}" for x in K.check_bucket(rec_front[r][0], prev["keys"][r], prev["warm_lo"], fm["bin"],
                                                                              fm["own"][r][fm["bin"]])]
        # ---- d: the median; the key exchange
        for r in range(R):
            bad += [f"{where} rank {r}: {x}" for x in K.check_median(scal[r][0], own_keys)]
            if key_exchange:
                bad += [f"{where} rank {r}: {x}" for x in K.check_key_exchange(rec_front[r][0], own_keys[r], ii[r], sc.m_pad)]
        # ---- e: the partial
        cs = K.with_states(c, states_in)
        for r in range(R):
            b2, figs = C.check_partial(cs, sc.rows(bounds, r), rec_C[r][0], est[r], sc.get(r, k, "Jg"), scal[r][0], it, nbo, f"{where} rank {r}",
                                       wmax_slot=R > 1 or key_exchange, sum_slot=key_exchange)
            bad += b2
            for q, (f, bar) in figs.items():
                sc.note(q, f, bar)
        # ---- f: the reduction
        parts = list(np.asarray(rec_C[0][1]).reshape(R, -1))
        if R > 1:
            H, b = C.fetched_expected(parts, n)
            for r in range(R):
                if not (np.array_equal(sc.get(r, k, "H"), H) and np.array_equal(sc.get(r, k, "b"), b)):
                    bad.append(f"{where} rank {r}: H / b are not the rank-ordered fp64 sum of the gathered partials over the largest wmax")
        if R > 1 or key_exchange:
            wmax = C.reduce_expected(parts, n)[2]
            bad += [f"{where} rank {r}: w_max {scal[r][1]!r}, the largest wmax slot is {wmax!r}" for r in range(R) if scal[r][1] != wmax]
        # ---- g: the decision
        slotsT = list(np.asarray(rec_A[0][1]).reshape(R, -1))
        nchain = nbd + (0 if init else nbl)
        sum_in = C.reduce_expected(parts, n)[3] if key_exchange else fm["sum_in"]
        sum_pred = 0.0 if init else C.sum_pred_model(sc.get(0, k, "r_pred"), scal[0][5])
        if stalled_pred:
            t_all = np.asarray(rounds[-1][0][1])
            sh = float(t_all[1])
            for q in range(R):
                sh = sh + float(t_all[2 * q])
            for j, rnd in enumerate(rounds):
                ta = np.asarray(rnd[0][1])
                if np.unique(_bits(ta[1::2])).size != 1:
                    bad.append(f"{where}: LM round {j}: the pose-chain part of the trial sum differs between ranks")
        else:
            sh = K.front_sums(slotsT, nbo, nchain)[1]
        want_init, want_trial = K.residuals(sum_in, sum_pred, sh, n, c.m, init)
        for r in range(R):
            if scal[r][2] != want_init:
                bad.append(f"{where} rank {r}: init_residual {scal[r][2]!r}, the model gives {want_init!r}")
            if scal[r][3] != want_trial:
                bad.append(f"{where} rank {r}: trial_residual {scal[r][3]!r}, the model gives {want_trial!r}")
            if not np.array_equal(res[r], res[0]) or not np.array_equal(_bits(sc.get(r, k, "states")), _bits(sc.get(0, k, "states"))):
                bad.append(f"{where} rank {r}: other states / lamda / trials / flags than rank 0")
        if not np.array_equal(res[0], single):
            bad.append(f"{where}: lamda / n_trials / flags {res[0].tolist()}, the unsharded engine: {single.tolist()}")
        accepted = bool(scal[0][3] < scal[0][2])
        # ---- b: exchange A as sent behind this call
        warm_lo = TR.warm_range_start(int(_bits([scal[0][0]])[0]), K.SHIFT)
        nxt = k + 1 < len(sc.ops) and sc.ops[k + 1][0] == "step"
        out_states = sc.get(0, k, "states")
        for r in range(R):
            hist, pn, pt = K.split_a(rec_A[r][0], nbo, stride)
            keys = sc.get(r, k, "keys")
            if int(sc.get(r, k, "warm_lo")) != warm_lo or int(sc.get(r, k, "shift")) != K.SHIFT:
                bad.append(f"{where} rank {r}: warm_lo {int(sc.get(r, k, 'warm_lo')):#x} at shift {int(sc.get(r, k, 'shift'))}, "
                           f"warm_range_start of c_obs at shift 44 is {warm_lo:#x}")
            if not np.array_equal(hist.astype(np.int64), K.own_hist(keys, warm_lo)):
                bad.append(f"{where} rank {r}: the histogram it sent in A is not the histogram of its next keys")
            if nxt or k == len(sc.ops) - 1:
                est2 = sc.get(r, k + 1, "est") if nxt else sc.get(r, k, "est_after")
                bad += [f"{where} rank {r}: {x}" for x in TR.check_keys(keys, uv[r], est2)]
                if accepted:
                    ref, bars, nl = K.slot_bars(c, sc.rows(bounds, r), est2, sc.get(r, k, "weight"), out_states, scal[r][5], init, sc.m_pad)
                    exact = []
                    figs = TR.slot_figures(ref, pt, pn, nl, exact)
                    bad += [f"{where} rank {r}: {x}" for x in exact]
                    for q, v in figs.items():
                        f = float(np.max(v)) / TR.U if np.size(v) else 0.0
                        sc.note(q, f, bars[q])
                        if not f <= bars[q]:
                            bad.append(f"{where} rank {r}: {q} is {f:.3g} x 2^-53 from the sum of its terms (bar {bars[q]:.3g})")
        prev = dict(A_recv=rec_A[0][1], warm_lo=warm_lo, keys=[sc.get(r, k, "keys") for r in range(R)], nchain=nchain)
        carried, states_in, stats_prev = True, out_states, stats
    print(f"FIGURES {sc.name} R={R}: " + " ".join(f"{q}={f:.2f}/{bar:.0f}" for q, (f, bar) in sc.figs.items()))
    return bad, log


def scenario(tmp_path_factory, world, name):
    return Scenario(world_run(world, tmp_path_factory), name, world)


# ------------------------------------------------------------------------------------------------ stepped calls
@pytest.mark.parametrize("case", ["slices", "head"])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_stepped(tmp_path_factory, world, case):
    sc = scenario(tmp_path_factory, world, f"{case}/step")
    bad, log = judge(sc)
    assert not bad, "\n".join(bad[:30])
    assert [x[1] for x in log] == ["hit"] * 3, log


# ------------------------------------------------------------------------------------------------ chained
def _all_taps(sc, r):
    return [t for k, op in enumerate(sc.ops) if op[0] != "reupload" for t in sc.taps(r, k)]


@pytest.mark.parametrize("kind", ["chain", "chain2"])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_chained(tmp_path_factory, world, kind):
    """No slot is exempt: every sent buffer of the chained run has the bits of the stepped run."""
    st, ch = scenario(tmp_path_factory, world, "slices/step"), scenario(tmp_path_factory, world, f"slices/{kind}")
    bad = []
    for r in range(world):
        a, b = _all_taps(st, r), _all_taps(ch, r)
        if [t[0].size for t in a] != [t[0].size for t in b]:
            bad.append(f"rank {r}: chained exchanges of {[t[0].size for t in b]} elements, stepped {[t[0].size for t in a]}")
            continue
        bad += [f"rank {r}: exchange {j} ({x[0].size} elements) was sent with other bits than stepped"
                for j, (x, y) in enumerate(zip(a, b)) if not np.array_equal(_bits(x[0]), _bits(y[0]))]
        last = len(ch.ops) - 1
        if not np.array_equal(_bits(st.get(r, 3, "states")), _bits(ch.get(r, last, "states"))) or not np.array_equal(st.get(r, 3, "res"), ch.get(r, last, "res")):
            bad.append(f"rank {r}: the chained run returns other states / lamda than stepping")
    print(f"FIGURES slices/{kind} R={world}: {len(_all_taps(ch, 0))} exchanges compared bit for bit with the stepped run")
    assert not bad, "\n".join(bad[:30])


# ------------------------------------------------------------------------------------------------ stalled calls
@pytest.mark.parametrize("how", ["step", "chain"])
@pytest.mark.parametrize("conf", ["2.2", "3"])
def test_stalled(tmp_path_factory, conf, how):
    st = scenario(tmp_path_factory, 3, f"rejecting-{conf}/step")
    trials = [int(st.get(0, k, "res")[1]) for k in range(2)]
    assert trials[0] == C.REJECT_TRIALS[float(conf)], trials
    if how == "step":
        bad, _log = judge(st)
        assert [int(x) for x in st.get(0, 1, "stats")[1:]] == [0, 2], "both calls were finished by the LM loop, none missed"
        assert not bad, "\n".join(bad[:30])
        return
    ch = scenario(tmp_path_factory, 3, f"rejecting-{conf}/chain")
    geo = [int(v) for v in ch.get(0, 0, "geo")]
    lenA, lenB, pc = K.len_a(geo[0], geo[4]), K.len_b(geo[3]), 27 * ch.c.n + 2
    # call 0 stalls: call 1 was enqueued behind it (B, C, A: skipped on the device), then the LM loop of call 0, call 1 again, its LM loop
    want = [2 * ch.m_pad, pc, lenA, lenB, pc, lenA] + [2] * trials[0] + [lenA, lenB, pc, lenA] + [2] * trials[1] + [lenA]
    bad = []
    for r in range(3):
        a, b = _all_taps(st, r), _all_taps(ch, r)
        if [t[0].size for t in b] != want:
            bad.append(f"rank {r}: chained exchanges of {[t[0].size for t in b]} elements, the protocol prescribes {want}")
            continue
        b = b[:3] + b[6:]                                           # (without the three exchanges of the skipped call)
        bad += [f"rank {r}: exchange {j} ({x[0].size} elements) was sent with other bits than stepped"
                for j, (x, y) in enumerate(zip(a, b)) if not np.array_equal(_bits(x[0]), _bits(y[0]))]
        if not np.array_equal(_bits(st.get(r, 1, "states")), _bits(ch.get(r, 0, "states"))) or not np.array_equal(st.get(r, 1, "res"), ch.get(r, 0, "res")):
            bad.append(f"rank {r}: the chained run returns other states / lamda than stepping")
    assert [int(x) for x in ch.get(0, 0, "stats")[1:]] == [0, 2]
    print(f"FIGURES rejecting-{conf}/chain R=3: trials {trials}, {len(want)} exchanges")
    assert not bad, "\n".join(bad[:30])


# ------------------------------------------------------------------------------------------------ misses
MISS = {"forced-1": (1, "forced/step", "forced"), "forced-2": (2, "forced/step", "forced"), "forced-3": (3, "forced/step", "forced"),
        "overflow-one-rank": (3, "overflow-one-rank/step", "overflow"), "overflow-twin": (3, "overflow-twin/step", None),
        "long-bin": (5, "long-bin/step", "long"), "long-twin": (5, "long-twin/step", None), "leaving": (3, "leaving/step", "leaving")}


@pytest.mark.parametrize("name", list(MISS))
def test_miss(tmp_path_factory, name):
    world, scn, reason = MISS[name]
    sc = scenario(tmp_path_factory, world, scn)
    bad, log = judge(sc)
    assert not bad, "\n".join(bad[:30])
    base = scn.split("/")[0]
    assert log, "a carried call ran"
    for _k, what, reasons, b, rank, in_bin, over in log:
        assert (what == "miss") == (reason is not None) and reasons == ([reason] if reason else []), (name, log)
        if base in K.BAND:
            per = K.BAND[base][3]
            assert in_bin == sum(per) and 0 < rank < in_bin, f"{name}: {in_bin} keys in the median's bin, wanted rank {rank}; made for {per}"
            assert over == ([0] if base == "overflow-one-rank" else []), (name, over)
        if base == "leaving":
            assert b == 0, f"{name}: the median's bin is {b}, the case was made for bin 0"
    print(f"FIGURES {name}: predicted {reason or 'hit'}, observed {[(x[1], x[2]) for x in log]}")


# ------------------------------------------------------------------------------------------------ re-upload
@pytest.mark.parametrize("world", [2, 3])
def test_reupload(tmp_path_factory, world):
    sc = scenario(tmp_path_factory, world, "slices/reupload")
    bad, log = judge(sc)
    assert not bad, "\n".join(bad[:30])
    assert [x[0] for x in log] == [1, 4] and all(x[1] == "hit" for x in log), f"calls 1 and 4 ran on carried keys, call 3 did not: {log}"


def test_every_reason(tmp_path_factory):
    """Every reason the front can miss for was reached by a case on the GPU (``lo == ~0`` stays out: unreachable, see
    tests/test_gpu_select_paths.py)."""
    for name in MISS:
        world, scn, _reason = MISS[name]
        judge(scenario(tmp_path_factory, world, scn))
    print(f"FIGURES reasons reached: { {q: len(v) for q, v in REACHED.items() if q} }")
    missing = [q for q in K.REASONS if not REACHED.get(q)]
    assert not missing, f"no case reached a miss for {missing}"
