"""Scaled data snooping on the CPU: the scratch layout of vba_snoop_scaled under the sanitizers (a stand-alone program), and the
driver loop of ``od_pipe.streaming_batched(snoop_each=...)`` with the NumPy oracle standing in for the GPU -- an injected
``ba_window`` and a stub of ``ba.snoop_scaled`` built from tests/power_oracle.py and tests/snoop_oracle.py -- against
``streaming_version(snoop=dict(scaled=True, ...))`` sequence by sequence over the same stub."""
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import power_oracle as PW
import snoop_oracle as S
from conftest import ROOT
from oracle import ba_oracle as O
from vinsat_amd import od_pipe, synth


def test_scratch_layout_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """A stand-alone program with its own main (CPU only); any ASan / UBSan finding aborts it with a non-zero code."""
    src = os.path.join(ROOT, "tests", "hostcheck", "sanitize_snoop_fit_main.cpp")
    exe = str(tmp_path / "sanitize_snoop_fit_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, src])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "sanitize_snoop_fit_main ok" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


# ------------------------------------------------------------------------------------------------ the oracle as the device
class _OracleDevice:
    """What the drivers see of ``vinsat_amd.ba``: ``BA_window`` (one window or a ragged list), ``snoop_scaled``, ``snoop`` with
    ``scaled=True`` and ``rejected``, over the CPU oracle.  Like the device it keeps the rejections of the resident rows: a
    ``BA_window`` call on other rows (another batch of the sequence) clears them."""

    def __init__(self):
        self.key, self.wins, self.masks = None, [], []
        self.ba_calls, self.snoop_calls = [], 0
        self.snoop_scaled = self._snoop_scaled
        self.snoop = self._snoop
        self.snoop_scaled.__func__.last = {}
        self.snoop.__func__.last = {}

    def BA_window(self, iters, inits, states, velocities, imu, uv, xyz, ii, time_idx, intr, conf, lam):
        ragged = isinstance(states, list)
        lists = [x if ragged else [x] for x in (states, imu, uv, xyz, ii, time_idx, intr, conf, lam)]
        key = tuple((c.data_ptr(), c.numel()) for c in lists[7])
        if key != self.key:
            self.key, self.masks = key, [np.zeros(c.numel(), dtype=bool) for c in lists[7]]
        self.wins, out = [], []
        for b, (st, im, u, x, i_, t_, k_, c_, l_) in enumerate(zip(*lists)):
            w = types.SimpleNamespace(cumrot_last=im[0, :, -1, 6:10].numpy(), landmarks_uv=u[0].numpy(), landmarks_xyz=x[0].numpy(),
                                      ii=np.asarray(i_), time_idx=np.asarray(t_), intrinsics=k_[0].numpy(), confidences=c_.numpy())
            s = st[0].numpy()
            for it, init in zip(iters, inits):
                s, l_, hess, _ = O.ba_iteration(it, s, w.cumrot_last, w.landmarks_uv, w.landmarks_xyz, w.ii, w.time_idx, w.intrinsics,
                                                self._conf(b, w), l_, initialize=init)
            w.st, w.lam, w.it = s, l_, list(iters)[-1]
            self.wins.append(w)
            out.append((torch.from_numpy(s)[None], l_, torch.from_numpy(hess)[None]))
        self.ba_calls.append((len(out), list(iters)))
        if ragged:
            return [o[0] for o in out], velocities, [o[1] for o in out], [o[2] for o in out]
        return out[0][0], velocities, out[0][1], out[0][2]

    def _conf(self, b, w):
        c = w.confidences.copy()
        c[self.masks[b]] = 0.0
        return c

    def _round(self, quantile, mode, min_rows):
        self.snoop_calls += 1
        counts, crits = [], []
        for b, w in enumerate(self.wins):
            ref, dbg = PW.at_states(w, w.st, w.lam, it=w.it, conf=self._conf(b, w))
            s0sq = ref["fit"][4]
            crit = quantile * np.sqrt(s0sq) if s0sq > 0 else np.nan
            now = np.zeros(w.ii.size, dtype=bool)
            if crit == crit:
                now, _ = S.select(ref["wtest"], dbg["w"], w.ii, w.st.shape[0], crit, mode, min_rows)
            self.masks[b] |= now
            counts.append([int(now.sum()), int(self.masks[b].sum())])
            crits.append(float(crit))
        return counts, crits

    def _snoop_scaled(self, iter=None, damped=False, quantile=3.29, mode=0, min_rows=6):
        counts, crits = self._round(quantile, mode, min_rows)
        single = len(self.wins) == 1
        self.snoop_scaled.__func__.last = dict(counts=counts[0] if single else counts, crit=crits[0] if single else crits)
        masks = [torch.from_numpy(m.copy())[None] for m in self.masks]
        return masks[0] if single else masks

    def _snoop(self, iter=None, damped=False, crit=3.29, scaled=True, mode=0, min_rows=6):
        assert scaled and len(self.wins) == 1
        counts, crits = self._round(crit, mode, min_rows)
        self.snoop.__func__.last = dict(counts=counts[0], crit=crits[0])
        return torch.from_numpy(self.masks[0].copy())[None]

    def rejected(self):
        return torch.from_numpy(self.masks[0].copy())[None]


def _patched(monkeypatch):
    from vinsat_amd import ba
    dev = _OracleDevice()
    for name in ("BA_window", "snoop_scaled", "snoop", "rejected"):
        monkeypatch.setattr(ba, name, getattr(dev, name))
    return dev


QUANTILE = 2.0      # (the synthetic sequences are clean: a low quantile so that rows are rejected at all)


def test_batched_driver_snoops_every_window_and_matches_the_sequential_driver(monkeypatch):
    """C1 (one batch), the two-pass sequence (two batches: round 1 has a single window left) and a second C1, ``until="rounds"`` in
    both drivers: identical errors, time stamps and rejected rows; the rows rejected in batch 0 of the two-pass sequence keep
    confidence 0 in its batch 1; ``snoop_log`` names round and sequence; every round is followed by its calls."""
    seqs = [synth.make_sequence("C1"), synth.make_two_pass_sequence(), synth.make_sequence("C1", seed=1)]
    cfg = dict(crit=QUANTILE, rounds=2, calls=2, min_rows=4, until="rounds")      # (the two-pass sequence has six rows per pose)
    dev = _patched(monkeypatch)
    log = []
    batched = od_pipe.streaming_batched([(d.copy(), o.copy()) for d, o in seqs], ba_window=dev.BA_window, snoop_each=cfg, snoop_log=log)
    assert [(r["round"], r["sequence"]) for r in log] == [(0, 0), (0, 1), (0, 2), (1, 1)]
    assert all(r["rows"].dtype == np.int64 for r in log) and sum(r["rows"].size for r in log) > 0
    assert [c for c in dev.ba_calls] == [(3, list(range(20))), (3, [19, 19]), (3, [19, 19]), (1, list(range(20))), (1, [19, 19]), (1, [19, 19])]
    assert dev.snoop_calls == 4
    for k, (d, o) in enumerate(seqs):
        one = _patched(monkeypatch)
        run = od_pipe.SequenceRun(d.copy(), o.copy())
        own = []
        e, fd, t = od_pipe.streaming_version(run=run, snoop=dict(cfg, scaled=True), snoop_log=own)
        assert np.array_equal(batched[k][0].numpy(), e.numpy()) and int(batched[k][1]) == int(fd)
        assert all(np.array_equal(np.atleast_1d(a), np.atleast_1d(b)) for a, b in zip(batched[k][2], t))
        mine = [r["rows"] for r in log if r["sequence"] == k]
        assert len(mine) == len(own) and all(np.array_equal(a, b) for a, b in zip(mine, own))
        if k == 1:      # the carry-over: the second batch starts from the confidences the first one's rejections zeroed
            assert mine[0].size > 0 and (run.conf.numpy()[mine[0]] == 0.0).all()


def test_until_clean_ends_at_the_first_round_that_rejects_nothing(monkeypatch):
    """``until="clean"`` with a quantile nothing exceeds: one snooping round per batch, no further call, empty logs, and the results
    of a run without ``snoop_each``; a finite quantile runs further rounds only while some window rejects."""
    seqs = [synth.make_sequence("C1"), synth.make_sequence("C1", seed=1)]
    dev = _patched(monkeypatch)
    ref = od_pipe.streaming_batched([(d.copy(), o.copy()) for d, o in seqs], ba_window=dev.BA_window)
    assert dev.snoop_calls == 0 and dev.ba_calls == [(2, list(range(20)))]
    dev = _patched(monkeypatch)
    log = []
    got = od_pipe.streaming_batched([(d.copy(), o.copy()) for d, o in seqs], ba_window=dev.BA_window, snoop_log=log,
                                    snoop_each=dict(crit=np.inf, rounds=3, calls=2))
    assert dev.snoop_calls == 1 and dev.ba_calls == [(2, list(range(20)))]
    assert [r["rows"].size for r in log] == [0, 0]
    assert all(np.array_equal(a[0].numpy(), b[0].numpy()) for a, b in zip(got, ref))
    dev = _patched(monkeypatch)
    log = []
    od_pipe.streaming_batched([(d.copy(), o.copy()) for d, o in seqs], ba_window=dev.BA_window, snoop_log=log,
                              snoop_each=dict(crit=QUANTILE, rounds=3, calls=1))
    extra = len(dev.ba_calls) - 1
    assert 1 <= extra <= 3 and dev.snoop_calls == min(extra + 1, 3)        # a round that rejected is followed by calls; a clean one ends
    assert sum(r["rows"].size for r in log) > 0


def test_arguments_are_checked():
    seqs = [synth.make_sequence("C1")]
    with pytest.raises(ValueError, match="until"):
        od_pipe.streaming_batched(seqs, ba_window=lambda *a: None, snoop_each=dict(until="never"))
    with pytest.raises(NotImplementedError, match="snoop_each"):
        od_pipe.streaming_batched(seqs, snoop=dict(crit=3.0))


def test_the_quantile_of_the_gpu_driver_comparison_is_unambiguous_on_the_oracle():
    """What tests/test_gpu_snoop_scaled.py relies on (tests/snoop_scaled_windows.py holds the values).  Measured here, quantile
    3.29, two rounds of four calls, mode 0, min_rows 6: the planted C2 sequence rejects 67 and 26 rows at crit 13.33 and 4.710
    (s0 4.050, 1.432; margins 1.7e-4, 4.1e-5), C1 rejects 2 and 0 rows at crit 2.468 and 2.412 (s0 0.7502, 0.7332; margins
    2.8e-6, 2.0e-6); no pose is ambiguous at crit (1 - 1e-6), crit or crit (1 + 1e-6) in any round."""
    import snoop_scaled_windows as SSW
    for k in range(2):
        rounds = SSW.oracle_loop(k)
        print(k, [(int(r["mask"].sum()), float("%.4g" % r["crit"]), float("%.4g" % r["s0"]), float("%.2g" % r["margin"])) for r in rounds])
        assert len(rounds) == SSW.ROUNDS and all(r["ambiguous"] == [] for r in rounds)
        assert rounds[0]["mask"].any()
