"""R ranks of the observation-sharded mode emulated on ONE GPU (shared by the GPU tests that drive the stage entry points)."""
import numpy as np


class EmulatedRanks:
    """R ranks of the observation-sharded mode on ONE GPU: one engine per rank holding its row slice, the three RCCL
    all-gathers replaced by device-side concatenation.  Drives the HIP stage entry points vba_sh_stage1..4 exactly as
    vinsat_amd/dist.py:ShardedBA.step does.  ``mode``: the kernel set of every rank's handle (``BAEngine``'s).
    ``after_stage``: called as ``after_stage(k, self)`` behind stage k of every rank (the buffers ``abs_l``, ``part_l``, ``trial_l`` are
    the layers' outputs)."""

    def __init__(self, n, m, ranks, xyz, uv, conf, ii, K, cumrot, time_idx, mode=-1, after_stage=None):
        import torch
        from vinsat_amd.dist import HipStageEngine, shard_bounds
        from vinsat_amd.engine import BAEngine
        self.torch, self.n, self.m, self.ranks = torch, n, m, ranks
        self.after_stage = after_stage
        b = shard_bounds(m, ranks)
        self.bounds = b
        m_pad = -(-m // ranks)
        self.m_pad = m_pad
        self.engs = []
        for r in range(ranks):
            lo, hi = int(b[r]), int(b[r + 1])
            e = BAEngine(n, hi - lo, mode=mode)
            e.upload_observations(xyz[lo:hi], uv[lo:hi], conf[lo:hi], ii[lo:hi], n)
            e.upload_window(K, cumrot, time_idx)
            self.engs.append(HipStageEngine(e))
        pc = self.engs[0].partial_count(n)
        f64 = dict(dtype=torch.float64, device="cuda")
        self.abs_l = [torch.full((2 * m_pad,), float("inf"), **f64) for _ in range(ranks)]
        self.part_l = [torch.empty(pc, **f64) for _ in range(ranks)]
        self.trial_l = [torch.empty(2, **f64) for _ in range(ranks)]

    def set_states(self, st, lam):
        for e in self.engs:
            e.set_states(st, lam)

    def _after(self, k):
        if self.after_stage is not None:
            self.after_stage(k, self)

    def call(self, it, init):
        """One BA() call on every emulated rank; returns the number of stage-3 rounds (LM trials + pivoted repeats)."""
        torch, engs = self.torch, self.engs
        for r, e in enumerate(engs):
            e.stage1(it, init, self.m, self.abs_l[r])
        self._after(1)
        abs_all = torch.cat(self.abs_l)
        for r, e in enumerate(engs):
            e.stage2(abs_all, self.part_l[r])
        self._after(2)
        part_all = torch.cat(self.part_l)
        first, rounds = True, 0
        while True:
            for r, e in enumerate(engs):
                e.stage3(part_all if first else None, self.ranks, self.trial_l[r])
            self._after(3)
            trial_all = torch.cat(self.trial_l)
            done = [e.stage4(trial_all, self.ranks) for e in engs]
            self._after(4)
            first = False
            rounds += 1
            assert all(d == done[0] for d in done)
            if done[0]:
                return rounds
            assert rounds < 12

    def results(self):
        outs = [e.get_states() for e in self.engs]
        for o in outs:      # every rank holds bit-identical normal equations, so bit-identical states and damping
            assert np.array_equal(o[0], outs[0][0]) and o[1] == outs[0][1]
        return outs[0]

    def close(self):
        for e in self.engs:
            e.close()
