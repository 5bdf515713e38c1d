"""CPU stand-ins of the device-side clipping operations of dp.DataParallelTrainer (test infrastructure, beside dp_oracle_ops.py): numpy
plays include/lrcn_clip.h through tests/clip_ref.py, and every call is logged so that a test can check the order the trainer drives."""
import torch

import clip_ref
from dp_oracle_ops import OracleGroupOps


class ClipOracleOps(OracleGroupOps):
    def __init__(self, dims):
        super().__init__(dims)
        self.slots = torch.zeros(9, dtype=torch.float64)
        self.scale, self.skip, self.norm = 1.0, False, 0.0
        self.steps = self.clipped = self.skipped = 0

    def grad_sumsq(self, g, slot=0, stream=None, group=-1):
        from lrcn_amd import dp
        if torch.is_tensor(g):
            self.log.append(("sumsq", slot, stream, g.numel()))
            self.slots[slot] = clip_ref.sumsq(g.numpy())
            return
        self.log.append(("sumsq_model", group, stream))
        for k in (range(9) if group < 0 else dp.GRAD_GROUPS[group]):
            self.slots[k] = clip_ref.sumsq(g[k].numpy())

    def clip_slots(self, n_slots):
        return self.slots[:n_slots]   # a view: an all-reduce of it lands in the control block

    def clip_set(self, max_norm, n_slots=9, stream=None):
        self.log.append(("clip_set", n_slots, stream))
        self.norm, self.scale, self.skip = clip_ref.clip_from_slots(self.slots[:n_slots].tolist(), max_norm)
        self.steps += 1
        self.clipped += int(self.scale < 1.0)
        self.skipped += int(self.skip)

    def clip_stats(self):
        return {"last_norm": self.norm, "last_scale": float(self.scale), "last_skipped": int(self.skip), "steps": self.steps,
                "clipped": self.clipped, "skipped": self.skipped}

    def _pre(self, g):
        return torch.as_tensor(clip_ref.scaled(g.numpy(), self.scale))

    def update(self, param, grads, optim, clipped=False):
        self.log.append(("adam_all", optim.t + 1, clipped))
        if clipped and self.skip:
            optim.t += 1
            return
        super().update(param, [self._pre(g) for g in grads] if clipped else grads, optim)

    def update_flat(self, w, g, m, v, optim, stream, clipped=False):
        if clipped and self.skip:
            return
        super().update_flat(w, self._pre(g) if clipped else g, m, v, optim, stream)
