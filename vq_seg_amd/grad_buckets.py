"""Data-parallel plumbing of the trainer: the gradient all-reduce over flat fp32 buckets, launched from post-accumulate hooks
while backward runs, and the one-broadcast-per-dtype copy of rank 0's module state (no reference counterpart: SURVEY 2, 8e)."""
from __future__ import annotations

from typing import Dict, List

import torch
import torch.distributed as dist
from torch import nn

from . import dist as vdist
from .utils.ckpoints import flat_copy, scatter_flat


class GradBuckets:
    """Owns the .grad storage of `params` as views into a few flat buffers ("buckets", filled in
    reverse parameter order = the order backward produces them).  With world_size > 1 each bucket is
    all-reduced (sum, then scaled by 1/world) as soon as all its gradients have been accumulated."""

    def __init__(self, params: List[nn.Parameter], bucket_mb: float = 64.0):
        self.params = [p for p in params if p.requires_grad]
        self.world = vdist.world_size()
        self.on = vdist.collectives_on()                   # world > 1, or the single-rank RCCL drive (VQSEG_DIST_SINGLE)
        cap = int(bucket_mb * (1 << 20) / 4)
        self.buckets: List[torch.Tensor] = []
        self.owner: Dict[int, int] = {}
        groups, cur, cur_n = [], [], 0
        for p in reversed(self.params):
            if cur and cur_n + p.numel() > cap:
                groups.append(cur)
                cur, cur_n = [], 0
            cur.append(p)
            cur_n += p.numel()
        if cur:
            groups.append(cur)
        for bi, g in enumerate(groups):
            flat = torch.zeros(sum(p.numel() for p in g), dtype=torch.float32, device=g[0].device)
            off = 0
            for p in g:
                p.grad = flat[off:off + p.numel()].view_as(p)
                off += p.numel()
                self.owner[id(p)] = bi
            self.buckets.append(flat)
        self._sizes = [len(g) for g in groups]
        self._pending = list(self._sizes)
        self._launched = [False] * len(groups)
        self._handles = []
        self._reported = set()
        # parameters that never report a gradient (the frozen codebooks -- vq_img.py:236-239 -- and, in the v1 model, the prototypes
        # that enter through `.data`, prototype.py:556) would keep their buckets from ever completing inside backward: they are
        # learnt on the first step (whoever has not reported by finish()) and left out of the count from then on
        self._silent = None
        self._names = {}
        self.launched_in_backward = []                     # per step: which buckets were reduced from inside backward (tests)
        self.launch_sequence: List[int] = []               # the order this step's bucket all-reduces were issued in (must be the same on
                                                           # every rank: bench.py / tests compare it across ranks)
        # RCCL has an averaging reduction; gloo (CPU tests, rehearsal) does not: sum, then scale
        self._avg = dist.ReduceOp.AVG if (self.on and dist.get_backend() == "nccl") else None
        self.producer_streams = []          # set by CPSTrainer: the side stream(s) the gradient kernels of these params run on
        for p in self.params:
            # the HIP weight-gradient kernels add straight into the bucket views (nnf grad sinks) and report here;
            # parameters whose gradient still comes from autograd (VQ-free torch ops) report through the hook
            p._vq_grad_sink = self._on_grad if self.on else None
            if self.on:
                p.register_post_accumulate_grad_hook(self._on_grad)

    def zero(self):
        for b in self.buckets:
            b.zero_()
        for p in self.params:
            p._vq_uses = 0
        self._pending = list(self._sizes)
        if self._silent:
            for pid in self._silent:
                self._pending[self.owner[pid]] -= 1
        self._launched = [False] * len(self.buckets)
        self._handles = []
        self._reported = set()
        self.launch_sequence = []

    def _launch(self, bi):
        self._launched[bi] = True
        self.launch_sequence.append(bi)
        # The collective orders itself after the CURRENT stream only.  The last gradient of a bucket may report from an
        # autograd hook running on another stream than the one the HIP weight-gradient kernels wrote the rest of the bucket
        # on, so order the current stream after everything those streams hold so far (all of this bucket's gradients).
        if self.producer_streams and self.buckets[bi].is_cuda:
            cur = torch.cuda.current_stream(self.buckets[bi].device)
            for s in self.producer_streams:
                if s != cur:
                    cur.wait_stream(s)
        self._handles.append(dist.all_reduce(self.buckets[bi], op=self._avg or dist.ReduceOp.SUM, async_op=True))

    def _on_grad(self, p):
        # A sunk parameter reports through its sink (last contribution) AND, later, through the post-accumulate hook
        # (autograd runs AccumulateGrad for it with an undefined gradient): count every parameter once per step.
        if id(p) in self._reported:
            return
        self._reported.add(id(p))
        bi = self.owner[id(p)]
        if self._silent and id(p) in self._silent:
            if self._launched[bi]:
                raise RuntimeError("a parameter classified as gradient-free on the first step produced a gradient after its bucket had "
                                   "been reduced; call GradBuckets.relearn() when the set of trained parameters changes")
            self._silent.discard(id(p))                    # it does report after all: count it again from the next step on
            return
        self._pending[bi] -= 1
        if self._pending[bi] == 0 and not self._launched[bi]:
            self._launch(bi)

    def finish(self):
        """Call after backward: reduce what is left (parameters without a gradient this step keep
        their bucket from completing), wait, average."""
        if not self.on:
            return
        self.launched_in_backward = list(self._launched)
        if self._silent is None:
            self._silent = {id(p) for p in self.params if id(p) not in self._reported}
        for bi in range(len(self.buckets)):
            if not self._launched[bi]:
                self._launch(bi)
        for h in self._handles:
            h.wait()
        if self._avg is None:                              # gloo: no averaging reduction
            for b in self.buckets:
                b.mul_(1.0 / self.world)

    def relearn(self):
        """forget which parameters are gradient-free (after freezing / unfreezing parts of the model)"""
        self._silent = None


def broadcast_module_state(m: nn.Module, src: int = 0) -> None:
    """rank `src`'s parameters and buffers to every rank: ONE broadcast per dtype over a flat copy (r3 issued ~750 per-tensor
    broadcasts per network)."""
    by_dtype: Dict[torch.dtype, List[torch.Tensor]] = {}
    for t in list(m.parameters()) + list(m.buffers()):
        by_dtype.setdefault(t.dtype, []).append(t.data)
    for ts in by_dtype.values():
        flat = flat_copy(ts)
        dist.broadcast(flat, src=src)
        scatter_flat(flat, ts)
