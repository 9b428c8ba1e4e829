"""Exponential moving averages ("teacher" networks) of the trained networks, kept inside the optimiser's launch.

No reference counterpart: the reference trains two students and evaluates whatever the last optimiser step left.  This is an
opt-in extension (CPSConfig.ema_decay) in the mould of `ema_update` and `cutmix_ratio`: off by default, a bit-exact no-op when off.

`AveragedNetwork` owns the teacher module and the STATIC pairing, by name, of the student's tensors with the teacher's.  It launches
nothing itself: `optim.HipAdam.attach_average(avg)` makes the student's one Adam launch (vqseg_adam_ema_step_f32) update the average
and rewrite the teacher's bf16 weight images from it while it holds the new parameter values.  There is no CPU path.

Pairing rule:
  * every floating parameter and every floating buffer of the student is paired with the teacher's tensor of the same name;
  * every tensor owned by a VectorQuantizer submodule (the codebooks and, with ema_update, cluster_size / embed_avg) is a COPY record:
    not gradient-trained, and k-means rewrites it in the first training forward;
  * everything else is averaged: e' = fma(w, p' - e, e), w = float32(1 - decay);
  * floating buffers (BatchNorm running statistics) are average-only records: the launch reads them and steps nothing;
  * integer buffers (num_batches_tracked, ema_updates) are copied on the host when the teacher's state is asked for.
The first update (updates == 0) copies everything: whatever the first training forwards initialised behind autograd's back (k-means
codebooks and prototypes, `.data` writes) reaches the teacher as it is.
"""
from __future__ import annotations

from typing import Callable, Dict, List, NamedTuple

import torch
from torch import nn

from . import _wcache


class Pair(NamedTuple):
    name: str
    student: torch.Tensor
    teacher: torch.Tensor
    copy: bool             # the teacher takes the student's new bits instead of the average
    average_only: bool     # a buffer: nothing steps it, the launch reads it


def _vq_owned_prefixes(module: nn.Module) -> List[str]:
    from .vector_quantizer.vq_img import VectorQuantizer
    return [name + "." for name, m in module.named_modules() if isinstance(m, VectorQuantizer)]


class AveragedNetwork:
    def __init__(self, student: nn.Module, build: Callable[[], nn.Module], decay: float):
        """`build()` returns a fresh module of the student's class (parameters carry kernel-side attributes that a deepcopy would drag
        along); it is loaded with the student's state and `initted` flags and stays in eval mode, without gradients."""
        decay = float(decay)
        if not 0.0 <= decay < 1.0:
            raise ValueError(f"AveragedNetwork: 0 <= decay < 1 required, got {decay}")
        self.student, self.decay, self.updates = student, decay, 0
        ref = next(iter(student.parameters()), None)
        teacher = build()
        if ref is not None:
            teacher = teacher.to(ref.device)
        self.module = teacher
        teacher.requires_grad_(False)
        teacher.eval()
        self.reset_from_student()
        self.pairs: List[Pair] = self._pair()

    def _pair(self) -> List[Pair]:
        owned = _vq_owned_prefixes(self.student)
        t_params, t_bufs = dict(self.module.named_parameters()), dict(self.module.named_buffers())
        pairs = []
        for is_buf, named, theirs in ((False, self.student.named_parameters(), t_params), (True, self.student.named_buffers(), t_bufs)):
            for name, s in named:
                if not s.is_floating_point():
                    continue
                t = theirs.get(name)
                if t is None or t.shape != s.shape or t.dtype != s.dtype:
                    raise ValueError(f"AveragedNetwork: build() made a module without a matching {name!r} {tuple(s.shape)}")
                pairs.append(Pair(name, s, t, any(name.startswith(p) for p in owned), is_buf))
        return pairs

    @torch.no_grad()
    def reset_from_student(self) -> None:
        """the teacher becomes a copy of the student (construction; a checkpoint that holds no teacher); updates = 0"""
        self.module.load_state_dict(self.student.state_dict())
        mods = dict(self.module.named_modules())
        for name, m in self.student.named_modules():
            if hasattr(m, "initted"):
                mods[name].initted = bool(m.initted)
        _wcache.invalidate(self.module)
        self.updates = 0

    @torch.no_grad()
    def sync_integer_buffers(self) -> None:
        """num_batches_tracked, ema_updates: the student's, copied when the teacher's state is asked for (never on the step path)"""
        theirs = dict(self.module.named_buffers())
        for name, s in self.student.named_buffers():
            if not s.is_floating_point() and name in theirs:
                theirs[name].copy_(s)

    def state_dict(self) -> Dict[str, object]:
        self.sync_integer_buffers()
        return {"module": self.module.state_dict(), "updates": int(self.updates)}

    @torch.no_grad()
    def load_state_dict(self, state: Dict[str, object]) -> None:
        self.module.load_state_dict(state["module"])
        _wcache.invalidate(self.module)
        self.updates = int(state["updates"])
