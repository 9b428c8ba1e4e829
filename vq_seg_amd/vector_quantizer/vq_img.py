"""VectorQuantizer / EuclideanCodebook with the reference's module surface, computed by
the gfx950 HIP kernels behind include/vqseg.h.

Mirrors vector_quantizer/vq_img.py of the reference: constructor keywords (:194-205), the
submodule path `.codebook.embedding.weight`, the `initted` flag, train/eval switching and
the 4-tuple returned by forward (:228-244).  The arithmetic is NOT the reference's op
sequence: distance + argmin + gather + straight-through + commitment + dead-code
histogram run as fused kernels (vq_seg_amd/csrc/vq_assign.hip, vq_filter.hip, vq_tail.hip), and backward is the
analytic gradient instead of an autograd graph over cdist.

Extension (opt-in, `ema_update=True`; default False = the reference's frozen codebook): the exponential-moving-average
codebook update BASELINE.json's north_star names.  The reference stores `decay` / `eps` and never uses them;
with the flag set they drive the published EMA rule (see include/vqseg.h, vqseg_vq_ema_update_f32) after every training
forward, with the per-code sums / counts all-reduced over RCCL when torch.distributed runs more than one rank.
`threshold_ema_dead_code` > 0 adds that rule's companion: a code whose moving count falls below the threshold takes a row of
the current batch, chosen by a hash of (revive_seed, number of updates so far, code) -- on the device, identically on every rank,
inside the same all-reduce (include/vqseg.h, vqseg_vq_revive_candidates / vqseg_vq_ema_update_revive_f32).
"""
from __future__ import annotations

import torch
from torch import nn

from .. import _hip
from .. import nnf
from .._wcache import cache_of as _cache_of, invalidate as _invalidate
from ..dist import collectives_on as _collectives_on, broadcast0 as _broadcast0, all_reduce_sum as _all_reduce_sum, rank as _rank, \
    world_size as _world_size


class _VQFunction(torch.autograd.Function):
    """rows (N, C) -> quant (N, C), idx (N,), loss (1,), dead_pct ()."""

    @staticmethod
    def forward(ctx, rows, codebook, training, commitment_weight, prepared=None):
        quant, idx, loss, dead = _hip.vq_forward(rows, codebook, training, commitment_weight, prepared=prepared)
        ctx.commitment_weight = float(commitment_weight)
        ctx.training = bool(training)
        ctx.bf16 = rows.dtype == torch.bfloat16
        if training:
            if ctx.bf16:
                ctx.save_for_backward(rows, idx, codebook)   # the code index, not the (bf16-rounded) quantised rows
            else:
                ctx.save_for_backward(rows, quant)
        ctx.mark_non_differentiable(idx, dead)
        return quant, idx, loss, dead

    @staticmethod
    def backward(ctx, g_quant, _g_idx, g_loss, _g_dead):
        if not ctx.training:
            return None, None, None, None, None             # eval: quant is a pure gather (constant in x)
        gl = g_loss.contiguous() if (g_loss is not None and ctx.commitment_weight > 0) else None
        if ctx.bf16:
            rows, idx, codebook = ctx.saved_tensors
            g_quant = torch.zeros_like(rows) if g_quant is None else g_quant.to(torch.bfloat16).contiguous()
            return _hip.vq_backward_bf16(g_quant, gl, rows, idx, codebook, ctx.commitment_weight), None, None, None, None
        rows, quant = ctx.saved_tensors
        if g_quant is None:
            g_quant = torch.zeros_like(rows)
        g_quant = g_quant.contiguous()
        gx = _hip.vq_backward(g_quant, gl, rows, quant, ctx.commitment_weight)
        return gx, None, None, None, None                   # the codebook receives no gradient (vq_img.py:236-239)


class _VQGroupFunction(torch.autograd.Function):
    """The forward of several independent VectorQuantizer layers with ONE distance + argmin launch (vqseg_vq_forward_group);
    per level exactly _VQFunction's outputs and gradient."""

    @staticmethod
    def forward(ctx, training, weights, n, fans, *tensors):
        rows, codebooks, prepared = tensors[:n], tensors[n:2 * n], tensors[2 * n:3 * n]
        ctx.fans = fans                                      # per level: (fan-in link of the feature map, its (b, h, w, c)) or None
        outs = _hip.vq_forward_group(list(rows), list(codebooks), list(prepared), training, weights)
        ctx.n, ctx.training, ctx.weights = n, bool(training), [float(w) for w in weights]
        ctx.bf16 = rows[0].dtype == torch.bfloat16
        if training:
            saved = []
            for r, cb, (q, idx, _l, _d) in zip(rows, codebooks, outs):
                saved += [r, idx, cb] if ctx.bf16 else [r, q]
            ctx.save_for_backward(*saved)
        flat, nondiff = [], []
        for q, idx, loss, dead in outs:
            nondiff += [idx, dead]
            flat += [q, idx, loss, dead]
        ctx.mark_non_differentiable(*nondiff)               # ONE call: a later call replaces the earlier one's set
        return tuple(flat)

    @staticmethod
    def backward(ctx, *grads):
        n = ctx.n
        none = (None, None, None, None) + (None,) * (3 * n)
        if not ctx.training:
            return none
        saved = ctx.saved_tensors
        gxs = []
        for i in range(n):
            g_quant, g_loss = grads[4 * i], grads[4 * i + 2]
            w = ctx.weights[i]
            gl = g_loss.contiguous() if (g_loss is not None and w > 0) else None
            if ctx.bf16:
                rows, idx, codebook = saved[3 * i:3 * i + 3]
                g_quant = torch.zeros_like(rows) if g_quant is None else g_quant.to(torch.bfloat16).contiguous()
                gxs.append(_hip.vq_backward_bf16(g_quant, gl, rows, idx, codebook, w))
            else:
                rows, quant = saved[2 * i:2 * i + 2]
                g_quant = torch.zeros_like(rows) if g_quant is None else g_quant.contiguous()
                gxs.append(_hip.vq_backward(g_quant, gl, rows, quant, w))
            fan = ctx.fans[i] if ctx.fans is not None else None
            if fan is not None and gxs[-1].dtype == fan[2] and nnf._fanin_deposit(fan[0], gxs[-1].reshape(fan[1])):
                gxs[-1] = None                               # the feature map's other consumer (the next encoder stage) adds it in its kernel
        return (None, None, None, None) + tuple(gxs) + (None,) * (2 * n)


def quantize_group(vqs, feats):
    """[vq(f) for vq, f in zip(vqs, feats)] for VectorQuantizer layers whose codebooks are ready, with their distance passes in
    one launch; None if the layers cannot be grouped (first training forward with k-means pending, the EMA extension, mixed row
    types, CPU tensors) -- the caller then runs them one by one.

    Split-3 features (nnf.S3: the no-grad eval forward in fp32 precision) are taken as they are when every level is one, no layer is
    in training mode and every shape is one the candidate filter serves: their [hi | lo] rows go straight into the launch (row type 2
    of vqseg_vq_forward_group) and each quantised feature comes back as an nnf.S3 -- no merge to fp32 in front, no split behind.
    None otherwise: the caller merges the features (S3.float()) and calls again."""
    if len(vqs) < 2 or len(vqs) > 4:
        return None
    if any(isinstance(f, nnf.S3) for f in feats):
        return _quantize_group_s3(vqs, feats)
    rows = []
    for vq, f in zip(vqs, feats):
        cb = vq.codebook
        if not torch.is_tensor(f) or not f.is_cuda or cb.ema_update or (cb.kmeans_init and vq.training and not cb.initted):
            return None
        rows.append(_rows_of(f))
    if len({r.dtype for r in rows}) != 1 or len({vq.training for vq in vqs}) != 1:
        return None
    n = len(vqs)
    weights = [float(vq.commitment_weight) for vq in vqs]
    fans = None
    if vqs[0].training and torch.is_grad_enabled():
        fans = []
        for f, r in zip(feats, rows):
            link = nnf._fanin_of(f)
            b, c, h, w = f.shape
            # rows must be a VIEW of the feature map (same dtype, channels_last): then the gradient of the rows IS the gradient of f
            fans.append((link, (b, h, w, c), f.dtype) if (link is not None and r.dtype == f.dtype and r.data_ptr() == f.data_ptr()) else None)
        if not any(fans):
            fans = None
    flat = _VQGroupFunction.apply(vqs[0].training, weights, n, fans, *rows, *[vq.codebook.embedding.weight.detach() for vq in vqs],
                                  *[vq.codebook.prepared() for vq in vqs])
    outs = []
    for i, f in enumerate(feats):
        b, c, h, w = f.shape
        quant, idx, loss, dead = flat[4 * i:4 * i + 4]
        outs.append((quant.reshape(b, h, w, c).permute(0, 3, 1, 2), idx.reshape(b, h, w), loss, dead))
    return outs


def _quantize_group_s3(vqs, feats):
    """quantize_group for split-3 features (see there); indices, loss (0) and dead-code share are those of the merged fp32 rows"""
    if not all(isinstance(f, nnf.S3) for f in feats) or torch.is_grad_enabled():
        return None
    L = _hip.lib()
    for vq, f in zip(vqs, feats):
        cb = vq.codebook
        b, c, h, w = f.shape
        if vq.training or cb.ema_update or not f.rows.is_cuda or c != cb.embedding_dim or \
                not L.vqseg_vq_filter_counter_offset(b * h * w, c, cb.num_embeddings):      # 0: not a shape of the candidate filter
            return None
    rows = [f.rows.reshape(-1, 2 * f.c) for f in feats]
    res = _hip.vq_forward_group(rows, [vq.codebook.embedding.weight.detach() for vq in vqs], [vq.codebook.prepared() for vq in vqs],
                                False, [float(vq.commitment_weight) for vq in vqs], s3=True)
    outs = []
    for f, (quant, idx, loss, dead) in zip(feats, res):
        b, c, h, w = f.shape
        outs.append((nnf.s3_from_rows(quant.reshape(b, h, w, 2 * c), c), idx.reshape(b, h, w), loss, dead))
    return outs


def _rows_of(x: torch.Tensor):
    """(B, C, H, W) -> contiguous (B*H*W, C) rows (free for channels_last input).  Under torch.autocast bf16 activations
    stay bf16 (the kernels up-cast on load: x.float() of vq_img.py:229 without the pass over memory, and the quantised
    output is bf16 -- what the autocast decoder would cast it to anyway); everything else becomes fp32."""
    b, c, h, w = x.shape
    if not (x.dtype == torch.bfloat16 and x.is_cuda and c % 8 == 0 and torch.is_autocast_enabled()):
        x = x.to(torch.float32)                             # outside autocast the layer returns fp32 like the reference
    rows = x.permute(0, 2, 3, 1)                            # vq_img.py:229,232
    if not rows.is_contiguous():
        rows = rows.contiguous()
    return rows.reshape(b * h * w, c)


def kmeans_init_means(rows: torch.Tensor, num_clusters: int) -> torch.Tensor:
    """sample_vectors (vq_img.py:10-17): pick the initial means with the device RNG."""
    n = rows.shape[0]
    if n >= num_clusters:
        pick = torch.randperm(n, device=rows.device)[:num_clusters]
    else:
        pick = torch.randint(0, n, (num_clusters,), device=rows.device)
    return rows[pick].contiguous()


def kmeans(rows: torch.Tensor, num_clusters: int, num_iters: int, init_means: torch.Tensor = None):
    """kmeans (vq_img.py:29-63) on the HIP path.  With torch.distributed initialised and more
    than one rank, every rank ends with the same means: rank 0's initial draw is broadcast
    and the per-iteration cluster sums / counts are all-reduced over RCCL."""
    means = (kmeans_init_means(rows, num_clusters) if init_means is None else init_means.clone()).contiguous()
    if not _collectives_on():
        return _hip.kmeans(rows, means, num_iters)
    _broadcast0(means)
    counts = torch.zeros(num_clusters, dtype=torch.int64, device=rows.device)
    for _ in range(num_iters):
        sums, counts = _hip.kmeans_accumulate(rows, means)
        _all_reduce_sum(sums)
        _all_reduce_sum(counts)
        _hip.kmeans_finalize(sums, counts, means)
    return means, counts


class EuclideanCodebook(nn.Module):
    def __init__(self, embedding_dim, num_embeddings, kmeans_init, kmeans_iters, decay, eps, num_codebook, ema_update=False,
                 threshold_ema_dead_code: float = 0.0, revive_seed: int = 0):
        super().__init__()
        if threshold_ema_dead_code < 0:
            raise ValueError(f"threshold_ema_dead_code must be >= 0, got {threshold_ema_dead_code}")
        if threshold_ema_dead_code > 0 and not ema_update:
            raise ValueError("threshold_ema_dead_code > 0 revives codes of the EMA update: it needs ema_update=True")
        self.kmeans_init = kmeans_init
        self.kmeans_iters = kmeans_iters
        self.initted = False
        self.num_codebook = num_codebook
        self.decay = decay                                   # unused unless ema_update -- as in the reference
        self.eps = eps
        self.ema_update = bool(ema_update)
        self.embedding = nn.Embedding(num_embeddings, embedding_dim)
        self.num_embeddings = num_embeddings
        self.embedding_dim = embedding_dim
        if not kmeans_init:
            self.embedding.weight.data.uniform_(-1 / num_embeddings, 1 / num_embeddings)   # vq_img.py:156-158
            self.initted = True
        if self.ema_update:                                  # extension state; absent from state_dict() otherwise
            self.register_buffer("cluster_size", torch.zeros(num_embeddings))
            self.register_buffer("embed_avg", self.embedding.weight.detach().clone())
        self.threshold_ema_dead_code = float(threshold_ema_dead_code)
        self.revive_seed = int(revive_seed)
        self.revived = None                                  # device int64 scalar: codes the last update revived (never read on the step path)
        if self.threshold_ema_dead_code > 0:                 # the `t` of the candidate hash; travels with the state, absent otherwise
            self.register_buffer("ema_updates", torch.zeros((), dtype=torch.int64))

    def prepared(self) -> torch.Tensor:
        """Kernel-side image of the codebook (include/vqseg.h: vqseg_vq_prepare_f32), rebuilt only when the weight may have
        changed (_wcache: version counter / storage / device, every optimiser step, explicit invalidation after `.data` writes)."""
        w = self.embedding.weight
        cache = _cache_of(w)
        if "vq_prepared" not in cache:
            cache["vq_prepared"] = _hip.vq_prepare(w.detach())
        return cache["vq_prepared"]

    @torch.no_grad()
    def _kmeans_init(self, rows: torch.Tensor):
        if self.initted:
            return
        means, bins = kmeans(rows, self.num_embeddings, self.kmeans_iters)
        self.embedding.weight.copy_(means)                   # in place on the parameter itself: bumps its version counter,
        _invalidate(self.embedding.weight)                   # which (with this) retires the prepared image of the old codebook
        if self.ema_update:
            self.embed_avg.copy_(means)
            self.cluster_size.copy_(bins.to(self.cluster_size.dtype))
        self.initted = True

    @torch.no_grad()
    def ema_step(self, rows: torch.Tensor, idx: torch.Tensor):
        """Extension: one EMA update from the rows (N, C) of this forward and their code indices."""
        if self.threshold_ema_dead_code > 0:
            return self._ema_revive_step(rows, idx)
        sums, counts = _hip.vq_code_sums(rows, idx.reshape(-1), self.num_embeddings)
        if _collectives_on():                                # every rank applies the same update to the same state
            _all_reduce_sum(sums)
            _all_reduce_sum(counts)
        _hip.vq_ema_update(self.cluster_size, self.embed_avg, self.embedding.weight.detach(), sums, counts, self.decay, self.eps)
        _invalidate(self.embedding.weight)                   # the kernel wrote the weight behind autograd's back

    def _ema_revive_step(self, rows: torch.Tensor, idx: torch.Tensor):
        """ema_step with the dead-code revival: the code sums, the candidate rows and their flags share ONE flat buffer
        [sums K*C | cand K*C | ok K], so data parallelism all-reduces one message where it all-reduced the sums."""
        k, c = self.num_embeddings, self.embedding_dim
        flat = torch.empty(2 * k * c + k, dtype=torch.float32, device=rows.device)
        sums, cand, ok = flat[:k * c].view(k, c), flat[k * c:2 * k * c].view(k, c), flat[2 * k * c:]
        _, counts = _hip.vq_code_sums(rows, idx.reshape(-1), k, out=sums)
        _hip.vq_revive_candidates(rows, self.revive_seed, self.ema_updates, k, _rank(), _world_size(), out=(cand, ok))
        if _collectives_on():
            _all_reduce_sum(flat)
            _all_reduce_sum(counts)
        if self.revived is None or self.revived.device != rows.device:
            self.revived = torch.zeros((), dtype=torch.int64, device=rows.device)
        _hip.vq_ema_update(self.cluster_size, self.embed_avg, self.embedding.weight.detach(), sums, counts, self.decay, self.eps,
                           candidates=cand, ok=ok, threshold=self.threshold_ema_dead_code, counter=self.ema_updates, revived=self.revived)
        _invalidate(self.embedding.weight)                   # the kernel wrote the weight behind autograd's back

    def forward(self, x: torch.Tensor):
        """x (B, HW, C) -> quantized (B, HW, C), embed_idx (B, HW), code_usage (dead-code %)."""
        b, hw, c = x.shape
        rows = x.float().reshape(b * hw, c).contiguous()
        if self.kmeans_init and self.training:
            self._kmeans_init(rows.detach())
        quant, idx, _loss, dead = _VQFunction.apply(rows.detach(), self.embedding.weight.detach(), False, 0.0,
                                                    self.prepared())
        return quant.reshape(b, hw, c), idx.reshape(b, hw), dead


class VectorQuantizer(nn.Module):
    def __init__(self, dim, num_embeddings, embedding_dim=None, decay=0.8, eps=1e-5, kmeans_init=False,
                 kmeans_iters=10, distance="euclidean", commitment_weight=1, num_codebook=1, ema_update=False,
                 threshold_ema_dead_code: float = 0.0, revive_seed: int = 0):
        super().__init__()
        embedding_dim = embedding_dim if embedding_dim is not None else dim
        self.num_embeddings = num_embeddings
        self.eps = eps
        self.commitment_weight = commitment_weight
        if distance != "euclidean":
            raise NotImplementedError(
                f"distance={distance!r}: only the euclidean codebook is on the accelerated path (SURVEY 2 #1; the "
                "cosine codebook is unused by the target configs)")
        self.codebook = EuclideanCodebook(embedding_dim=embedding_dim, num_embeddings=num_embeddings,
                                          kmeans_init=kmeans_init, kmeans_iters=kmeans_iters, decay=decay, eps=eps,
                                          num_codebook=num_codebook, ema_update=ema_update,
                                          threshold_ema_dead_code=threshold_ema_dead_code, revive_seed=revive_seed)

    def forward(self, x: torch.Tensor):
        """x (B, C, H, W) -> (quantize (B, C, H, W) f32 -- bf16 for bf16 input --, embed_index (B, H, W) i64, loss (1,), code_usage ())."""
        b, c, h, w = x.shape
        rows = _rows_of(x)
        cb = self.codebook
        if cb.kmeans_init and self.training and not cb.initted:
            cb._kmeans_init(rows.detach().float())                           # vq_img.py:165-166
        ema = cb.ema_update and self.training
        weight = cb.embedding.weight.detach()
        if ema:
            weight = weight.clone()                          # backward re-reads the codebook THIS forward quantised with
        quant, idx, loss, dead = _VQFunction.apply(rows, weight, self.training, float(self.commitment_weight), cb.prepared())
        if ema:
            cb.ema_step(rows.detach(), idx)
        quantize = quant.reshape(b, h, w, c).permute(0, 3, 1, 2)             # vq_img.py:242 (channels_last view)
        return quantize, idx.reshape(b, h, w), loss, dead
