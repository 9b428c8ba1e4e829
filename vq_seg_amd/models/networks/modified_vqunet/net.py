"""VQ-UNet with reliable prototype loss: `vqreptunet1x1` (v1) and `vqreptunet1x1v2` (v2).

Reference: models/networks/modified_vqunet/net.py:1141-1222 (v1, the later of two identical
definitions, q1) and :184-260 (v2).  Same constructor keywords, attributes (`encoder`, `codebook`,
`decoder`, `segmentation_head`, `prototype_loss`, `upsampling`), forward signatures and the 4-tuple
`(logits, commitment (1,), code_usage (n_vq,) on the CPU, prototype_loss | None)`.

Kept quirks: commitment is averaged over len(features)=5 although 3 levels are quantised (q2);
code_usage is the percentage of DEAD codes (q4).  Dropped: the per-level host syncs -- v1's tensor
truthiness test (:1188; a zero loss adds nothing, q3) and the three `.cpu()` calls (:1191) are
replaced by ONE device->host copy of the stacked usage vector at the end of forward.
"""
import torch
from torch import nn

from .... import nnf
from ....vector_quantizer import make_vq_module, Identity as _IdentityVQ, quantize_group as _quantize_group
from ...encoders import make_encoder
from ...modules.prototype import ReliablePrototypeLoss, ReliablePrototypeLossv2
from ..unet.decoder import UnetDecoder
from ..unet.net import _to_device_layout


class _Upsampling(nn.Module):
    """nn.UpsamplingBilinear2d(scale_factor): bilinear, align_corners=True."""

    def __init__(self, scale_factor):
        super().__init__()
        self.scale_factor = scale_factor

    def forward(self, x):
        return nnf.upsample_bilinear(x, scale_factor=self.scale_factor, align_corners=True)


class _Head1x1(nn.Conv2d):
    def forward(self, x):
        return nnf.head_conv1x1(x, self.weight)


class _VQRePTUnet1x1Base(nn.Module):
    _proto_cls = None

    def __init__(self, encoder_name: str, num_classes: int, vq_cfg: dict, margin=1.5, scale=1., use_feature=False,
                 encoder_weights=None, in_channels: int = 3, decoder_channels=None, depth: int = 5,
                 activation=nn.Identity, upsampling=2, pt_init="kmeans"):
        super().__init__()
        self.encoder = make_encoder(encoder_name, in_channels, depth, weights=encoder_weights, padding_mode="reflect")
        enc_ch = self.encoder.out_channels()
        self.codebook = make_vq_module(vq_cfg, enc_ch, depth)
        if decoder_channels is None:
            decoder_channels = [c // 2 for c in enc_ch[1:]][::-1]
        self.decoder = UnetDecoder(enc_ch, decoder_channels)
        self.segmentation_head = _Head1x1(decoder_channels[-1], num_classes, 1, bias=False)
        self.prototype_loss = self._proto_cls(num_classes, decoder_channels[-1], margin=margin, scale=scale, init=pt_init,
                                              use_feature=use_feature)
        self.device = None
        self.upsampling = _Upsampling(upsampling) if upsampling > 1 else nn.Identity()

    # -- shared trunk in three phases: encoder -> VQ on the configured levels -> decoder + 1x1 head.  forward() runs them
    # back to back; trainer.CPSTrainer drives the phases of its two networks separately so that the distance kernels of
    # the VQ phase have the GPU to themselves while everything else of the two networks overlaps on two streams.
    def encode(self, x):
        if self.device is None:
            self.device = x.device
        # a no-grad eval-mode fp32 forward (the trainers' pseudo-label passes) runs in split-3 form on the bf16 kernels (nnf.S3)
        with nnf.s3_scope(not self.training and not torch.is_grad_enabled()):
            feats = self.encoder(_to_device_layout(x))[1:]
        if len(feats) != len(self.codebook):
            raise NotImplementedError
        return feats

    def quantize(self, feats):
        loss = torch.zeros(1, device=feats[0].device)
        usage = []
        levels = [i for i, vq in enumerate(self.codebook) if not isinstance(vq, _IdentityVQ)]
        vqs = [self.codebook[i] for i in levels]
        group = nnf.py_opt("py_vq_group", 1)
        # the quantised levels are independent: their distance passes share ONE launch when they can (vq_img.quantize_group).
        # Split-3 levels go into it as they are when the group can take them (VQSEG_OPTS=py_vq_s3=0: never) and come back split-3 ...
        grouped = None
        if group and nnf.py_opt("py_vq_s3", 1) and any(isinstance(feats[i], nnf.S3) for i in levels):
            grouped = _quantize_group(vqs, [feats[i] for i in levels])
        if grouped is None:
            for i in levels:                                 # ... everything else takes fp32 rows (Identity levels pass split-3 tensors through)
                if isinstance(feats[i], nnf.S3):
                    feats[i] = feats[i].float()
            grouped = _quantize_group(vqs, [feats[i] for i in levels]) if group else None
        grouped = dict(zip(levels, grouped)) if grouped is not None else {}
        for i, vq in enumerate(self.codebook):
            quantize, _idx, commitment, dead = grouped[i] if i in grouped else vq(feats[i])
            feats[i] = quantize
            if commitment is not None:
                loss = loss + commitment
            if dead is not None:
                usage.append(dead.detach())
        return feats, loss / len(feats), usage

    def decode(self, feats, perturb=None):
        """-> decoder_out, logits; with a perturbation spec `perturb` (see _perturb_spec) -> decoder_out, logits, logits_fp: the
        feature-perturbation stream of UniMatch (deprecated/train_UNIMatch.py:172,183-185; models/networks/deeplabv3/net.py:109-116:
        decoder(torch.cat((f, nn.Dropout2d(0.5)(f))))).  Every decoder input -- all five levels, after quantisation, in the dtype it has
        here -- is doubled to 2B images by nnf.channel_dropout_cat with its own slice of ONE keep table (nnf.channel_keep: one launch),
        so the encoder and the VQ phase ran on B images and only the decoder and the head run on 2B (their BatchNorm statistics are
        taken over the 2B batch, as in the reference).  The clean halves are what is returned first; the table is left under
        perturb["scale"]."""
        if perturb is None:
            decoder_out = self.decoder(*feats)
            if self.training:                                # two consumers in training mode: the head and the prototype loss
                nnf.fanin_tag(decoder_out)
            return decoder_out, self.segmentation_head(decoder_out)
        self._training_only(perturb)
        b = feats[0].shape[0]
        table, scales = nnf.channel_keep([(b, f.shape[1]) for f in feats], perturb["p"], perturb["seed"], perturb["stream"], perturb["step"],
                                         feats[0].device)
        perturb["scale"] = table
        # the encoder features gain no consumer (the one op stands where the decoder stood); its gradient goes back through autograd,
        # and so do the two gradients of decoder_out (the head sees 2B images, the prototype loss the clean half): the unfused adds
        decoder_out = self.decoder(*[nnf.channel_dropout_cat(f, s) for f, s in zip(feats, scales)])
        logits = self.segmentation_head(decoder_out)
        return decoder_out[:b], logits[:b], logits[b:]

    def _training_only(self, need_fp):
        if need_fp and not self.training:
            raise RuntimeError("feature perturbation (need_fp / a perturbation spec) is a training-mode option: this model is in eval "
                               "mode -- call train() first, or leave need_fp off")

    def _perturb_spec(self, need_fp, side):
        """The perturbation spec of this forward, or None: a dict with the drop probability "p" and the draw's key "seed", "stream",
        "step" (nnf.channel_keep: the table is a pure function of them).  `need_fp`: False, a spec, or True for p = 0.5 under seed 0,
        stream 0 and this module's count of such forwards as the step; `side`: a caller-owned dict may carry one under "perturb"
        (trainer.CPSTrainer: per network and iteration).  The dict is the caller's: the table is left in it under "scale"."""
        self._training_only(need_fp)
        if need_fp is True:
            step = self.__dict__.get("_fp_forwards", 0)
            self.__dict__["_fp_forwards"] = step + 1
            return dict(p=0.5, seed=0, stream=0, step=step)
        if need_fp:
            return need_fp
        return side.get("perturb") if side is not None else None

    def _side_terms(self, decoder_out, gt, side):
        """`side`: a dict the CALLER of finish() supplies and owns (trainer.CPSTrainer; nothing is kept on the module).  In training mode
        the callable under "sup_con" (loss.SupConLoss) is evaluated on this forward's decoder output and targets -- here, on this network's
        stream and under its autocast -- and its scalar left under "sup_con_loss"; with "keep", the decoder output under "decoder_out"."""
        if side is None or not self.training:
            return
        if side.get("sup_con") is not None:
            side["sup_con_loss"] = side["sup_con"](decoder_out, gt)
        if side.get("keep"):
            side["decoder_out"] = decoder_out.detach()

    def _trunk(self, x):
        feats, loss, usage = self.quantize(self.encode(x))
        decoder_out, logits = self.decode(feats)
        return decoder_out, logits, loss, usage

    # `async_code_usage = True` (set by trainer.CPSTrainer): the code-usage vector is copied to PINNED host memory without
    # blocking the host -- the returned CPU tensor is valid once the stream has been synchronised.  The default keeps the
    # reference's semantics (a CPU tensor that is valid on return), at the price of one host-device sync per forward, which
    # stalls the host's kernel queue (and keeps the two networks of a CPS pair from overlapping).
    async_code_usage = False

    def _usage_to_host(self, usage, like):
        if not usage:
            return torch.tensor([])
        stacked = torch.stack(usage)
        if not (self.async_code_usage and stacked.is_cuda):
            return stacked.cpu()                                      # the one device->host copy of forward
        ring = self.__dict__.setdefault("_usage_ring", [])            # a few pinned buffers, reused round-robin
        if len(ring) < 8:
            ring.append(torch.empty(stacked.shape, dtype=stacked.dtype, pin_memory=True))
        buf = ring[self.__dict__.setdefault("_usage_i", 0) % len(ring)]
        self.__dict__["_usage_i"] += 1
        buf.copy_(stacked, non_blocking=True)
        return buf

    @torch.no_grad()
    def pseudo_label(self, x):
        _, logits, _, _ = self._trunk(x)
        return torch.argmax(logits, dim=1).long()


class VQRePTUnet1x1(_VQRePTUnet1x1Base):
    _proto_cls = ReliablePrototypeLoss

    def forward(self, x, gt=None, code_usage_loss=False, percent=None, need_fp=False):
        """`need_fp` (training mode only): True or a perturbation spec appends `output_fp`, the prediction of the feature-perturbation
        stream (decode), to the usual tuple; False leaves tuple and computation as they are"""
        self._training_only(need_fp)
        return self.finish(*self.quantize(self.encode(x)), gt=gt, code_usage_loss=code_usage_loss, percent=percent, need_fp=need_fp)

    def finish(self, feats, loss, usage, gt=None, code_usage_loss=False, percent=None, side=None, need_fp=False):
        spec = self._perturb_spec(need_fp, side)
        decoder_out, output, *fp = self.decode(feats, spec)
        self._side_terms(decoder_out, gt, side)
        prototype_loss = None
        if self.training:
            with torch.no_grad():
                if nnf.softmax_stats_supported(output):
                    entropy = nnf.softmax_stats(output, want_label=False)[1].reshape(-1)     # (b, h, w) order, one HIP pass
                else:
                    prob = torch.softmax(output.float().permute(0, 2, 3, 1).reshape(-1, output.shape[1]), dim=1)
                    entropy = -torch.sum(prob * torch.log(prob + 1e-10), dim=1)
            prototype_loss = self.prototype_loss(decoder_out, gt, percent=percent, entropy=entropy)
        output = self.upsampling(output)
        fp = tuple(self.upsampling(o) for o in fp)              # (output_fp,) with a perturbation spec, else empty
        if code_usage_loss:
            return (output, loss, self._usage_to_host(usage, output), torch.stack(usage).sum()[None] / len(self.codebook)) + fp
        return (output, loss, self._usage_to_host(usage, output), prototype_loss) + fp


class VQRePTUnet1x1v2(_VQRePTUnet1x1Base):
    _proto_cls = ReliablePrototypeLossv2

    def forward(self, x, gt=None, code_usage_loss=False, th=None, need_fp=False):
        """`need_fp`: as VQRePTUnet1x1.forward"""
        self._training_only(need_fp)
        return self.finish(*self.quantize(self.encode(x)), gt=gt, code_usage_loss=code_usage_loss, th=th, need_fp=need_fp)

    def finish(self, feats, loss, usage, gt=None, code_usage_loss=False, th=None, side=None, need_fp=False):
        spec = self._perturb_spec(need_fp, side)
        decoder_out, output, *fp = self.decode(feats, spec)
        self._side_terms(decoder_out, gt, side)
        prototype_loss = self.prototype_loss(decoder_out, gt, th) if self.training else None
        output = self.upsampling(output)
        fp = tuple(self.upsampling(o) for o in fp)              # (output_fp,) with a perturbation spec, else empty
        if code_usage_loss:
            return (output, loss, self._usage_to_host(usage, output), torch.stack(usage).sum()[None] / len(self.codebook)) + fp
        return (output, loss, self._usage_to_host(usage, output), prototype_loss) + fp
