"""Cross-pseudo-supervision (CPS) training of two VQ-UNets: the caller of the hot path.

Mirrors the loop bodies of the reference's trainers
  v2: train_vqreptunet1x1v2.py:137-211  (score-mask CPS, CE + Dice, confidence threshold)
  v1: deprecated/train_with_test_pt_pseudo_entropy_reg.py:141-203 (entropy-percentile pseudo labels,
      criterion from cfg, `percent` schedule)
as one `CPSTrainer.step()`; data-parallel across the GPUs of a node with a bucketed gradient
all-reduce over RCCL that overlaps the backward pass (no reference counterpart: SURVEY 2, 8e).
wandb / image dumps of the reference trainer are out of scope.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Union

import torch
import torch.distributed as dist
from torch import nn

from . import dist as vdist
from .data import augmentations
from .data.synthetic import SyntheticCropWeed  # noqa: F401  (its home; imported from here by the benchmark, tools and tests)
from .grad_buckets import GradBuckets, broadcast_module_state
from .lanes import OFF, Lanes
from .loss import compute_class_weight, cross_entropy, make_loss
from .loss.dice_loss import DiceLoss, ce_dice_loss, dice_loss
from .loss.focal_loss import FocalLoss
from .loss.contrastive_loss import SupConLoss
from .loss.conf_ce_loss import conf_ce_loss, unreliable_weight
from .measurement import confusion_matrix_device, miou_device
from . import nnf
from .averaging import AveragedNetwork
from .evaluate import test_loop
from .utils.visualize import default_palette
from .utils import regions, saliency, superpixel
from .models import init_weight
from .models.networks import make_model
from .optim import HipAdam
from .predict import Prediction, Predictor
from .utils.ckpoints import gather_rank_buffers, load_training_state, restore_initted, restore_rank_buffers, save_ckpoints
from .utils.lr_schedulers import CosineAnnealingLR


@dataclass
class CPSConfig:
    model: dict
    recipe: str = "v1"                       # "v1": entropy-percentile CPS; "v2": score-mask CPS
    num_classes: int = 3
    learning_rate: float = 1e-4
    min_lr: float = 1e-7
    total_iters: int = 1000
    warmup_steps: int = 0
    cps_loss_weight: float = 1.0
    total_commitment_loss_weight: float = 1.0
    total_prototype_loss_weight: float = 0.01
    unsup_loss_drop_percent: float = 20.0
    confidence_threshold: float = 0.7
    criterion: str = "dice_loss"
    init_weights: bool = True
    bn_eps: float = 1e-5
    bn_momentum: float = 0.1
    amp_dtype: Optional[torch.dtype] = None   # torch.bfloat16 = the ROCm-native counterpart of the reference's fp16 AMP
    eval_amp: bool = False                    # False = the reference: the two no-grad pseudo-label forwards run OUTSIDE autocast, in
                                              # fp32 (train_vqreptunet1x1v2.py:143-149; deprecated/train_with_test_pt_pseudo_entropy_
                                              # reg.py:150-156); True = an all-bf16 step (a build-side speed mode, NOT the reference's)
    keep_aux: bool = False                    # keep the step's pseudo-label masks / scores in `CPSTrainer.aux` (parity tests)
    bucket_mb: float = 64.0
    two_streams: bool = True                  # each network of the pair on its own HIP stream (see CPSTrainer.__init__)
    wgrad_side_stream: bool = False           # opt-in: weight-gradient kernels on a side stream per network (nnf.WGRAD_SIDE_STREAMS); measured +-0 (r3)
    seed: int = 42
    cutmix_ratio: Optional[float] = None      # CutMix (data/augmentations.py of the reference; deprecated/train_vqpt_easyhard_aug.py:90,119-123): the
                                              # unlabelled TRAINING forwards see box-mixed images, the pseudo targets are mixed with the same boxes
                                              # (area ratio of the box); None = the plain step, the mixing code is not entered
    cutmix_boxes: str = "batch"               # "batch": one box per step for all samples (CutMix.__call__); "sample": one per sample (augmentation())
    focal_alpha: float = 0.25                 # criterion "focal_loss": FocalLoss(num_classes, alpha, gamma, ignore_index=255), the module form
    focal_gamma: float = 2.0                  # (deprecated/train_vq_pt_unet_withtest.py:81,281-282)
    class_weight: Optional[Union[str, Sequence[float]]] = None
                                              # recipe v1 only.  "balanced": compute_class_weight(num_classes, l_target) once per step, handed to both
                                              # supervised and both CPS terms (deprecated/train_vq_pt_unet_balncedweightedloss.py:135-141); made and kept on
                                              # the device, per rank under data parallelism; nothing of it is checkpointed.  A sequence: fixed weights
                                              # (train_vq_pt_unet_withtest.py:283).  None = today's step
    ema_decay: Optional[float] = None         # exponential moving average ("teacher") of each network, kept inside its Adam launch
                                              # (averaging.AveragedNetwork, optim.HipAdam.attach_average; no reference counterpart): e' = e + (1 - decay)(p' - e)
                                              # after every step, the first update a copy.  None = no teacher, nothing of it is entered
    teacher_pseudo_labels: bool = False       # the two no-grad eval forwards that open the step run the teachers instead of the students
    easy_aug: Optional[str] = None            # "similarity": the easy augmentation of deprecated/train_vqpt_easyhard_aug.py:118-123 -- the two no-grad
                                              # pseudo-label forwards see a flipped / rotated unlabelled batch (data.augmentations.similarity_transform, one
                                              # affine-warp launch), and each score map is warped back into the clean frame before anything derives a pseudo
                                              # label from it (corners a rotation leaves uncovered: all-zero logits).  None = the plain step, nothing is entered
    easy_aug_per: str = "batch"               # "batch": one transform per step for all samples (the reference); "sample": one per image
    easy_aug_max_angle: float = 90.0          # rotation angles are drawn of [0, max) degrees (the reference: 90)
    easy_aug_codes: Sequence[int] = tuple(range(10))      # the transform codes drawn from (0 / 9 identity, 1 / 2 flips, 3-8 rotations without / with a flip)
    sup_con_loss_weight: Optional[float] = None   # pixel-pair supervised contrastive term (deprecated/train_supcon_unet.py:116-153, config/sup_con_loss.json: 0.5):
                                              # each network's LABELLED training forward evaluates loss.SupConLoss on its decoder output and l_target, on its
                                              # own stream, and weight * (l_1 + l_2) joins the total (reported as `sup_con_loss`).  Needs more than 2 labelled
                                              # images.  None = today's step: nothing of it is entered, launches and tensors are the same
    sup_con_temperature: float = 0.04         # SupConLoss(temperature)
    unsup_criterion: Optional[str] = None     # recipe v1 only.  "conf_ce": the confidence-weighted soft CPS term of deprecated/train_vq_pt_unet_conf_ce.py:
                                              # 222-229 -- network k's CPS term becomes crit(labelled predictions, the other's mask) + uw * conf_ce_loss(its
                                              # unlabelled logits <- the other's unlabelled LOGITS), both directions from one nnf.conf_ce_pair call on the
                                              # caller's stream (the gradient crosses networks).  None = today's step: nothing of it is entered
    conf_ce_threshold: float = 0.6            # conf_ce_loss(threshold, threshold_neg, temperature_value): the reference's call uses its defaults
    conf_ce_threshold_neg: float = 0.0
    conf_ce_temperature: float = 1.0
    conf_ce_unreliable_weight: bool = True    # uw = loss.unreliable_weight(the target-side logits, 100 - unsup_loss_drop_percent * (1 - epoch_frac)); False: 1
    conf_ce_detach_targets: bool = False      # True: no gradient to the network that made the targets (not the reference's)
    superpixel_mean: Optional[int] = None     # the component count (the reference's: 1600).  deprecated/train_slic.py:44-69,152-160: each network's fp32
                                              # TRAINING logits are averaged over SLIC superpixels of the images they were computed from (utils.superpixel)
                                              # before the losses and the pseudo labels are taken -- both criteria, the masks handed to the other network,
                                              # the metrics and conf-CE see pooled logits.  One label map per batch and step, made on the device on the
                                              # caller's stream (the unlabelled one after CutMix) and shared by both networks; the two no-grad pseudo-label
                                              # forwards are not pooled.  None = today's step: nothing of it is entered
    superpixel_compactness: float = 10.0      # slic(compactness, iters): the reference's fast_slic call uses compactness 10 and its default 10 iterations
    superpixel_iters: int = 10
    salient_mask: Optional[float] = None      # the threshold (the reference's: 0.1).  deprecated/train_salient.py:29-34,122-126: where the RBD saliency map
                                              # (utils.saliency) of the image is <= the threshold, each network's fp32 TRAINING scores of every class >= 1
                                              # are multiplied by 0 (after the superpixel pooling, when that is on) -- the losses, the masks handed to the
                                              # other network, the metrics and conf-CE see masked scores.  One map per batch and step, made on the device on
                                              # the caller's stream from the images the training forwards receive (the unlabelled ones after CutMix); the
                                              # reference can only read the map of the un-augmented file from disk.  The two no-grad pseudo-label forwards
                                              # are not masked.  None = today's step: nothing of it is entered
    salient_segments: int = 250               # saliency_rbd(n_segments): the reference's get_saliency_rbd default; SLIC with superpixel_compactness / _iters.
                                              # Equal to superpixel_mean: one SLIC run per batch serves both options
    hard_aug: Optional[str] = None            # "photometric": the colour half of the strong view (data.augmentations.photometric; no reference counterpart,
                                              # its hard augmentation stops at CutMix) -- the CLEAN unlabelled batch is colour-jittered, grayscaled and blurred
                                              # once per step on the caller's stream (a mean pass + one launch of the photometric kernel), and the two
                                              # unlabelled TRAINING forwards see it; CutMix, when on, mixes the distorted images.  Score maps are not touched
                                              # (no pixel moves), nor are the pseudo-label forwards or the labelled batch.  None = today's step, nothing entered
    hard_aug_per: str = "sample"              # "sample": one parameter row per image; "batch": one for the step
    hard_aug_jitter: Sequence[float] = (0.5, 0.5, 0.5, 0.25)   # (B, C, S, Hh): brightness / contrast / saturation factors of 1 +- X, hue shift of +- Hh turns
    hard_aug_jitter_p: float = 0.8            # the probabilities of the jitter, the grayscale and the blur (the usual FixMatch / UniMatch strong view)
    hard_aug_gray_p: float = 0.2
    hard_aug_blur_p: float = 0.5
    hard_aug_sigma: Sequence[float] = (0.1, 2.0)              # blur sigma drawn of [lo, hi]; radius ceil(3 sigma) <= 8
    pseudo_min_area: Optional[int] = None     # speckle removal in the pseudo labels (utils.regions; no reference counterpart): in the mask each network hands
                                              # to the other, a connected region of one class (255 belongs to no region) with fewer than this many pixels
                                              # becomes 255, on that network's stream -- both recipes.  Per rank; no collective.  None = today's step: no
                                              # launch is added and no tensor made
    pseudo_connectivity: int = 4              # 4 or 8: which neighbours connect a region
    feature_perturb: Optional[float] = None   # the drop probability (the reference's: 0.5).  UniMatch's feature-perturbation stream (deprecated/
                                              # train_UNIMatch.py:172,183-185; models/networks/deeplabv3/net.py:109-116), per network of the CPS pair: in the
                                              # UNLABELLED training forward every decoder input passes the decoder and the head a second time under channel
                                              # dropout (one 2B-image decoder pass, nnf.channel_dropout_cat), and that prediction is supervised by the OTHER
                                              # network's mask: cps_k += feature_perturb_weight * crit(pred_fp_k, mask_other[unlabelled]).  The keep table of
                                              # network k (0, 1) in iteration i is nnf.channel_keep(seed=cfg.seed, stream=2 * rank + k, step=i): a pure
                                              # function of (seed, rank, network, iteration, level, sample, channel), drawn on the device in one launch -- no
                                              # host generator, no host-to-device copy, nothing to checkpoint.  The labelled pair and the pseudo-label pair
                                              # are untouched.  None = today's step: nothing of it is entered, launches and tensors are the same
    feature_perturb_weight: float = 0.5       # the reference's weight of the perturbed stream's term
    extra: dict = field(default_factory=dict)

    def __post_init__(self):
        if self.feature_perturb is not None:
            try:
                nnf.channel_keep_params(self.feature_perturb)
            except ValueError:
                raise ValueError(f"feature_perturb must be None or a drop probability in [0, 1), got {self.feature_perturb!r}") from None
            self.feature_perturb = float(self.feature_perturb)
            if self.unsup_criterion == "conf_ce":
                raise ValueError("feature_perturb does not combine with unsup_criterion='conf_ce': that option composes the unlabelled half of "
                                 "the CPS term differently (soft targets across the networks), and the combination is not tested")
        if isinstance(self.feature_perturb_weight, bool) or not float(self.feature_perturb_weight) >= 0.0 \
                or float(self.feature_perturb_weight) == float("inf"):
            raise ValueError(f"feature_perturb_weight must be a finite number >= 0, got {self.feature_perturb_weight!r}")
        if self.pseudo_min_area is not None:
            self.pseudo_min_area = nnf.region_min_area(self.pseudo_min_area, "pseudo_min_area")
        self.pseudo_connectivity = nnf.region_settings(self.pseudo_connectivity, (), "pseudo_connectivity")[0]
        if self.hard_aug not in (None, "photometric"):
            raise ValueError(f"hard_aug must be None or 'photometric', got {self.hard_aug!r}")
        if self.hard_aug_per not in ("batch", "sample"):
            raise ValueError(f"hard_aug_per must be 'batch' or 'sample', got {self.hard_aug_per!r}")
        augmentations.check_photometric_ranges(self.hard_aug_jitter, self.hard_aug_jitter_p, self.hard_aug_gray_p, self.hard_aug_blur_p,
                                               self.hard_aug_sigma)
        self.hard_aug_jitter = tuple(float(v) for v in self.hard_aug_jitter)
        self.hard_aug_sigma = tuple(float(v) for v in self.hard_aug_sigma)
        if self.ema_decay is not None and not 0.0 <= float(self.ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be None or lie in [0, 1), got {self.ema_decay!r}")
        if self.teacher_pseudo_labels and self.ema_decay is None:
            raise ValueError("teacher_pseudo_labels needs a teacher: set ema_decay")
        if self.easy_aug not in (None, "similarity"):
            raise ValueError(f"easy_aug must be None or 'similarity', got {self.easy_aug!r}")
        if self.easy_aug_per not in ("batch", "sample"):
            raise ValueError(f"easy_aug_per must be 'batch' or 'sample', got {self.easy_aug_per!r}")
        self.easy_aug_codes = tuple(int(c) for c in self.easy_aug_codes)
        if not self.easy_aug_codes or min(self.easy_aug_codes) < 0 or max(self.easy_aug_codes) > 9:
            raise ValueError(f"easy_aug_codes must be a non-empty selection of 0..9, got {self.easy_aug_codes!r}")
        if not 0.0 <= float(self.easy_aug_max_angle) <= 180.0:
            raise ValueError(f"easy_aug_max_angle must lie in [0, 180], got {self.easy_aug_max_angle!r}")
        if self.sup_con_loss_weight is not None and not float(self.sup_con_temperature) > 0.0:
            raise ValueError(f"sup_con_temperature must be positive, got {self.sup_con_temperature!r}")
        if self.unsup_criterion not in (None, "conf_ce"):
            raise ValueError(f"unsup_criterion must be None or 'conf_ce', got {self.unsup_criterion!r}")
        if self.unsup_criterion is not None:
            if self.recipe != "v1":
                raise ValueError("unsup_criterion applies to recipe 'v1': the reference's conf_ce trainer is a single-criterion one")
            if not float(self.conf_ce_temperature) > 0.0:
                raise ValueError(f"conf_ce_temperature must be positive, got {self.conf_ce_temperature!r}")
            if not float(self.conf_ce_threshold_neg) >= 0.0:
                raise ValueError(f"conf_ce_threshold_neg must be >= 0, got {self.conf_ce_threshold_neg!r}")
        if self.superpixel_mean is not None and (isinstance(self.superpixel_mean, bool) or int(self.superpixel_mean) != self.superpixel_mean
                                                 or int(self.superpixel_mean) < 1):
            raise ValueError(f"superpixel_mean must be None or a positive component count, got {self.superpixel_mean!r}")
        if not 0.0 <= float(self.superpixel_compactness) <= 1e9:
            raise ValueError(f"superpixel_compactness must lie in [0, 1e9], got {self.superpixel_compactness!r}")
        if isinstance(self.superpixel_iters, bool) or int(self.superpixel_iters) != self.superpixel_iters or int(self.superpixel_iters) < 0:
            raise ValueError(f"superpixel_iters must be an integer >= 0, got {self.superpixel_iters!r}")
        if self.salient_mask is not None and (isinstance(self.salient_mask, bool) or not 0.0 <= float(self.salient_mask) < 1.0):
            raise ValueError(f"salient_mask must be None or a threshold in [0, 1), got {self.salient_mask!r}")
        if (isinstance(self.salient_segments, bool) or int(self.salient_segments) != self.salient_segments
                or not 1 <= int(self.salient_segments) <= nnf.RBD_MAX_SEGMENTS):
            raise ValueError(f"salient_segments must be an integer in 1..{nnf.RBD_MAX_SEGMENTS}, got {self.salient_segments!r}")
        if self.recipe != "v1" and (self.criterion != "dice_loss" or self.class_weight is not None):
            raise ValueError("criterion / class_weight apply to recipe 'v1', the single-criterion recipe; the reference has no weighted or "
                             "focal form of recipe 'v2' (CE + Dice)")
        if isinstance(self.class_weight, str):
            if self.class_weight != "balanced":
                raise ValueError(f"class_weight must be None, 'balanced' or {self.num_classes} numbers, got {self.class_weight!r}")
        elif self.class_weight is not None and len(self.class_weight) != self.num_classes:
            raise ValueError(f"class_weight: one weight per class required ({self.num_classes}), got {len(self.class_weight)}")


def regularized_pseudo_label(raw: torch.Tensor, percent: float) -> torch.Tensor:
    """make_regularized_pseudo_label (deprecated/train_with_test_pt_pseudo_entropy_reg.py:30-39) with
    the percentile taken on the device (np.percentile's linear interpolation between two order statistics)."""
    if nnf.softmax_stats_supported(raw):
        label, entropy, _ = nnf.softmax_stats(raw)          # one HIP pass (vqseg_softmax_stats_f)
    else:
        prob = torch.softmax(raw.float(), dim=1)
        label = torch.argmax(prob, dim=1)
        entropy = -torch.sum(prob * torch.log(prob + 1e-10), dim=1)
    if entropy.is_cuda:
        thresh = nnf.percentile(entropy, percent)         # exact radix select (vqseg_order_stats_f), no sort, no size limit
    else:
        thresh = torch.quantile(entropy.detach().flatten(), percent / 100.0)
    return label.masked_fill_(entropy >= thresh, 255)         # (`label` is this function's own tensor: in place, one pass less than where + full_like)


def _argmax_classes(score: torch.Tensor) -> torch.Tensor:
    """torch.argmax(score, dim=1) (first maximum) -- on the device through the pseudo-label statistics kernel (one pass at memory speed;
    ATen's strided reduction over the class dimension takes ~200 us for 32 x 3 x 512 x 512 logits, this ~35)"""
    if nnf.softmax_stats_supported(score):
        return nnf.softmax_stats(score, want_label=True, want_entropy=False, want_top=False)[0]
    return torch.argmax(score, dim=1)


def score_mask(pred: torch.Tensor, pseudo: torch.Tensor, th: float = 0.7) -> torch.Tensor:
    """train_vqreptunet1x1v2.py:43-46."""
    if nnf.softmax_stats_supported(pred):
        top = nnf.softmax_stats(pred, want_label=False, want_entropy=False, want_top=True)[2]
    else:
        top = torch.softmax(pred.float(), dim=1).max(dim=1)[0]
    return torch.where(top > th, pseudo, torch.full_like(pseudo, 255))


class CPSTrainer:
    averages: Sequence[AveragedNetwork] = ()              # cfg.ema_decay: one per network (and `teachers`, their modules); empty = no teacher
    teachers: Sequence[nn.Module] = ()

    def __init__(self, cfg: CPSConfig, device, models: Optional[List[nn.Module]] = None):
        """`models`: an already built (model_1, model_2) pair on `device` (fixtures with given weights); else the pair is built
        from cfg.model as the reference trainer does (train_vqreptunet1x1v2.py:70-80)."""
        self.cfg, self.device = cfg, device
        if cfg.ema_decay is not None and not (torch.device(device).type == "cuda" and nnf.py_opt("py_hip_adam", 1)):
            raise ValueError("ema_decay: the averaged networks are kept inside optim.HipAdam's launch, which needs a 'cuda' (ROCm) device and "
                             "py_hip_adam = 1. There is no CPU path.")
        self.aux: Dict[str, torch.Tensor] = {}
        torch.manual_seed(cfg.seed)                      # same initial weights on every rank
        self.models = list(models) if models is not None else [make_model(cfg.model).to(device), make_model(cfg.model).to(device)]
        if cfg.init_weights and models is None:          # train_vqreptunet1x1v2.py:73-80
            for m in self.models:
                init_weight([m.decoder, m.segmentation_head], nn.init.kaiming_normal_, nn.BatchNorm2d, cfg.bn_eps,
                            cfg.bn_momentum, mode="fan_in", nonlinearity="relu")
        if vdist.collectives_on():
            for m in self.models:
                broadcast_module_state(m)
                nnf.invalidate_weight_caches(m)          # `.data` writes do not bump the version counter (_wcache)
        for m in self.models:
            m.async_code_usage = True                     # no host sync inside forward (usage is read after the step)
        self.buckets = [GradBuckets(list(m.parameters()), cfg.bucket_mb) for m in self.models]
        # the two networks of a CPS pair are independent until the loss: each runs on its own HIP stream (lanes.Lanes) so that one
        # model's small, latency-bound kernels (statistics merges, reductions, packs) hide under the other's large ones
        two = device.type == "cuda" and cfg.two_streams and os.environ.get("VQSEG_TWO_STREAMS", "1") == "1"
        prio = nnf.py_opt("py_stream_prio", 0) if device.type == "cuda" else 0      # A/B: 1 = the networks' streams above the weight-gradient side streams
        self.lanes = Lanes(device, len(self.models), two, bool(two and cfg.wgrad_side_stream and nnf.py_opt("py_wgrad_side", 1)), prio)
        self._glue = OFF                                  # where the glue between the forwards runs this step: see step()
        for k, b in enumerate(self.buckets):
            b.producer_streams = self.lanes.producers(k)
        # the reference's optimiser (train_vqreptunet1x1v2.py:106-107) on the HIP step kernel: Adam + the convolution kernels' weight
        # images in one launch per network (optim.HipAdam IS a torch.optim.Adam: same state / state_dict layout)
        self.opts = [HipAdam(m.parameters(), lr=cfg.learning_rate, betas=(0.9, 0.999)) if self.device.type == "cuda" and nnf.py_opt("py_hip_adam", 1)
                     else torch.optim.Adam(m.parameters(), lr=cfg.learning_rate, betas=(0.9, 0.999), fused=self.device.type == "cuda")
                     for m in self.models]
        # the teachers (cfg.ema_decay): built after the init and the rank-0 broadcast, so every rank's teacher starts from the same bits;
        # network k's teacher is written by network k's Adam launch on network k's stream (the end-of-step _join() shows it to the caller)
        if cfg.ema_decay is not None:
            self.averages = []
            with torch.random.fork_rng(devices=[device]):    # building the teachers draws nothing from the run's generators
                for m, o in zip(self.models, self.opts):
                    avg = AveragedNetwork(m, lambda: make_model(cfg.model), cfg.ema_decay)
                    avg.module.async_code_usage = True
                    o.attach_average(avg)
                    self.averages.append(avg)
            self.teachers = [a.module for a in self.averages]
        self.sched = CosineAnnealingLR(cfg.learning_rate, cfg.min_lr, cfg.total_iters, cfg.warmup_steps)
        self.ce = nn.CrossEntropyLoss(ignore_index=255)
        fixed = None
        if cfg.class_weight is not None and not isinstance(cfg.class_weight, str):
            fixed = torch.tensor([float(v) for v in cfg.class_weight], dtype=torch.float32, device=device)
        self._fixed_weight = fixed
        self.criterion = make_loss(cfg.criterion, cfg.num_classes, ignore_index=255, weight=fixed)
        if isinstance(self.criterion, FocalLoss):
            self.criterion.alpha, self.criterion.gamma = cfg.focal_alpha, cfg.focal_gamma
        self.sup_con = SupConLoss(cfg.sup_con_temperature) if cfg.sup_con_loss_weight is not None else None
        self.iter = 0

    @property
    def _two_streams(self) -> bool:
        """whether the networks run on their own streams; assignable on a live trainer (tools run single-stream sections), read
        at the start of every step and forward pair"""
        return self.lanes.enabled

    @_two_streams.setter
    def _two_streams(self, on: bool):
        self.lanes.enabled = on

    def _fwd_pair(self, a1, a2, use_amp=True, models=None, sides=None, **kw):
        """model 1 on a1 = (x[, gt]) and model 2 on a2, phase by phase: encoders overlap on the two streams, the VQ phases
        run one after the other with the other stream idle (the distance kernels fill the GPU on their own, and their
        in-stream timing -- bench.py's roofline -- then measures the kernel, not the sharing), decoders overlap again.
        One stream or two, the phases are enqueued in this order (also the order of the RNG draws of the k-means inits).
        `use_amp=False`: this pair runs outside autocast whatever cfg.amp_dtype says (the pseudo-label passes).
        `models`: the pair of modules to run (the teachers, for their pseudo labels), on the same streams; default the students.
        `sides`: a pair of dicts, one per network, handed to its finish() as `side` (the contrastive term of the labelled pair)."""
        m1, m2 = models or self.models
        L, amp = self.lanes, self.cfg.amp_dtype if use_amp else None

        def run(k, fn, *args, **kws):
            with L.on(k, amp):
                return fn(*args, **kws)

        L.fork()
        f1, f2 = run(0, m1.encode, a1[0]), run(1, m2.encode, a2[0])
        alone = L.enabled and nnf.py_opt("py_vq_alone", 1)              # 0 (A/B runs): the VQ phases share the chip like everything else
        if alone:
            L.hold(0)                                                   # model 2's encoder done before model 1 quantises
        q1 = run(0, m1.quantize, f1)
        if alone:
            L.hold(1)
        q2 = run(1, m2.quantize, f2)
        if alone:
            L.hold(0)                                                   # ... and model 1 stays idle meanwhile
        if sides is None:
            o1, o2 = run(0, m1.finish, *q1, *a1[1:], **kw), run(1, m2.finish, *q2, *a2[1:], **kw)
        else:
            o1, o2 = run(0, m1.finish, *q1, *a1[1:], side=sides[0], **kw), run(1, m2.finish, *q2, *a2[1:], side=sides[1], **kw)
            L.to_caller(*(v for d in sides for v in d.values()))
        L.to_caller(*o1, *o2)
        return o1, o2

    def _join(self):
        """the caller's stream waits for everything queued on the per-model streams"""
        self.lanes.join()

    def step(self, l_input, l_target, ul_input, epoch_frac: float = 0.0) -> Dict[str, torch.Tensor]:
        """One CPS iteration on B labelled + B unlabelled images (6 forwards, 4 backwards per pair of
        models).  Returns device scalars (no host sync)."""
        # r4: the glue between the forwards -- bucket zeroing, pseudo-label targets, the loss block -- runs on the two networks' OWN
        # streams (what network k's stream produced is consumed there; the one exchange is the other network's mask / target, an event
        # each way) instead of joining both streams into the caller's and running ~150 small kernels there with the chip idle (measured
        # on a kernel trace: 3.2 ms of a 152 ms step).  Same operations, same operands, same order per network.  Decided here, once
        # per step; py_loss_streams=0 (A/B) leaves the forwards on the lanes and runs the glue on the caller's stream after a join.
        on_lanes = self.lanes.enabled and l_input.is_cuda and nnf.py_opt("py_loss_streams", 1) == 1
        self._glue = g = self.lanes if on_lanes else OFF
        g.fork()
        for k, b in enumerate(self.buckets):                            # each network's buckets are written by ITS stream's backward:
            with g.on(k):                                               # zeroed there too, under the first forward's kernels
                b.zero()
        nnf.drop_pending_wgrads()
        if l_input.is_cuda:
            # one layout conversion per batch instead of one per forward, and one stem patch matrix per batch for the six
            # forwards of the step (nnf.stem_share_*): the two networks and the two passes over the unlabelled batch see
            # the same images
            l_input = l_input.contiguous(memory_format=torch.channels_last)
            ul_input = ul_input.contiguous(memory_format=torch.channels_last)
            if nnf.py_opt("py_stem_share", 1):
                nnf.stem_share_begin()
        prev = nnf.set_fanin_fusion(True)                              # fan-in adds inside the consumers' kernels; checked after backward
        try:
            return self._step(l_input, l_target, ul_input, epoch_frac)
        finally:
            nnf.set_fanin_fusion(prev)
            nnf.stem_share_end()

    def _step(self, l_input, l_target, ul_input, epoch_frac):
        """the phases of a step, in order; each adds what it has in scope to `self.aux` (cfg.keep_aux)"""
        cfg = self.cfg
        if cfg.keep_aux:
            self.aux = {}
        score_1, score_2 = self._pseudo_scores(ul_input)
        ul_train, score_1, score_2 = self._cutmix(self._photometric(ul_input), score_1, score_2)
        gt_ul_1, gt_ul_2, kw = self._targets(score_1, score_2, epoch_frac)
        segments = self._superpixels(l_input, ul_train)
        salient = self._saliency(l_input, ul_train, segments)
        sup, unsup, sup_con = self._train_forwards(l_input, l_target, ul_train, gt_ul_1, gt_ul_2, kw)
        fused, ps1, sup_terms, cps_terms, fp = self._terms(l_target, sup, unsup, score_1, score_2, kw, segments, salient)
        lr = self.sched.get_lr(self.iter)
        for o in self.opts:
            o.param_groups[0]["lr"] = lr
        loss, terms = self._total_loss(fused, sup_terms, cps_terms, [o[1] for o in sup + unsup], [o[3] for o in sup + unsup])
        if fp is not None:                                              # reported unweighted; cps_loss holds it with feature_perturb_weight
            terms["fp_loss"] = fp[0] + fp[1]
        if sup_con is not None:                                         # train_supcon_unet.py:143-153: weight * (l_1 + l_2) joins the total
            terms["sup_con_loss"] = (sup_con[0] + sup_con[1]) * cfg.sup_con_loss_weight
            loss = loss + terms["sup_con_loss"]
        self._backward_and_step(loss)
        self.iter += 1
        with torch.no_grad():
            miou, _ = miou_device(confusion_matrix_device(ps1, l_target, cfg.num_classes))
        self._join()
        return {"loss": loss.detach(), **{k: v.detach() for k, v in terms.items()}, "miou": miou, "lr": torch.tensor(lr)}

    @torch.no_grad()
    def _pseudo_scores(self, ul_input):
        """The two eval forwards (students, or teachers) over the unlabelled batch -> score_1, score_2 in fp32, each on its
        network's stream.  With the easy augmentation the forwards see the warped batch and the scores are warped back, so
        what is returned is always in the clean frame."""
        cfg, g = self.cfg, self._glue
        m1, m2 = self.models
        m1.eval(); m2.eval()
        ul_easy = ul_input
        if cfg.easy_aug is not None:
            # easy augmentation: the step's transforms on the host, a pure function of (seed, rank, iteration[, sample]) under a key of
            # their own (the CutMix boxes of the step do not move).  The images are warped ONCE on the caller's stream, for both networks
            codes, angles = augmentations.step_transforms(ul_input.shape[0], cfg.seed, vdist.rank(), self.iter, cfg.easy_aug_per,
                                                          cfg.easy_aug_codes, cfg.easy_aug_max_angle)
            ul_easy = augmentations.warp_batch(ul_input, augmentations.similarity_matrices(codes, angles))
            self.lanes.share(ul_easy)
        o1, o2 = self._fwd_pair((ul_easy,), (ul_easy,), use_amp=cfg.eval_amp, models=self.teachers if cfg.teacher_pseudo_labels else None)
        if g is OFF:
            self._join()
        with g.on(0):
            score_1 = o1[0].float()
        with g.on(1):
            score_2 = o2[0].float()
        if cfg.easy_aug is not None:
            # back into the clean frame, each score map on the stream that made it; from here on the step is the plain one
            back = augmentations.similarity_matrices(codes, angles, inverse=True)
            easy_1, easy_2 = score_1, score_2
            with g.on(0):
                score_1 = augmentations.warp_batch(easy_1, back)
            with g.on(1):
                score_2 = augmentations.warp_batch(easy_2, back)
            if cfg.keep_aux:                                            # the forwards' own maps beside the clean-frame ones
                self.aux.update(ul_easy=ul_easy, easy_codes=list(codes), easy_angles=list(angles), score_1_easy=easy_1, score_2_easy=easy_2)
                g.to_caller(easy_1, easy_2)
        m1.train(); m2.train()
        if cfg.keep_aux:                                                # the clean-frame maps, before any mixing
            self.aux.update(score_1=score_1, score_2=score_2)
            g.to_caller(score_1, score_2)
        return score_1, score_2

    @torch.no_grad()
    def _photometric(self, ul_input):
        """cfg.hard_aug -> the clean unlabelled batch through the step's photometric rows (colour jitter, grayscale, blur): the images
        the unlabelled training forwards (and CutMix before them) receive; else the batch as it came, and nothing is entered."""
        cfg, g = self.cfg, self._glue
        if cfg.hard_aug is None:
            return ul_input
        # rows on the host, a pure function of (seed, rank, iteration[, sample]) under a key of their own (the boxes and the easy
        # transforms of the step do not move).  Distorted ONCE on the caller's stream (both networks get the same tensor object: one stem
        # patch matrix); the score maps stay as they are -- no pixel moves
        rows = augmentations.step_photometric(ul_input.shape[0], cfg.seed, vdist.rank(), self.iter, cfg.hard_aug_per, cfg.hard_aug_jitter,
                                              cfg.hard_aug_jitter_p, cfg.hard_aug_gray_p, cfg.hard_aug_blur_p, cfg.hard_aug_sigma)
        ul_hard = augmentations.photometric(ul_input, rows)
        g.share(ul_hard)
        if cfg.keep_aux:
            self.aux.update(ul_photometric=ul_hard, photometric_params=list(rows))
        return ul_hard

    @torch.no_grad()
    def _cutmix(self, ul_input, score_1, score_2):
        """-> the images of the two unlabelled training forwards and the score maps the pseudo labels come from: box-mixed with
        the same boxes (cfg.cutmix_ratio), or as they came."""
        cfg, g = self.cfg, self._glue
        if cfg.cutmix_ratio is None:
            return ul_input, score_1, score_2
        # boxes on the host, a pure function of (seed, rank, iteration[, sample]) -- no generator state to checkpoint, nothing taken
        # from the global generators.  The images are mixed ONCE (both networks get the same tensor object: one stem patch matrix),
        # each score map on the stream that made it, before anything derives a pseudo label from it; from here on the step is the
        # plain one on mixed scores and, for the two training forwards, mixed images.
        boxes = augmentations.step_boxes(ul_input.shape[0], ul_input.shape[-2], ul_input.shape[-1], cfg.cutmix_ratio, cfg.seed,
                                         vdist.rank(), self.iter, cfg.cutmix_boxes)
        ul_train = augmentations.mix_boxes(ul_input, boxes)
        g.share(ul_train)
        with g.on(0):
            mixed_1 = augmentations.mix_boxes(score_1, boxes)
        with g.on(1):
            mixed_2 = augmentations.mix_boxes(score_2, boxes)
        if cfg.keep_aux:                                                # what the step used, beside the clean maps
            self.aux.update(ul_mixed=ul_train, score_1_mixed=mixed_1, score_2_mixed=mixed_2, boxes=list(boxes))
        return ul_train, mixed_1, mixed_2

    @torch.no_grad()
    def _superpixels(self, l_input, ul_train):
        """cfg.superpixel_mean -> (labelled label maps, unlabelled label maps, K_eff): SLIC of the two batches as the training forwards
        receive them, once each, on the caller's stream, for both networks' lanes; else None, and nothing is entered."""
        cfg, g = self.cfg, self._glue
        if cfg.superpixel_mean is None:
            return None
        maps = []
        for images in (l_input, ul_train):
            labels, _centers, (gy, gx) = superpixel.slic(images.float(), cfg.superpixel_mean, cfg.superpixel_compactness, cfg.superpixel_iters,
                                                         return_centers=True)
            maps.append(labels)
        self._slic_grid = (gy, gx)                                      # for _saliency, when it can use these maps
        g.fork()                                                        # the lanes wait for the maps
        for labels in maps:
            g.share(labels)
        if cfg.keep_aux:
            self.aux.update(superpixels_l=maps[0], superpixels_ul=maps[1])
        return maps[0], maps[1], gy * gx

    @torch.no_grad()
    def _saliency(self, l_input, ul_train, segments=None):
        """cfg.salient_mask -> (labelled maps, unlabelled maps): RBD saliency of the two batches as the training forwards receive them,
        once each, on the caller's stream, for both networks' lanes; else None, and nothing is entered.  SLIC with cfg.salient_segments
        components and cfg.superpixel_compactness / superpixel_iters (10 and 10: the reference's); where cfg.superpixel_mean asks for the
        same component count, `segments`' label maps serve both and SLIC runs once per batch, else each option runs its own."""
        cfg, g = self.cfg, self._glue
        if cfg.salient_mask is None:
            return None
        if segments is not None and cfg.superpixel_mean == cfg.salient_segments:
            maps = [saliency.saliency_rbd_from_slic(images.float(), labels, self._slic_grid)
                    for images, labels in ((l_input, segments[0]), (ul_train, segments[1]))]
        else:
            maps = [saliency.saliency_rbd(images.float(), cfg.salient_segments, cfg.superpixel_compactness, cfg.superpixel_iters)
                    for images in (l_input, ul_train)]
        g.fork()                                                        # the lanes wait for the maps
        for m in maps:
            g.share(m)
        if cfg.keep_aux:
            self.aux.update(saliency_l=maps[0], saliency_ul=maps[1])
        return maps[0], maps[1]

    def _targets(self, score_1, score_2, epoch_frac):
        """-> gt_ul_1, gt_ul_2 (each network's unlabelled target comes from the OTHER network's scores, made on that network's
        stream) and the recipe's keyword of the training forwards"""
        cfg, g = self.cfg, self._glue
        if cfg.recipe != "v1":
            return score_2, score_1, dict(th=cfg.confidence_threshold)
        with g.on(1):
            gt_ul_1 = _argmax_classes(score_2)
        with g.on(0):
            gt_ul_2 = _argmax_classes(score_1)
        return gt_ul_1, gt_ul_2, dict(percent=100 - cfg.unsup_loss_drop_percent * (1 - epoch_frac))

    def _train_forwards(self, l_input, l_target, ul_train, gt_ul_1, gt_ul_2, kw):
        """the labelled and the unlabelled training forward pair -> ((out_1, out_2), (out_1, out_2), sup_con), out = (pred, commitment,
        usage, prototype).  The targets cross lanes: as of now (they are ready), waited for only before the unlabelled pair.
        sup_con: cfg.sup_con_loss_weight -- each network's contrastive scalar of its labelled forward, made inside that forward on its
        stream (the dicts are this call's own: nothing stays on the modules); else None, and the pair runs exactly as without the option."""
        g = self._glue
        ready = g.mark()
        sup_con = None
        if self.sup_con is None:
            sup = self._fwd_pair((l_input, l_target), (l_input, l_target), **kw)
        else:
            sides = tuple(dict(sup_con=self.sup_con, keep=self.cfg.keep_aux) for _ in self.models)
            sup = self._fwd_pair((l_input, l_target), (l_input, l_target), sides=sides, **kw)
            sup_con = tuple(d["sup_con_loss"] for d in sides)
            if self.cfg.keep_aux:
                self.aux.update(decoder_out_1=sides[0]["decoder_out"], decoder_out_2=sides[1]["decoder_out"], sup_con_1=sup_con[0].detach(),
                                sup_con_2=sup_con[1].detach())
        g.exchange(gt_ul_2, gt_ul_1, marks=ready)
        if self.cfg.feature_perturb is None:
            unsup = self._fwd_pair((ul_train, gt_ul_1), (ul_train, gt_ul_2), **kw)
        else:
            # cfg.feature_perturb: each network's unlabelled forward decodes 2B images (models: decode with a perturbation spec) and
            # returns the perturbed stream's prediction as a fifth output.  The key of network k's keep table: (cfg.seed, 2 * rank + k,
            # iteration) -- drawn on its stream by nnf.channel_keep and left in the dict under "scale"
            sides = tuple(dict(perturb=dict(p=self.cfg.feature_perturb, seed=self.cfg.seed, stream=2 * vdist.rank() + k, step=self.iter))
                          for k in range(len(self.models)))
            unsup = self._fwd_pair((ul_train, gt_ul_1), (ul_train, gt_ul_2), sides=sides, **kw)
            self.lanes.to_caller(*(d["perturb"]["scale"] for d in sides))
            if self.cfg.keep_aux:
                self.aux.update(perturb_scale_1=sides[0]["perturb"]["scale"], perturb_scale_2=sides[1]["perturb"]["scale"])
        if g is OFF:
            self._join()
        return sup, unsup, sup_con

    def _criterion(self, cls_weight, pred):
        """-> (crit(pred, target), fused): what the four terms of a step are computed with.  fused: the terms stay as their
        (inter, sets[, ce]) sums and _total_loss combines them in one launch."""
        cfg, crt = self.cfg, self.criterion
        if cls_weight is not None or not isinstance(crt, DiceLoss):    # recipe v1 only (cfg.__post_init__)
            return (lambda p, t: self._weighted(p, t, cls_weight)), False
        if cfg.unsup_criterion is not None:                            # the CPS terms gain a scalar the one-launch combination does not take
            return crt, False
        if cfg.feature_perturb is not None:                            # likewise: the perturbed stream's term
            return (crt if cfg.recipe == "v1" else self._ce_dice), False
        if (crt.weight is None and crt.ignore_index is not None and pred.is_cuda and nnf.dice_sums_supported(pred, crt.num_classes)
                and nnf.py_opt("py_loss_combine", 1) == 1):
            sums = nnf.dice_sums if cfg.recipe == "v1" else nnf.dice_ce_sums
            return (lambda p, t: sums(p, t, crt.ignore_index)), True
        return (crt if cfg.recipe == "v1" else self._ce_dice), False

    def _perturbed_pred(self, pu_fp, segments=None, salient=None):
        """a network's fp32 prediction of its feature-perturbation stream (cfg.feature_perturb) through the steps its clean unlabelled
        prediction takes in _own_mask -- the superpixel mean, the salient masking -- on this network's stream; it contributes to no mask"""
        pu_fp = pu_fp.float()
        if segments is not None:
            pu_fp = superpixel.superpixel_mean(pu_fp, segments[1], segments[2])
        if salient is not None:
            pu_fp = saliency.salient_masking(pu_fp, salient[1], self.cfg.salient_mask)
        return pu_fp

    def _own_mask(self, ps, pu, kw, segments=None, salient=None):
        """a network's fp32 predictions (labelled, unlabelled, both), the pseudo-label mask it hands to the other network, and that mask
        before the area filter (cfg.pseudo_min_area; the same tensor when the option is off).
        `segments` (cfg.superpixel_mean): both predictions are first averaged over their batch's superpixels, on this network's stream.
        `salient` (cfg.salient_mask): then the scores of the classes >= 1 are zeroed where the batch's saliency map is <= the threshold"""
        ps, pu = ps.float(), pu.float()
        if segments is not None:
            ps, pu = superpixel.superpixel_mean(ps, segments[0], segments[2]), superpixel.superpixel_mean(pu, segments[1], segments[2])
        if salient is not None:
            ps, pu = (saliency.salient_masking(ps, salient[0], self.cfg.salient_mask),
                      saliency.salient_masking(pu, salient[1], self.cfg.salient_mask))
        pred = torch.cat([ps, pu], dim=0)
        if self.cfg.recipe == "v1":
            mask = regularized_pseudo_label(pred, kw["percent"])
        else:
            mask = score_mask(pred, _argmax_classes(pred), kw["th"])
        raw = mask
        if self.cfg.pseudo_min_area is not None:                        # specks of confident noise do not supervise the other network
            mask = regions.remove_small_regions(raw, self.cfg.pseudo_min_area, self.cfg.pseudo_connectivity, ignore=(255,), fill=255)
        return ps, pu, pred, mask, raw

    def _terms(self, l_target, sup, unsup, score_1, score_2, kw, segments=None, salient=None):
        """Each network's own mask and its two criterion terms (supervised; CPS against the other's mask) on its stream ->
        fused, pred_sup_1, (sup_1, sup_2), (cps_1, cps_2), fp.  Ends the glue: the caller's stream joins the lanes.
        fp: cfg.feature_perturb -- (fp_1, fp_2), network k's criterion of its perturbed stream's prediction against the OTHER network's
        mask of the unlabelled batch, on its stream, already inside cps_k with cfg.feature_perturb_weight; else None, nothing entered."""
        cfg, g = self.cfg, self._glue
        cls_weight = self._fixed_weight
        if cfg.class_weight == "balanced":
            # this step's labelled targets weigh all four terms, as train_vq_pt_unet_balncedweightedloss.py:135-141 does; the counting
            # kernel leaves the weights on the device (no bincount, no host round trip).  One tensor for both networks' streams.
            cls_weight = compute_class_weight(cfg.num_classes, l_target)
            g.fork()
            g.share(cls_weight)
        with g.on(0):
            ps1, pu1, pred_1, mask_1, raw_1 = self._own_mask(sup[0][0], unsup[0][0], kw, segments, salient)
        with g.on(1):
            ps2, pu2, pred_2, mask_2, raw_2 = self._own_mask(sup[1][0], unsup[1][0], kw, segments, salient)
        g.exchange(mask_1, mask_2)
        crit, fused = self._criterion(cls_weight, pred_1)
        soft = cfg.unsup_criterion is not None                          # the unlabelled half of the CPS terms is _soft_cps's
        b_l = ps1.shape[0]
        with g.on(0):
            cps_1, sup_1 = (crit(ps1, mask_2[:b_l]) if soft else crit(pred_1, mask_2)), crit(ps1, l_target)
        with g.on(1):
            cps_2, sup_2 = (crit(ps2, mask_1[:b_l]) if soft else crit(pred_2, mask_1)), crit(ps2, l_target)
        fp = None
        if cfg.feature_perturb is not None:
            with g.on(0):
                pu_fp_1 = self._perturbed_pred(unsup[0][4], segments, salient)
                fp_1 = crit(pu_fp_1, mask_2[b_l:])
                cps_1 = cps_1 + cfg.feature_perturb_weight * fp_1
            with g.on(1):
                pu_fp_2 = self._perturbed_pred(unsup[1][4], segments, salient)
                fp_2 = crit(pu_fp_2, mask_1[b_l:])
                cps_2 = cps_2 + cfg.feature_perturb_weight * fp_2
            fp = (fp_1, fp_2)
        g.join()
        if fp is not None:
            g.to_caller(fp_1, fp_2, pu_fp_1, pu_fp_2, pu1, ps2)
            if cfg.keep_aux:                                            # what fp_loss and cps_loss are restated from
                self.aux.update(pred_fp_1=pu_fp_1.detach(), pred_fp_2=pu_fp_2.detach(), pred_ul_1=pu1.detach(), pred_sup_2=ps2.detach())
        g.to_caller(cps_1, sup_1, cps_2, sup_2, ps1, pu2, mask_1, mask_2, score_1, score_2)
        if soft:
            g.to_caller(pu1, ps2)
            cps_1, cps_2 = self._soft_cps(cps_1, cps_2, ps1, ps2, pu1, pu2, kw)
        if cfg.keep_aux:
            self.aux.update(mask_1=mask_1, mask_2=mask_2, pred_sup_1=ps1.detach(), pred_ul_2=pu2.detach())
            if cfg.pseudo_min_area is not None:                         # the masks before the area filter
                self.aux.update(mask_1_unfiltered=raw_1, mask_2_unfiltered=raw_2)
                g.to_caller(raw_1, raw_2)
            if segments is not None:                                    # the unpooled logits of network 1, and what the terms are restated from
                raw_s, raw_u = sup[0][0].detach().float(), unsup[0][0].detach().float()
                self.aux.update(pred_sup_1_unpooled=raw_s, pred_ul_1_unpooled=raw_u, pred_1=pred_1.detach(), pred_2=pred_2.detach())
                g.to_caller(raw_s, raw_u, pred_1, pred_2)
            if salient is not None:                                     # the unmasked logits of network 1, and what the terms are restated from
                raw_s, raw_u = sup[0][0].detach().float(), unsup[0][0].detach().float()
                self.aux.update(pred_sup_1_unmasked=raw_s, pred_ul_1_unmasked=raw_u, pred_1=pred_1.detach(), pred_2=pred_2.detach())
                g.to_caller(raw_s, raw_u, pred_1, pred_2)
            if cls_weight is not None or not isinstance(self.criterion, DiceLoss):     # what the criterion arms' terms are restated from
                self.aux.update(pred_1=pred_1.detach(), pred_2=pred_2.detach(), class_weight=cls_weight)
                g.to_caller(pred_1, pred_2)
        return fused, ps1, (sup_1, sup_2), (cps_1, cps_2), fp

    def _soft_cps(self, cps_1, cps_2, ps1, ps2, pu1, pu2, kw):
        """cfg.unsup_criterion == "conf_ce" -> the two CPS terms with their unlabelled halves added, on the caller's stream after the
        lanes have joined (the term's gradient reaches both networks): network k's is uw_other * conf_ce_loss(pu_k <- pu_other),
        uw_other the unreliable weight of the logits that serve as targets (train_vq_pt_unet_conf_ce.py:225-228)."""
        cfg = self.cfg
        par = (cfg.conf_ce_threshold, cfg.conf_ce_threshold_neg, cfg.conf_ce_temperature)
        if nnf.conf_ce_supported(pu1, pu2):
            l_1, l_2 = nnf.conf_ce_pair(pu1, pu2, *par, cfg.conf_ce_detach_targets)      # one launch forward, one backward, both directions
        else:
            l_1 = conf_ce_loss(pu1, pu2, True, *par, detach_targets=cfg.conf_ce_detach_targets)
            l_2 = conf_ce_loss(pu2, pu1, True, *par, detach_targets=cfg.conf_ce_detach_targets)
        if cfg.conf_ce_unreliable_weight:
            uw_1, uw_2 = unreliable_weight(pu1.detach(), kw["percent"]), unreliable_weight(pu2.detach(), kw["percent"])
        else:
            uw_1 = uw_2 = torch.ones((), dtype=torch.float32, device=pu1.device)
        if cfg.keep_aux:                                                # uw_k: of network k's logits, so it weighs the OTHER network's term
            self.aux.update(conf_ce_1=l_1.detach(), conf_ce_2=l_2.detach(), uw_1=uw_1, uw_2=uw_2, pred_ul_1=pu1.detach(), pred_sup_2=ps2.detach())
        return cps_1 + uw_2 * l_1, cps_2 + uw_1 * l_2

    def _total_loss(self, fused, sup, cps, commit, proto):
        """-> loss and the reported terms.  fused: the whole combination -- terms from their sums, commitment, prototype, total, and
        its gradient -- is one launch (nnf.cps_loss_combine); else scalar torch ops.  `commit` / `proto`: the four forwards' losses,
        labelled pair first."""
        cfg = self.cfg
        if fused:
            combined = nnf.cps_loss_combine(list(sup), list(cps), cfg.cps_loss_weight, 0.0 if cfg.recipe == "v1" else 0.5,
                                            commit, cfg.total_commitment_loss_weight, proto, cfg.total_prototype_loss_weight)
            if combined is not None:
                loss, stats = combined
                return loss, dict(sup_loss_1=stats[4], sup_loss_2=stats[5], cps_loss=stats[3], commitment_loss=stats[1], prototype_loss=stats[2])

            def scalar(t):                                              # inputs the kernel does not take: the same terms with torch ops
                dice = 1 - (2 * t[0] / (t[1] + 1e-6)).mean(dim=0).mean()
                return dice if len(t) == 2 else 0.5 * (t[2][:, 0].sum() / t[2][:, 1].sum()) + dice
            c1, s1, c2, s2 = scalar(cps[0]), scalar(sup[0]), scalar(cps[1]), scalar(sup[1])
            cps, sup = (c1, c2), (s1, s2)
        cps_sum = cps[0] + cps[1]
        commitment = (commit[0] + commit[1] + commit[2] + commit[3]) * cfg.total_commitment_loss_weight
        prototype = (proto[0] + proto[1] + proto[2] + proto[3]) * cfg.total_prototype_loss_weight
        com_sum = commitment.sum()
        loss = sup[0] + sup[1] + cfg.cps_loss_weight * cps_sum + com_sum + prototype.float()
        return loss, dict(sup_loss_1=sup[0], sup_loss_2=sup[1], cps_loss=cps_sum, commitment_loss=com_sum, prototype_loss=prototype)

    def _backward_and_step(self, loss):
        """backward (weight gradients on their side streams, if configured), gradient reduction, optimiser step"""
        L = self.lanes
        L.wgrad_sides(True)
        try:
            loss.backward()
        finally:
            L.wgrad_sides(False)
        nnf.flush_pending_wgrads()                                      # two-use weight gradients whose second use never came (none, normally)
        nnf.check_fanin_consumed()
        if L.enabled and nnf.py_opt("py_opt_streams", 1):
            # each network's gradient reduction + optimiser step on ITS stream (the sinks wrote p.grad there): the two Adam launches
            # overlap each other and the metric kernels of the caller; the caller's stream joins both before the step returns.
            # (backward's leaf streams are joined into the caller's by autograd; the side streams are not)
            L.fork(sides=True)
            for k, (b, o) in enumerate(zip(self.buckets, self.opts)):
                with L.on(k):
                    b.finish()
                    o.step()
        else:
            L.join(*range(len(self.models)), sides=True)               # the sinks wrote p.grad on the per-model (and side) streams
            for b in self.buckets:
                b.finish()
            for o in self.opts:
                o.step()

    def sync_buffers(self):
        """Data parallel: BatchNorm running statistics are per-rank (each rank normalises with its own batch statistics -- the
        reference's single-device semantics per rank; parameters and codebooks ARE identical on all ranks).  This broadcasts
        rank 0's buffers to every rank -- an EXPLICIT act (end of training, before an all-rank evaluation).  Nothing on the training
        path calls it: the eval-mode pseudo-label forwards read the running statistics, so a hidden sync (round 2 had one inside
        save_checkpoint) would make the trajectory of ranks > 0 depend on how often checkpoints are written."""
        if vdist.collectives_on():
            for m in self.models:
                for b in m.buffers():
                    dist.broadcast(b.data, src=0)

    def state_dicts(self, sync: bool = False):
        """(model_1, model_2, optimizer_1, optimizer_2) state_dicts for utils.ckpoints.save_ckpoints -- THIS rank's state.
        `sync=True` first broadcasts rank 0's BatchNorm buffers (a collective that changes ranks > 0: see sync_buffers)."""
        if sync:
            self.sync_buffers()
        return (self.models[0].state_dict(), self.models[1].state_dict(), self.opts[0].state_dict(), self.opts[1].state_dict())

    def save_checkpoint(self, filepath, epoch: int = 0, batch_idx: int = 0):
        """The reference's checkpoint dictionary (utils/ckpoints.py:7-13: model_1, model_2, epoch, batch_idx, optimizer_1,
        optimizer_2) plus what a bit-exact resume needs and the reference does not store: the `initted` flags and
        the iteration counter that positions the cosine schedule.  Rank 0 writes ITS state (parameters, codebooks and optimiser
        moments are identical on all ranks; the BatchNorm running statistics in the file are rank 0's); no collective, no rank's
        state is touched -- writing a checkpoint cannot alter the run."""
        extra = {"iter": self.iter}
        if self.averages and vdist.rank() == 0:              # the teachers, beside the reference's keys
            for i, a in enumerate(self.averages):
                extra[f"ema_model_{i + 1}"] = a.state_dict()["module"]
            extra["ema_updates"] = [int(a.updates) for a in self.averages]
        if vdist.collectives_on() and vdist.world_size() > 1:    # every rank's own BatchNorm statistics (a collective; copies)
            for i, m in enumerate(self.models):
                extra[f"bn_buffers_model_{i + 1}"] = gather_rank_buffers(m, self.device)
        if vdist.rank() == 0:
            m1, m2, o1, o2 = self.state_dicts()
            save_ckpoints(m1, m2, epoch, batch_idx, o1, o2, filepath, models=self.models, extra=extra)

    def load_checkpoint(self, filepath):
        """Resume from save_checkpoint's file (or a reference-written one: then the flags and the counter stay as they are).
        Returns (epoch, batch_idx)."""
        state = load_training_state(filepath, map_location=self.device)
        for m, o, i in zip(self.models, self.opts, (1, 2)):
            m.load_state_dict(state[f"model_{i}"])
            o.load_state_dict(state[f"optimizer_{i}"])
            nnf.invalidate_weight_caches(m)
        for m, flags in zip(self.models, state.get("initted") or (None, None)):
            restore_initted(m, flags)
        for i, m in enumerate(self.models):                # data-parallel resume: this rank's own BatchNorm statistics (see save_checkpoint)
            restore_rank_buffers(m, state.get(f"bn_buffers_model_{i + 1}"), vdist.rank())
        for i, a in enumerate(self.averages):
            # a file without teachers (a reference checkpoint, or one written with the feature off): each a copy of the loaded student
            a.reset_from_student()
            if f"ema_model_{i + 1}" in state:
                a.load_state_dict({"module": state[f"ema_model_{i + 1}"], "updates": state["ema_updates"][i]})
        self.iter = int(state.get("iter", self.iter))
        return state.get("epoch", 0), state.get("batch_idx", 0)

    def _networks(self, which: str):
        """the pair `which` names: "student" the trained weights, "teacher" their exponential moving averages (cfg.ema_decay)"""
        if which not in ("student", "teacher"):
            raise ValueError(f"which must be 'student' or 'teacher', got {which!r}")
        if which == "teacher" and not self.teachers:
            raise ValueError("which='teacher' needs a teacher: set CPSConfig.ema_decay")
        return self.teachers if which == "teacher" else self.models

    def evaluate(self, batches, which: str = "student", index: int = 0, fused: bool = False, visualize=None, window=None, stride=None,
                 blend: str = "linear", window_batch=None, net_size=None, crf=None, min_area=None, min_area_fill=0, connectivity: int = 4,
                 region_ignore=(), boundary=None, panoptic=None):
        """evaluate.test_loop on network `index` of the pair: which="student" scores the trained weights, which="teacher" their
        exponential moving average (cfg.ema_decay), under cfg.amp_dtype.  `batches` yields (images, labels).  `fused`: resize, arg-max
        and confusion counts in one kernel (evaluate.test_loop's opt-in; the same numbers).  `visualize` (with fused): a callable
        (batch_index, viz_v1, viz_v2) that receives the test script's two uint8 sheets per batch (evaluate.test_loop).  `window`
        (with fused; `stride`, `blend`, `window_batch`, `net_size`): tiled scoring, as predict.Predictor(window=...) predicts.  `crf`
        (with fused; a utils.crf.DenseCRF or True): the dense-CRF refinement is scored, as predict.Predictor(crf=...) predicts.
        `min_area` (with fused; `min_area_fill`, `connectivity`, `region_ignore`): the area-filtered class maps are scored, as
        predict.Predictor(min_area=...) predicts.  `boundary` (with fused; True or a dict of `tolerance`, `width`, `ignore`): boundary F1,
        boundary IoU and the Hausdorff distance of the scored class maps are added (utils.boundary.BoundaryMeasurement).  `panoptic` (with
        fused; True or a dict of `things`, `void`, `connectivity`, `capacity`): panoptic, segmentation and recognition quality and the
        instance-count error of the scored class maps are added (utils.instances.InstanceMeasurement)."""
        model = self._networks(which)[index]
        return test_loop(model, batches, self.cfg.num_classes, device=self.device, amp_dtype=self.cfg.amp_dtype, fused=fused, visualize=visualize,
                         window=window, stride=stride, blend=blend, window_batch=window_batch, net_size=net_size, crf=crf, min_area=min_area,
                         min_area_fill=min_area_fill, connectivity=connectivity, region_ignore=region_ignore, boundary=boundary, panoptic=panoptic)

    @torch.no_grad()
    def example_image(self, l_input, l_target, ul_input, which: str = "student", index: int = 0, half: bool = True):
        """The trainer's end-of-epoch sheet (train_vqreptunet1x1v2.py:239-244): [input | target | prediction | 20 px white |
        0.6 unlabelled input + 0.4 its prediction], the batch stacked vertically, as a uint8 (B * H [/ 2], (4 W + 20) [/ 2], 3) numpy
        array (utils.visualize.make_example_img; `half`: its resize_factor = 0.5).  The predictions are no-grad eval-mode forwards
        of network `index` of the pair `which` names, under cfg.amp_dtype; the reference feeds the TRAIN-mode predictions of the
        epoch's last step, which this trainer does not keep.  Every network's mode is restored on the way out."""
        from .utils.visualize import make_example_img
        model = self._networks(which)[index]
        p = Predictor(model, self.cfg.num_classes, amp_dtype=self.cfg.amp_dtype, device=self.device)
        was_training = model.training
        model.eval()
        try:
            (sup,), _ = p.views(l_input)
            (unsup,), _ = p.views(ul_input)
        finally:
            model.train(was_training)
        dev = sup.device
        return make_example_img(l_input.to(dev), l_target.to(dev), sup, ul_input.to(dev), unsup, colormap=default_palette(self.cfg.num_classes),
                                resize_factor=0.5 if half else None)

    def predict(self, images, size=None, which: str = "student", index: int = 0, ensemble: bool = False, tta=("none",),
                want_confidence: bool = False, window=None, stride=None, blend: str = "linear", window_batch=None, net_size=None,
                crf=None, superpixels=None, min_area=None, min_area_fill=0, connectivity: int = 4, region_ignore=()) -> Prediction:
        """Class maps of `images` (N, 3, H, W) at `size` (None: their own): predict.Predictor on network `index` of the pair `which`
        names, or with `ensemble` on both of them (mean of the two networks' logits), times the flipped views of `tta`, under
        cfg.amp_dtype.  `window` (with `stride`, `blend`, `window_batch`, `net_size`): tiled prediction at the images' own size
        (predict.Predictor).  `crf` (a utils.crf.DenseCRF or True; not with `window`): dense-CRF refinement of the prediction.
        `superpixels` (a component count or dict(num_components=, compactness=, iters=); not with `window` or `crf`): the class
        probabilities are averaged over SLIC superpixels of the images before the arg-max.  `min_area` (with `min_area_fill`,
        `connectivity`, `region_ignore`; every mode): regions of one class smaller than that are replaced after the arg-max.
        -> Prediction(label (N, Ho, Wo) uint8, confidence (N, Ho, Wo) f32 | None)."""
        nets = self._networks(which)
        return Predictor(list(nets) if ensemble else nets[index], self.cfg.num_classes, amp_dtype=self.cfg.amp_dtype, tta=tta,
                         device=self.device, window=window, stride=stride, blend=blend, window_batch=window_batch,
                         net_size=net_size, crf=crf, superpixels=superpixels, min_area=min_area, min_area_fill=min_area_fill,
                         connectivity=connectivity, region_ignore=region_ignore)(images, size=size, want_confidence=want_confidence)

    def _weighted(self, pred, target, weight):
        """the configured criterion with this step's class weights: the module's own parameters (ignore index 255, the focal
        alpha / gamma and its module form), only the weights come from outside"""
        crt = self.criterion
        if isinstance(crt, DiceLoss):
            return dice_loss(pred, target, crt.num_classes, weight=weight, ignore_index=crt.ignore_index)
        if isinstance(crt, FocalLoss):
            return FocalLoss(crt.num_classes, crt.alpha, crt.gamma, crt.ignore_index, crt.reduction, weight)(pred, target)
        if weight is None and nnf.dice_sums_supported(pred, pred.shape[1]):
            ce = nnf.dice_ce_sums(pred, target, crt.ignore_index)[2]     # the unweighted mean from the fused pass's CE sums
            return ce[:, 0].sum() / ce[:, 1].sum()
        return cross_entropy(pred, target, weight=weight, ignore_index=crt.ignore_index)

    def _ce_dice(self, pred, target):
        """0.5 * CE(ignore 255) + criterion (train_vqreptunet1x1v2.py:165-187); with the Dice criterion both terms come from
        one fused pass over the logits."""
        if isinstance(self.criterion, DiceLoss):
            return ce_dice_loss(pred, target, self.criterion.num_classes, 0.5, self.criterion.weight, self.criterion.ignore_index)
        return 0.5 * self.ce(pred, target) + self.criterion(pred, target)

    def supervised_step(self, l_input, l_target) -> torch.Tensor:
        """Plain supervised step of model 1 (Dice + 0.5 CE), for the single-model throughput figure."""
        m = self.models[0]
        self.buckets[0].zero()
        m.train()
        kw = dict(percent=80.0) if self.cfg.recipe == "v1" else dict(th=self.cfg.confidence_threshold)
        L = self.lanes
        L.fork(0)                                                       # inputs / zeroed buckets come from the caller's stream
        with L.on(0, self.cfg.amp_dtype):
            out = m(l_input, l_target, **kw)
        L.to_caller(*out)                                               # consumed on the caller's stream
        self._join()
        pred, closs, _u, ploss = out
        pred = pred.float()
        loss = self._ce_dice(pred, l_target) + closs.sum() + 0.01 * ploss.float()
        loss.backward()
        nnf.flush_pending_wgrads()
        L.join(0)                                                       # backward ran on network 1's stream
        self.buckets[0].finish()
        self.opts[0].step()
        return loss.detach()
