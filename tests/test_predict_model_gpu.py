"""The prediction path on real networks: Predictor and evaluate.test_loop(fused=True) on the small golden model (built as
tests/test_model_gpu.py builds it, masks 1.5 x the input), CPSTrainer.predict on a freshly initialised pair.  Every comparison is an
equality with the two-kernel path (upsample_bilinear, then softmax_stats / confusion counts / arg-max) on the same forward's logits."""
import functools

import pytest
import torch

from tests import cases, golden_io

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def golden_model():
    from tests.test_model_gpu import build
    fx = golden_io.load("model_v1")
    return build(fx.meta["name"], fx.meta["margin"], fx.meta["scale"], fx.meta["model_seed"])


@functools.lru_cache(maxsize=None)
def golden_batches():
    x, gt, _ = cases.model_inputs()
    tgt = torch.nn.functional.interpolate(gt[:, None].float(), scale_factor=1.5, mode="nearest")[:, 0].long()
    tgt[:, ::7, ::5] = 255                                   # ignored pixels among the classes
    assert all(len(torch.unique(t[t != 255])) == 3 for t in tgt)          # every class in every image: recall is finite
    return [(x, tgt), (x.flip(0), tgt.flip(0))]


def eval_logits(model, x, amp_dtype=None):
    was = model.training
    model.eval()
    with torch.no_grad():
        if amp_dtype is not None:
            with torch.autocast("cuda", dtype=amp_dtype):
                out = model(x)
        else:
            out = model(x)
    model.train(was)
    return out[0].float()


def test_predictor_on_the_golden_model_is_the_arg_max_of_the_resized_logits():
    from vq_seg_amd import nnf
    from vq_seg_amd.predict import Predictor
    model = golden_model()
    x, tgt = golden_batches()[0]
    size = tuple(tgt.shape[-2:])
    assert size == (96, 96)
    x = x.to(DEV)
    up = nnf.upsample_bilinear(eval_logits(model, x), size=size, align_corners=False)
    calls = nnf.RESIZE_ARGMAX_CALLS
    pred = Predictor(model, 3)(x, size=size, want_confidence=True)
    assert nnf.RESIZE_ARGMAX_CALLS == calls + 1
    assert pred.label.dtype == torch.uint8 and pred.label.shape == (2, 96, 96)
    assert torch.equal(pred.label.long(), up.argmax(dim=1))
    assert torch.equal(pred.confidence, nnf.softmax_stats(up, want_label=False, want_entropy=False, want_top=True)[2])
    own = Predictor(model, 3)(x)                            # size=None: the input's own
    assert own.label.shape == (2, 64, 64) and own.confidence is None
    assert torch.equal(own.label.long(), eval_logits(model, x).argmax(dim=1))


@pytest.mark.parametrize("amp", [None, torch.bfloat16], ids=["fp32", "bf16"])
def test_fused_test_loop_equals_the_unfused_loop_on_the_golden_model(amp):
    import numpy as np
    from vq_seg_amd import nnf
    from vq_seg_amd.evaluate import test_loop
    model = golden_model()
    plain = test_loop(model, golden_batches(), 3, device=DEV, amp_dtype=amp)
    calls = nnf.RESIZE_ARGMAX_CALLS
    fused = test_loop(model, golden_batches(), 3, device=DEV, amp_dtype=amp, fused=True)
    assert nnf.RESIZE_ARGMAX_CALLS == calls + 2               # one launch per batch
    assert fused == plain, (fused, plain)
    assert all(np.isfinite(v).all() for v in plain.values()) and 0.0 < plain["test_acc"] < 1.0


def _model():
    return {"name": "vqreptunet1x1", "params": {"encoder_name": "resnet50", "num_classes": 3, "depth": 5,
                                                "vq_cfg": {"num_embeddings": [0, 0, 64, 64, 64], "distance": "euclidean", "kmeans_init": True},
                                                "margin": 0.0, "scale": 1.0, "use_feature": False, "encoder_weights": None}}


@functools.lru_cache(maxsize=None)
def trainer():
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer
    return CPSTrainer(CPSConfig(model=_model(), recipe="v1", total_iters=8, amp_dtype=torch.bfloat16), DEV)


def two_kernel_path(acc):
    from vq_seg_amd import nnf
    label, _ent, top = nnf.softmax_stats(acc, want_label=True, want_entropy=False, want_top=True)
    return label.to(torch.uint8), top


def test_trainer_predict_ensemble_and_flipped_views():
    from vq_seg_amd import nnf
    from vq_seg_amd.trainer import SyntheticCropWeed
    tr = trainer()
    x, _lab = SyntheticCropWeed(64, 2, DEV, seed=9).labelled()
    size = (96, 80)
    modes = [m.training for m in tr.models]

    def up(model, img, unflip=()):
        """the view's logits, un-flipped at their own resolution (an exact permutation), then resized"""
        z = eval_logits(model, img.flip(unflip) if unflip else img, torch.bfloat16)
        return nnf.upsample_bilinear(z.flip(unflip) if unflip else z, size=size, align_corners=False)

    m1, m2 = tr.models
    single = tr.predict(x, size=size, index=1, want_confidence=True)
    assert all(torch.equal(a, b) for a, b in zip(single, two_kernel_path(up(m2, x))))
    both = tr.predict(x, size=size, ensemble=True, want_confidence=True)
    assert all(torch.equal(a, b) for a, b in zip(both, two_kernel_path((up(m1, x) + up(m2, x)) * 0.5)))
    flipped = tr.predict(x, size=size, tta=("none", "hflip"), want_confidence=True)
    assert all(torch.equal(a, b) for a, b in zip(flipped, two_kernel_path((up(m1, x) + up(m1, x, (-1,))) * 0.5)))
    four = tr.predict(x.cpu(), size=size, ensemble=True, tta=("vflip", "hvflip"))       # images on the host are moved to the trainer's device
    acc = ((up(m1, x, (-2,)) + up(m1, x, (-2, -1))) + up(m2, x, (-2,))) + up(m2, x, (-2, -1))
    assert torch.equal(four.label, two_kernel_path(acc * 0.25)[0]) and four.confidence is None
    assert [m.training for m in tr.models] == modes
    assert tr.predict(x).label.shape == (2, 64, 64)
    with pytest.raises(ValueError, match="needs a teacher"):
        tr.predict(x, which="teacher")
    with pytest.raises(ValueError, match="'student' or 'teacher'"):
        tr.predict(x, which="pupil")
    with pytest.raises(ValueError, match="1, 2 or 4"):
        tr.predict(x, tta=("none", "hflip", "vflip"))


def test_trainer_evaluate_passes_fused_through():
    from vq_seg_amd import nnf
    from vq_seg_amd.trainer import SyntheticCropWeed
    tr = trainer()
    data = SyntheticCropWeed(64, 2, DEV, seed=7, cell=8)                   # 64 cells per image: every class in every image
    batches = [data.labelled() for _ in range(2)]
    assert all(len(torch.unique(lab[i])) == 3 for _, lab in batches for i in range(lab.shape[0]))
    calls = nnf.RESIZE_ARGMAX_CALLS
    plain = tr.evaluate(batches)
    assert nnf.RESIZE_ARGMAX_CALLS == calls
    assert tr.evaluate(batches, fused=True) == plain and nnf.RESIZE_ARGMAX_CALLS == calls + 2
