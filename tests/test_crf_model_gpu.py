"""Dense-CRF refinement through the model-level surface: predict.Predictor(crf=...) against the composition it stands for, spelled
out with torch ops around nnf.dense_crf; evaluate.test_loop(fused=True, crf=...) against the Predictor's own labels; CPSTrainer's
evaluate / predict; and the untouched paths (`crf=None`)."""
import numpy as np
import pytest
import torch

from tests import crf_cases
from tests import predict_cases as P

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CUT = crf_cases.SETTINGS["cut"]


def images(n=2, h=24, w=40, seed=31):
    """blocky images (the CRF then moves labels), every image its own"""
    return torch.from_numpy(crf_cases.make_inputs(seed, n, 3, h, w)[0].copy())


def composition(models, flips, x, size, settings):
    """what Predictor(crf=...) stands for: resize each view's logits, un-flip, mean, softmax, dense CRF under the (resized) images,
    arg-max and top probability of the refined energies"""
    from vq_seg_amd import nnf
    x = x.to(DEV)
    acc = None
    with torch.no_grad():
        for m in models:
            for f in flips:
                z = m(x.flip(P.FLIP_DIMS[f]) if f else x)[0].float()
                if tuple(z.shape[-2:]) != tuple(size):
                    z = nnf.upsample_bilinear(z, size=tuple(size), align_corners=False)
                z = z.flip(P.FLIP_DIMS[f]) if f else z
                acc = z if acc is None else acc + z
        n_views = len(models) * len(flips)
        if n_views > 1:
            acc = acc * (1.0 / n_views)
        img = x if tuple(x.shape[-2:]) == tuple(size) else nnf.upsample_bilinear(x, size=tuple(size), align_corners=False)
        e = nnf.dense_crf(img, torch.softmax(acc, dim=1), out="logits", **settings)
    return e, e.argmax(dim=1), torch.softmax(e.double(), dim=1).amax(dim=1), acc


@pytest.mark.parametrize("size", [None, (30, 33)], ids=["own-size", "other-size"])
def test_predictor_with_crf_is_the_spelled_out_composition(size):
    from vq_seg_amd.predict import Predictor
    from vq_seg_amd.utils.crf import DenseCRF
    x = images()
    stub = P.Stub(3, seed=2, pool=2).to(DEV).eval()              # logits at half the images' size: the resize is exercised
    settings = dict(CUT, iter_max=3)
    pred = Predictor(stub, 3, device=DEV, crf=DenseCRF(**settings))(x, size=size, want_confidence=True)
    out = tuple(x.shape[-2:]) if size is None else size
    e, label, top, acc = composition([stub], [0], x, out, settings)
    assert pred.label.dtype == torch.uint8 and tuple(pred.label.shape) == (2,) + tuple(out)
    assert torch.equal(pred.label.long(), label)
    assert (pred.confidence.double() - top).abs().max() <= 1e-6
    assert (top - torch.softmax(acc.double(), dim=1).amax(dim=1)).abs().max() > 1e-3            # crf= is not ignored
    assert Predictor(stub, 3, device=DEV, crf=DenseCRF(**settings))(x, size=size).confidence is None


def test_ensemble_and_flipped_view_with_crf_and_the_defaults():
    from vq_seg_amd.predict import Predictor, predict_batches
    x = images(seed=32)
    stubs = [P.Stub(3, seed=3).to(DEV), P.Stub(3, seed=4).to(DEV)]
    pred = Predictor(stubs, 3, device=DEV, tta=("none", "hflip"), crf=True)(x, want_confidence=True)
    assert all(m.training for m in stubs)                        # modes restored
    for m in stubs:
        m.eval()
    defaults = dict(crf_cases.DEFAULTS, iter_max=10)
    e, label, top, _ = composition(stubs, [0, 1], x, tuple(x.shape[-2:]), defaults)
    assert torch.equal(pred.label.long(), label)
    assert (pred.confidence.double() - top).abs().max() <= 1e-6
    again = list(predict_batches(stubs, [x, (x, None)], 3, device=DEV, tta=("none", "hflip"), crf=True))
    assert len(again) == 2 and all(torch.equal(p.label, pred.label) for p in again)


def test_crf_with_window_raises_and_crf_none_is_todays_path():
    from vq_seg_amd import nnf
    from vq_seg_amd.predict import Predictor
    x = images(seed=33)
    stub = P.Stub(3, seed=5, pool=2).to(DEV)
    with pytest.raises(ValueError, match="not built"):
        Predictor(stub, 3, device=DEV, window=16, crf=True)
    pred = Predictor(stub, 3, device=DEV, tta=("none", "vflip"), crf=None)(x, size=(31, 29), want_confidence=True)
    stub.eval()
    with torch.no_grad():
        views = [stub(x.to(DEV))[0].float(), stub(x.to(DEV).flip(2))[0].float()]
    label, top, _ = nnf.resize_argmax(views, (31, 29), flips=[0, 2], want_top=True)
    assert torch.equal(pred.label, label) and torch.equal(pred.confidence, top)


def test_test_loop_with_crf_scores_the_predictors_labels():
    from vq_seg_amd.evaluate import test_loop
    from vq_seg_amd.measurement import Measurement
    from vq_seg_amd.predict import Predictor
    from vq_seg_amd.utils.crf import DenseCRF
    stub = P.Stub(3, seed=6, pool=2).to(DEV)
    crf = DenseCRF(iter_max=2, **CUT)
    batches = []
    for seed in (7, 8):
        t = torch.randint(0, 3, (2, 36, 44), generator=torch.Generator().manual_seed(seed))       # masks larger than the images
        t[:, ::5, ::3] = 255
        batches.append((images(seed=seed), t))
    out = test_loop(stub, batches, 3, device=DEV, fused=True, crf=crf)
    meas, miou, acc, ious = Measurement(3), 0.0, 0.0, np.zeros(3)
    for x, t in batches:
        label = Predictor(stub, 3, device=DEV, crf=crf)(x, size=(36, 44)).label
        conf = P.confusion(label, t, 3).numpy()
        m, per = meas.miou(conf)
        miou, ious = miou + float(m) / 2, ious + np.array(per) / 2
        acc += float((label.cpu().long() == t).flatten(1).double().mean(dim=1).mean()) / 2
    assert out["test_miou"] == pytest.approx(miou, abs=1e-12) and out["test_acc"] == pytest.approx(acc, abs=1e-12)
    assert out["test_ious"] == np.round(ious, 5).tolist()
    plain = test_loop(stub, batches, 3, device=DEV, fused=True)
    assert set(out) == set(plain)
    assert plain == test_loop(stub, batches, 3, device=DEV, fused=True, crf=None)
    with pytest.raises(ValueError, match="crf needs fused=True"):
        test_loop(stub, batches, 3, device=DEV, crf=crf)


def test_trainer_evaluate_and_predict_thread_crf():
    """one real vqreptunet1x1 through CPSTrainer.predict / evaluate with crf=: the trainer's result is the Predictor's"""
    from tests.test_predict_model_gpu import trainer
    from vq_seg_amd.predict import Predictor
    from vq_seg_amd.trainer import SyntheticCropWeed
    from vq_seg_amd.utils.crf import DenseCRF
    tr = trainer()
    x, lab = SyntheticCropWeed(64, 2, DEV, seed=12, cell=8).labelled()
    crf = DenseCRF(iter_max=2, **CUT)
    pred = tr.predict(x, crf=crf, want_confidence=True)
    want = Predictor(tr.models[0], tr.cfg.num_classes, amp_dtype=tr.cfg.amp_dtype, device=DEV, crf=crf)(x, want_confidence=True)
    assert torch.equal(pred.label, want.label) and torch.equal(pred.confidence, want.confidence)
    assert torch.equal(tr.predict(x).label, tr.predict(x, crf=None).label)
    scored = tr.evaluate([(x, lab)], fused=True, crf=crf)
    hits = float((pred.label.long() == lab).flatten(1).double().mean(dim=1).mean())
    assert scored["test_acc"] == pytest.approx(hits, abs=1e-12)
    with pytest.raises(ValueError, match="crf needs fused=True"):
        tr.evaluate([(x, lab)], crf=crf)
