"""CPSConfig.criterion / class_weight on the GPU (recipe v1, 64 x 64, batch 2 + 2, 64 codes, two steps): every arm's loss terms are
the torch-op criteria in fp64 on the step's own logits and masks (`keep_aux`), all terms are finite and the parameters move; with
the new fields at their defaults the step is bit-identical to a trainer built without them and still takes the one-launch
combination.

Bar of the restated terms: 2e-6 relative, the bar the fused loss passes are held to (tests/test_focal_gpu.py).  The step
comparisons of tests/test_cutmix_trainer_gpu.py are bit-equalities between two runs of the same float32 code; a float32 kernel
against a float64 restatement cannot be held to that, the defaults-off arm below is."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ARMS = {"balanced_dice": dict(criterion="dice_loss", class_weight="balanced"),
        "focal": dict(criterion="focal_loss"),
        "balanced_focal": dict(criterion="focal_loss", class_weight="balanced"),
        "balanced_ce": dict(criterion="cross_entropy", class_weight="balanced"),
        "fixed_focal": dict(criterion="focal_loss", class_weight=[0.5, 0.8, 1.0], focal_gamma=3.0)}


def _model():
    return {"name": "vqreptunet1x1", "params": {"encoder_name": "resnet50", "num_classes": 3, "depth": 5,
                                                "vq_cfg": {"num_embeddings": [0, 0, 64, 64, 64], "distance": "euclidean", "kmeans_init": True},
                                                "margin": 0.0, "scale": 1.0, "use_feature": False, "encoder_weights": None}}


def _trainer(**kw):
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer
    return CPSTrainer(CPSConfig(model=_model(), recipe="v1", total_iters=8, amp_dtype=torch.bfloat16, keep_aux=True, **kw), torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def _batches():
    from vq_seg_amd.trainer import SyntheticCropWeed
    dev = torch.device("cuda:0")
    lab, ul = SyntheticCropWeed(64, 2, dev, seed=5), SyntheticCropWeed(64, 2, dev, seed=6)
    return [(lab.labelled(), ul.unlabelled()) for _ in range(2)]


def _state(tr):
    torch.cuda.synchronize()
    return [t.detach().clone() for m in tr.models for t in m.state_dict().values()]


def _restated(kw, aux, l_target):
    """the four terms with torch ops in fp64 from the step's own logits and masks"""
    from vq_seg_amd.loss import compute_class_weight
    from vq_seg_amd.loss.dice_loss import dice_loss
    from vq_seg_amd.loss.focal_loss import _focal_torch
    cw = kw.get("class_weight")
    w = compute_class_weight(3, l_target.cpu())[:3].double() if cw == "balanced" else torch.tensor(cw, dtype=torch.float64) if cw else None
    if cw is not None:
        assert torch.equal(aux["class_weight"].cpu().double(), w.float().double())

    def crit(pred, target):
        pred, target = pred.cpu().double(), target.cpu()
        if kw["criterion"] == "dice_loss":
            return dice_loss(pred, target, 3, weight=w, ignore_index=255)
        if kw["criterion"] == "cross_entropy":
            return F.cross_entropy(pred, target, weight=w, ignore_index=255)
        return _focal_torch(torch.softmax(pred, 1), target, 0.25, kw.get("focal_gamma", 2.0), 3, 255, "mean", w)       # the module form

    b = l_target.shape[0]
    return {"sup_loss_1": crit(aux["pred_1"][:b], l_target), "sup_loss_2": crit(aux["pred_2"][:b], l_target),
            "cps_loss": crit(aux["pred_1"], aux["mask_2"]) + crit(aux["pred_2"], aux["mask_1"])}


@pytest.mark.parametrize("arm", sorted(ARMS))
def test_arm_terms_are_the_torch_op_criteria_on_the_steps_own_logits(arm):
    kw = ARMS[arm]
    tr = _trainer(**kw)
    before = _state(tr)
    for (l_in, l_tg), ul in _batches():
        out = tr.step(l_in, l_tg, ul)
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(v).all()) for v in out.values()), out
        want = _restated(kw, tr.aux, l_tg)
        for k, v in want.items():
            err = abs(float(out[k]) - float(v))
            print(f"{arm} {k}: step {float(out[k]):.9g} restated {float(v):.9g} err {err:.3e} bar {2e-6 * abs(float(v)):.3e}")
            assert err <= 2e-6 * abs(float(v)), (arm, k)
        total = float(out["sup_loss_1"]) + float(out["sup_loss_2"]) + float(out["cps_loss"]) + float(out["commitment_loss"]) + float(out["prototype_loss"])
        assert abs(float(out["loss"]) - total) <= 1e-5 * abs(total)
    after = _state(tr)
    moved = [not torch.equal(a, b) for a, b in zip(before, after) if a.is_floating_point()]
    assert sum(moved) > 0.9 * len(moved)


def test_defaults_are_bit_identical_and_keep_the_one_launch_combine(monkeypatch):
    from vq_seg_amd import nnf
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer
    calls, real = [], nnf.cps_loss_combine

    def spy(*a, **k):
        r = real(*a, **k)
        calls.append(r is not None)
        return r

    monkeypatch.setattr(nnf, "cps_loss_combine", spy)
    runs = []
    for kw in (dict(), dict(criterion="dice_loss", class_weight=None, focal_alpha=0.25, focal_gamma=2.0)):
        tr = CPSTrainer(CPSConfig(model=_model(), recipe="v1", total_iters=8, amp_dtype=torch.bfloat16, keep_aux=True, **kw), torch.device("cuda:0"))
        outs = [{k: v.detach().clone() for k, v in tr.step(l_in, l_tg, ul).items()} for (l_in, l_tg), ul in _batches()]
        assert "pred_1" not in tr.aux and "class_weight" not in tr.aux
        runs.append((outs, _state(tr)))
    assert calls == [True] * 4                                             # the one-launch combination, every step of both trainers
    (oa, sa), (ob, sb) = runs
    for x, y in zip(oa, ob):
        assert all(torch.equal(x[k], y[k]) for k in x)
    assert len(sa) == len(sb) and all(torch.equal(x, y) for x, y in zip(sa, sb))
