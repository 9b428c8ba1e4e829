"""CPSConfig.superpixel_mean on the GPU (recipe v1, 64 x 64, batch 2 + 2, 64 codes, two steps, bf16 autocast, `keep_aux` -- the set-up
of tests/test_conf_ce_trainer_gpu.py): each network's fp32 training logits are averaged over SLIC superpixels of the batch they were
computed from before anything else sees them.  The label maps are utils.superpixel.slic of the inputs; the pooled predictions are
exactly constant within every superpixel and equal segment_mean64 (tests/slic_cases.py) of the unpooled logits to n_k * 2^-23 *
max|x|; `sup_loss_1` and `cps_loss`, restated in float64 from the pooled tensors and the masks, meet the 2e-6 relative bar of the fused
loss passes; both decoders learn.  With the option None no vqseg_slic* / vqseg_segment* entry point is launched and the step is
bit-identical to a trainer built without the new fields; with it, the Lab launch runs twice per step, once per batch."""
import functools

import numpy as np
import pytest
import torch

from tests import slic_cases as sc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
K = 36


def _model(recipe="v1"):
    name = "vqreptunet1x1" if recipe == "v1" else "vqreptunet1x1v2"
    return {"name": name, "params": {"encoder_name": "resnet50", "num_classes": 3, "depth": 5,
                                     "vq_cfg": {"num_embeddings": [0, 0, 64, 64, 64], "distance": "euclidean", "kmeans_init": True},
                                     "margin": 0.0, "scale": 1.0, "use_feature": False, "encoder_weights": None}}


def _trainer(recipe="v1", **kw):
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer
    return CPSTrainer(CPSConfig(model=_model(recipe), recipe=recipe, total_iters=8, amp_dtype=torch.bfloat16, keep_aux=True, **kw), DEV)


@functools.lru_cache(maxsize=None)
def _batches():
    from vq_seg_amd.trainer import SyntheticCropWeed
    lab, ul = SyntheticCropWeed(64, 2, DEV, seed=5), SyntheticCropWeed(64, 2, DEV, seed=6)
    return [(lab.labelled(), ul.unlabelled()) for _ in range(2)]


def _state(tr):
    torch.cuda.synchronize()
    return [t.detach().clone() for m in tr.models for t in m.state_dict().values()]


def _constant_per_segment(pred, seg):
    pred, seg = pred.cpu().numpy(), seg.cpu().numpy()
    for n in range(pred.shape[0]):
        flat, at = pred[n].reshape(pred.shape[1], -1), seg[n].reshape(-1)
        for s_ in np.unique(at):
            part = flat[:, at == s_]
            if not (part.max(axis=1) == part.min(axis=1)).all():
                return False
    return True


def test_pooled_predictions_restated_losses_and_learning():
    from vq_seg_amd.loss.dice_loss import dice_loss
    from vq_seg_amd.utils.superpixel import slic
    tr = _trainer(superpixel_mean=K)
    for step, ((l_in, l_tg), ul) in enumerate(_batches()):
        out = tr.step(l_in, l_tg, ul)
        torch.cuda.synchronize()
        aux = tr.aux
        assert all(bool(torch.isfinite(v).all()) for v in out.values()), out
        assert set(out) == {"loss", "sup_loss_1", "sup_loss_2", "cps_loss", "commitment_loss", "prototype_loss", "miou", "lr"}
        # the label maps: slic of the batches the training forwards received
        seg_l, seg_ul = aux["superpixels_l"], aux["superpixels_ul"]
        assert seg_l.dtype == torch.int32 and torch.equal(seg_l, slic(l_in, K)) and torch.equal(seg_ul, slic(ul, K))
        # the pooled predictions
        ps1, raw = aux["pred_sup_1"], aux["pred_sup_1_unpooled"]
        assert ps1.dtype == torch.float32 and _constant_per_segment(ps1, seg_l) and _constant_per_segment(aux["pred_ul_2"], seg_ul)
        want = sc.segment_mean64(raw.cpu().numpy(), seg_l.cpu().numpy(), K)[0]
        assert (np.abs(ps1.cpu().numpy() - want) <= sc.mean_bound(raw.cpu().numpy(), seg_l.cpu().numpy(), K)).all()
        assert not torch.equal(ps1, raw)
        b_l = l_tg.shape[0]
        assert torch.equal(aux["pred_1"][:b_l], ps1) and _constant_per_segment(aux["pred_1"][b_l:], seg_ul)
        # the terms, restated in float64 from the pooled tensors and the masks
        pred = {k: aux[f"pred_{k}"].cpu().double() for k in (1, 2)}
        mask = {k: aux[f"mask_{k}"].cpu() for k in (1, 2)}
        sup_1 = dice_loss(pred[1][:b_l], l_tg.cpu(), 3, ignore_index=255)
        cps = dice_loss(pred[1], mask[2], 3, ignore_index=255) + dice_loss(pred[2], mask[1], 3, ignore_index=255)
        for got, want, what in ((out["sup_loss_1"], sup_1, "sup_loss_1"), (out["cps_loss"], cps, "cps_loss")):
            err = abs(float(got) - float(want))
            print(f"step {step}: {what} {float(got):.9g} restated {float(want):.9g} err {err:.3e} bar {2e-6 * abs(float(want)):.3e}")
            assert err <= 2e-6 * abs(float(want)), what
        for m in tr.models:                                            # this step's gradients (zeroed when the next step begins)
            grads = [p.grad for p in m.decoder.parameters() if p.grad is not None]
            assert grads and any(bool(g.any()) for g in grads) and all(bool(torch.isfinite(g).all()) for g in grads)
    assert all(bool(torch.isfinite(t).all()) for t in _state(tr) if t.is_floating_point())


def test_recipe_v2_runs_on_pooled_logits():
    """confidence_threshold 0.4: averaging makes an untrained network's scores less confident still (largest pooled top probability
    of these 64 x 64 batches: 0.67 and 0.61), and at the default 0.7 network 1's score mask keeps 80 pixels in the first step and none
    in the second -- recipe v2's cross-entropy over zero kept pixels is then 0 / 0, with or without this option (measured: the plain
    step at threshold 0.999 gives the same NaN; the reference's CrossEntropyLoss does the same).  The masks are asserted non-empty so
    that the finiteness checked here is that of the pooled path."""
    tr = _trainer(recipe="v2", superpixel_mean=K, confidence_threshold=0.4)
    for (l_in, l_tg), ul in _batches():
        out = tr.step(l_in, l_tg, ul)
        torch.cuda.synchronize()
        assert all(bool((tr.aux[f"mask_{k}"] != 255).any()) for k in (1, 2))
        assert all(bool(torch.isfinite(v).all()) for v in out.values()), out
        assert _constant_per_segment(tr.aux["pred_sup_1"], tr.aux["superpixels_l"])
        assert _constant_per_segment(tr.aux["pred_ul_2"], tr.aux["superpixels_ul"])
    assert all(bool(torch.isfinite(t).all()) for t in _state(tr) if t.is_floating_point())


def test_option_off_launches_nothing_of_it_and_is_bit_identical(monkeypatch):
    from vq_seg_amd import nnf
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer
    names, real = [], nnf._launch
    monkeypatch.setattr(nnf, "_launch", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    runs = []
    for kw in (dict(), dict(superpixel_mean=None, superpixel_compactness=10.0, superpixel_iters=10)):
        tr = CPSTrainer(CPSConfig(model=_model(), recipe="v1", total_iters=8, amp_dtype=torch.bfloat16, keep_aux=True, **kw), DEV)
        outs = [{k: v.detach().clone() for k, v in tr.step(l_in, l_tg, ul).items()} for (l_in, l_tg), ul in _batches()]
        assert "superpixels_l" not in tr.aux and "pred_sup_1_unpooled" not in tr.aux
        runs.append((outs, _state(tr)))
    assert names and not [n for n in names if n.startswith(("vqseg_slic", "vqseg_segment"))]
    (oa, sa), (ob, sb) = runs
    for x, y in zip(oa, ob):
        assert all(torch.equal(x[k], y[k]) for k in x)
    assert len(sa) == len(sb) and all(torch.equal(x, y) for x, y in zip(sa, sb))
    names.clear()
    tr = _trainer(superpixel_mean=K)
    (l_in, l_tg), ul = _batches()[0]
    tr.step(l_in, l_tg, ul)
    assert names.count("vqseg_slic_lab_f") == 2             # the labelled and the unlabelled batch, once each -- not once per forward
    assert names.count("vqseg_segment_sums_f") == 8         # four pooled tensors forward, four gradients backward
