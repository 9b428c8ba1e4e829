"""CPSConfig.unsup_criterion = "conf_ce" on the GPU (recipe v1, 64 x 64, batch 2 + 2, 64 codes, two steps -- the set-up of
tests/test_balanced_trainer_gpu.py): the step's CPS term is the masked criterion on the labelled half plus uw * conf_ce_loss on the
unlabelled logits, restated in float64 from the step's own tensors (`keep_aux`); the unreliable weights are loss.unreliable_weight
of those logits; parameters stay finite and both decoders receive gradient.  With the option None no conf_ce entry point is
launched and the step is bit-identical to a trainer built without the new fields.

Bar of the restated term: 2e-6 relative, the forward bar of the fused loss passes (tests/test_conf_ce_kernel_gpu.py).  The step's
logits are what they are, not margin-clean: a pixel within a float32 rounding of a threshold would move a sum by a whole term.  The
test prints M and Mn of both directions, so that such a failure can be read for what it is."""
import functools

import pytest
import torch

from tests import conf_ce_cases as cc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
OPTION = dict(unsup_criterion="conf_ce", conf_ce_threshold_neg=0.1)


def _model():
    return {"name": "vqreptunet1x1", "params": {"encoder_name": "resnet50", "num_classes": 3, "depth": 5,
                                                "vq_cfg": {"num_embeddings": [0, 0, 64, 64, 64], "distance": "euclidean", "kmeans_init": True},
                                                "margin": 0.0, "scale": 1.0, "use_feature": False, "encoder_weights": None}}


def _trainer(**kw):
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer
    return CPSTrainer(CPSConfig(model=_model(), recipe="v1", total_iters=8, amp_dtype=torch.bfloat16, keep_aux=True, **kw), DEV)


@functools.lru_cache(maxsize=None)
def _batches():
    from vq_seg_amd.trainer import SyntheticCropWeed
    lab, ul = SyntheticCropWeed(64, 2, DEV, seed=5), SyntheticCropWeed(64, 2, DEV, seed=6)
    return [(lab.labelled(), ul.unlabelled()) for _ in range(2)]


def _state(tr):
    torch.cuda.synchronize()
    return [t.detach().clone() for m in tr.models for t in m.state_dict().values()]


def test_cps_term_is_the_restated_sum_and_both_decoders_learn():
    from vq_seg_amd.loss import unreliable_weight
    from vq_seg_amd.loss.dice_loss import dice_loss
    tr = _trainer(**OPTION)
    cfg = tr.cfg
    par = (cfg.conf_ce_threshold, cfg.conf_ce_threshold_neg, cfg.conf_ce_temperature)
    for step, ((l_in, l_tg), ul) in enumerate(_batches()):
        out = tr.step(l_in, l_tg, ul)
        torch.cuda.synchronize()
        aux = tr.aux
        assert all(bool(torch.isfinite(v).all()) for v in out.values()), out
        b_l = l_tg.shape[0]
        pu = {k: aux[f"pred_ul_{k}"].cpu() for k in (1, 2)}
        ps = {k: aux[f"pred_sup_{k}"].cpu().double() for k in (1, 2)}
        mask = {k: aux[f"mask_{k}"].cpu() for k in (1, 2)}
        assert pu[1].dtype == torch.float32 and mask[1].shape[0] == 2 * b_l
        percent = 100 - cfg.unsup_loss_drop_percent                    # epoch_frac = 0
        for k in (1, 2):                                               # uw_k: of network k's logits; it weighs the OTHER network's term
            assert torch.equal(aux[f"uw_{k}"], unreliable_weight(aux[f"pred_ul_{k}"], percent))
            want = cc.unreliable_weight64(pu[k], percent)              # (the entropies differ in their last bit: a few pixels may swap sides)
            assert abs(float(aux[f"uw_{k}"]) - want) <= 2e-3 * want, (k, float(aux[f"uw_{k}"]), want)
        parts_1, parts_2 = {}, {}
        c_1, c_2 = cc.restate(pu[1], pu[2], *par, parts=parts_1), cc.restate(pu[2], pu[1], *par, parts=parts_2)
        print(f"step {step}: M {parts_1['m']} / {parts_2['m']}, Mn {parts_1['mn']} / {parts_2['mn']} of {pu[1].numel() // 3} pixels; "
              f"conf_ce {float(c_1):.6g} / {float(c_2):.6g}, uw {float(aux['uw_1']):.6g} / {float(aux['uw_2']):.6g}")
        for got, want, what in ((aux["conf_ce_1"], c_1, "conf_ce_1"), (aux["conf_ce_2"], c_2, "conf_ce_2")):
            assert abs(float(got) - float(want)) <= 2e-6 * abs(float(want)), (what, float(got), float(want))
        want = (dice_loss(ps[1], mask[2][:b_l], 3, ignore_index=255) + float(aux["uw_2"]) * c_1
                + dice_loss(ps[2], mask[1][:b_l], 3, ignore_index=255) + float(aux["uw_1"]) * c_2)
        err = abs(float(out["cps_loss"]) - float(want))
        print(f"step {step}: cps_loss {float(out['cps_loss']):.9g} restated {float(want):.9g} err {err:.3e} bar {2e-6 * abs(float(want)):.3e}")
        assert err <= 2e-6 * abs(float(want))
        total = float(out["sup_loss_1"]) + float(out["sup_loss_2"]) + float(out["cps_loss"]) + float(out["commitment_loss"]) + float(out["prototype_loss"])
        assert abs(float(out["loss"]) - total) <= 1e-5 * abs(total)
        for m in tr.models:                                            # this step's gradients (zeroed when the next step begins)
            grads = [p.grad for p in m.decoder.parameters() if p.grad is not None]
            assert grads and any(bool(g.any()) for g in grads) and all(bool(torch.isfinite(g).all()) for g in grads)
    assert all(bool(torch.isfinite(t).all()) for t in _state(tr) if t.is_floating_point())


def test_gradient_crosses_the_networks_unless_the_targets_are_detached():
    """the unlabelled logits of network 2 receive gradient from network 1's term (the path through the weight); detached, they do not"""
    from vq_seg_amd import nnf
    a = torch.randn(2, 3, 64, 64, device=DEV)
    b = torch.randn(2, 3, 64, 64, device=DEV).requires_grad_(True)
    for detach in (False, True):
        l_ab, _l_ba = nnf.conf_ce_pair(a, b, 0.4, 0.1, 1.0, detach)
        (g_b,) = torch.autograd.grad(l_ab, b, allow_unused=True)
        assert bool(g_b.any()) != detach


def test_option_off_launches_nothing_of_it_and_is_bit_identical(monkeypatch):
    from vq_seg_amd import nnf
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer
    names, real = [], nnf._launch
    monkeypatch.setattr(nnf, "_launch", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    runs = []
    for kw in (dict(), dict(unsup_criterion=None, conf_ce_threshold=0.6, conf_ce_threshold_neg=0.0, conf_ce_temperature=1.0,
                            conf_ce_unreliable_weight=True, conf_ce_detach_targets=False)):
        tr = CPSTrainer(CPSConfig(model=_model(), recipe="v1", total_iters=8, amp_dtype=torch.bfloat16, keep_aux=True, **kw), DEV)
        outs = [{k: v.detach().clone() for k, v in tr.step(l_in, l_tg, ul).items()} for (l_in, l_tg), ul in _batches()]
        assert "conf_ce_1" not in tr.aux and "uw_1" not in tr.aux
        runs.append((outs, _state(tr)))
    assert names and not [n for n in names if n.startswith("vqseg_conf_ce")]
    (oa, sa), (ob, sb) = runs
    for x, y in zip(oa, ob):
        assert all(torch.equal(x[k], y[k]) for k in x)
    assert len(sa) == len(sb) and all(torch.equal(x, y) for x, y in zip(sa, sb))
    names.clear()
    tr = _trainer(**OPTION)
    (l_in, l_tg), ul = _batches()[0]
    tr.step(l_in, l_tg, ul)
    assert names.count("vqseg_conf_ce_forward_f") == 1 and names.count("vqseg_conf_ce_backward_f") == 1      # both directions, one launch each way
