"""CPSConfig.feature_perturb on the GPU (64 x 64, batch 2 + 2, 64 codes, two steps -- the set-up and the pattern of
tests/test_conf_ce_trainer_gpu.py), both recipes: network k's CPS term gains feature_perturb_weight * crit(pred_fp_k, the other's mask of
the unlabelled batch); `fp_loss` (the two unweighted terms) and `cps_loss` are restated in float64 from the step's own tensors
(`keep_aux`) within 2e-6 relative, that test's bar for restated terms; the keep tables are nnf.channel_keep of the documented key
(cfg.seed, 2 * rank + k, iteration); two trainers with one seed agree bit for bit; every encoder and decoder learns.  With the
option None no vqseg_channel_* entry point is launched and the steps are bit-identical to a trainer built without the new fields."""
import functools

import pytest
import torch

from vq_seg_amd import nnf

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ENC = (64, 256, 512, 1024, 2048)                             # the decoder inputs' channels, shallow to deep (resnet50)


def _model(recipe):
    return {"name": "vqreptunet1x1" if recipe == "v1" else "vqreptunet1x1v2",
            "params": {"encoder_name": "resnet50", "num_classes": 3, "depth": 5,
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


def _crit64(recipe, pred, target):
    """the recipe's criterion in float64: Dice (v1), 0.5 CE + Dice (v2: train_vqreptunet1x1v2.py:165-187)"""
    from vq_seg_amd.loss.dice_loss import dice_loss
    d = dice_loss(pred, target, 3, ignore_index=255)
    if recipe == "v1":
        return d
    return 0.5 * torch.nn.functional.cross_entropy(pred, target, ignore_index=255) + d


@pytest.mark.parametrize("recipe", ["v1", "v2"])
def test_terms_are_the_restated_sums_and_every_network_learns(recipe):
    tr = _trainer(recipe, feature_perturb=0.5)
    w = tr.cfg.feature_perturb_weight
    assert w == 0.5
    tables = []
    for step, ((l_in, l_tg), ul) in enumerate(_batches()):
        out = tr.step(l_in, l_tg, ul)
        torch.cuda.synchronize()
        aux = tr.aux
        assert all(bool(torch.isfinite(v).all()) for v in out.values()), out
        b_l = l_tg.shape[0]
        ps = {k: aux[f"pred_sup_{k}"].cpu().double() for k in (1, 2)}
        pu = {k: aux[f"pred_ul_{k}"].cpu().double() for k in (1, 2)}
        pf = {k: aux[f"pred_fp_{k}"].cpu().double() for k in (1, 2)}
        mask = {k: aux[f"mask_{k}"].cpu() for k in (1, 2)}
        assert aux["pred_fp_1"].dtype == torch.float32 and pf[1].shape == pu[1].shape == (b_l, 3, 64, 64) and mask[1].shape[0] == 2 * b_l
        assert not torch.equal(pf[1], pu[1]) and not torch.equal(pf[2], pu[2])
        fp = {k: _crit64(recipe, pf[k], mask[3 - k][b_l:]) for k in (1, 2)}
        want_fp = fp[1] + fp[2]
        err = abs(float(out["fp_loss"]) - float(want_fp))
        print(f"{recipe} step {step}: fp_loss {float(out['fp_loss']):.9g} restated {float(want_fp):.9g} err {err:.3e} bar {2e-6 * abs(float(want_fp)):.3e}")
        assert err <= 2e-6 * abs(float(want_fp))
        want = sum(_crit64(recipe, torch.cat([ps[k], pu[k]]), mask[3 - k]) + w * fp[k] for k in (1, 2))
        err = abs(float(out["cps_loss"]) - float(want))
        print(f"{recipe} step {step}: cps_loss {float(out['cps_loss']):.9g} restated {float(want):.9g} err {err:.3e} bar {2e-6 * abs(float(want)):.3e}")
        assert err <= 2e-6 * abs(float(want))
        total = float(out["sup_loss_1"]) + float(out["sup_loss_2"]) + float(out["cps_loss"]) + float(out["commitment_loss"]) + float(out["prototype_loss"])
        assert abs(float(out["loss"]) - total) <= 1e-5 * abs(total)
        # the keep tables: the documented key (cfg.seed, 2 * rank + k, iteration), all five levels of B = 2 images in one table
        for k in (0, 1):
            want_t, _ = nnf.channel_keep([(b_l, c) for c in ENC], 0.5, tr.cfg.seed, k, step, DEV)
            got = aux[f"perturb_scale_{k + 1}"]
            assert got.shape == (b_l * sum(ENC),) and torch.equal(got, want_t), (k, step)
            assert torch.equal(got.cpu(), nnf.channel_keep([(b_l, c) for c in ENC], 0.5, tr.cfg.seed, k, step, "cpu")[0])
        assert not torch.equal(aux["perturb_scale_1"], aux["perturb_scale_2"])
        tables.append(aux["perturb_scale_1"].clone())
        for m in tr.models:                                            # this step's gradients (zeroed when the next step begins)
            for part in (m.encoder, m.decoder):
                grads = [p.grad for p in part.parameters() if p.grad is not None]
                assert grads and any(bool(g.any()) for g in grads) and all(bool(torch.isfinite(g).all()) for g in grads)
    assert not torch.equal(tables[0], tables[1])
    assert all(bool(torch.isfinite(t).all()) for t in _state(tr) if t.is_floating_point())


def test_two_trainers_with_one_seed_agree_bit_for_bit():
    (l_in, l_tg), ul = _batches()[0]
    runs = []
    for _ in range(2):
        tr = _trainer(feature_perturb=0.5)
        tr.step(l_in, l_tg, ul)
        torch.cuda.synchronize()
        runs.append({k: tr.aux[k].clone() for k in ("perturb_scale_1", "perturb_scale_2", "pred_fp_1", "pred_fp_2")})
    for k, v in runs[0].items():
        assert torch.equal(v, runs[1][k]), k


def test_option_off_launches_nothing_of_it_and_is_bit_identical(monkeypatch):
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer
    names, real = [], nnf._launch
    monkeypatch.setattr(nnf, "_launch", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    runs = []
    for kw in (dict(), dict(feature_perturb=None, feature_perturb_weight=0.5)):
        tr = CPSTrainer(CPSConfig(model=_model("v1"), recipe="v1", total_iters=8, amp_dtype=torch.bfloat16, keep_aux=True, **kw), DEV)
        outs = [{k: v.detach().clone() for k, v in tr.step(l_in, l_tg, ul).items()} for (l_in, l_tg), ul in _batches()]
        assert "pred_fp_1" not in tr.aux and "perturb_scale_1" not in tr.aux and "fp_loss" not in outs[0]
        runs.append((outs, _state(tr)))
    assert names and not [n for n in names if n.startswith("vqseg_channel_")]
    (oa, sa), (ob, sb) = runs
    for x, y in zip(oa, ob):
        assert all(torch.equal(x[k], y[k]) for k in x)
    assert len(sa) == len(sb) and all(torch.equal(x, y) for x, y in zip(sa, sb))
    names.clear()
    tr = _trainer(feature_perturb=0.5)
    for (l_in, l_tg), ul in _batches():
        names.clear()
        tr.step(l_in, l_tg, ul)
        # per step: one draw per network, and the forward and the backward pass of five levels of two networks
        assert names.count("vqseg_channel_keep_f") == 2
        assert names.count("vqseg_channel_dropout_cat_f") == 5 * 2 and names.count("vqseg_channel_dropout_fold_f") == 5 * 2
