"""CPSConfig.hard_aug = "photometric" on the GPU: with all probabilities 0 the step is the plain one bit for bit (and the kernel did run);
off is off; with the defaults the step distorts the clean unlabelled batch with the documented rows, and nothing upstream of the
unlabelled training forwards moves; CutMix mixes the distorted images with the boxes it had; the step stays deterministic,
stream-independent and resumable; SLIC sees the batch the training forwards receive.  The harness of tests/test_easy_aug_trainer_gpu.py:
64 x 64 images, 32 codes, two steps, both recipes."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

RECIPES = ["v1", "v2"]
ZERO = dict(hard_aug_jitter_p=0.0, hard_aug_gray_p=0.0, hard_aug_blur_p=0.0)


def _model(recipe):
    name = "vqreptunet1x1" if recipe == "v1" else "vqreptunet1x1v2"
    return {"name": name, "params": {"encoder_name": "resnet50", "num_classes": 3, "depth": 5,
                                     "vq_cfg": {"num_embeddings": [0, 0, 32, 32, 32], "distance": "euclidean", "kmeans_init": True},
                                     "margin": 0.0, "scale": 1.0, "use_feature": False, "encoder_weights": None}}


def _trainer(recipe, hard, cutmix=None, two_streams=True, **extra):
    """hard: None = hard_aug off, "zero" = on with all probabilities 0, "on" = the defaults"""
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer
    kw = {} if hard is None else dict(hard_aug="photometric", **(ZERO if hard == "zero" else {}))
    cfg = CPSConfig(model=_model(recipe), recipe=recipe, total_iters=8, amp_dtype=torch.bfloat16, two_streams=two_streams, keep_aux=True,
                    cutmix_ratio=cutmix, seed=42, **kw, **extra)
    return CPSTrainer(cfg, torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def _batches():
    from vq_seg_amd.trainer import SyntheticCropWeed
    dev = torch.device("cuda:0")
    lab = SyntheticCropWeed(64, 2, dev, seed=5)
    ul = SyntheticCropWeed(64, 2, dev, seed=6)
    return [(lab.labelled(), ul.unlabelled()) for _ in range(2)]


def _state(tr):
    torch.cuda.synchronize()
    return [t.detach().clone() for m in tr.models for t in m.state_dict().values()]      # parameters, BatchNorm buffers, codebooks


def _steps(tr, batches):
    from vq_seg_amd import _hip
    outs, auxes, calls = [], [], []
    for (l_in, l_tg), ul in batches:
        before = _hip.PHOTOMETRIC_CALLS
        outs.append({k: v.detach().clone() for k, v in tr.step(l_in, l_tg, ul).items()})
        calls.append(_hip.PHOTOMETRIC_CALLS - before)
        auxes.append({k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in tr.aux.items()})
    return outs, auxes, _state(tr), calls


@functools.lru_cache(maxsize=None)
def _run(recipe, hard, cutmix=None, two_streams=True):
    """computed once, shared by the tests below, never modified"""
    return _steps(_trainer(recipe, hard, cutmix, two_streams), _batches())


def _same(a, b):
    (oa, sa), (ob, sb) = (a[0], a[2]), (b[0], b[2])
    for i, (x, y) in enumerate(zip(oa, ob)):
        diff = {k: (float(x[k]), float(y[k])) for k in x if not torch.equal(x[k], y[k])}
        assert not diff, (i, diff)
    assert len(sa) == len(sb) and all(torch.equal(x, y) for x, y in zip(sa, sb))


@pytest.mark.parametrize("recipe", RECIPES)
def test_all_probabilities_zero_is_the_plain_step_and_off_is_off(recipe):
    from vq_seg_amd.data import IDENTITY_PHOTOMETRIC
    on, off = _run(recipe, "zero"), _run(recipe, None)
    assert on[3] == [1, 1] and off[3] == [0, 0]                               # the kernel ran once per step; off: no call is made
    for aux in off[1]:
        assert "ul_photometric" not in aux and "photometric_params" not in aux
    for it, aux in enumerate(on[1]):
        assert aux["photometric_params"] == [IDENTITY_PHOTOMETRIC] * 2
        ul = _batches()[it][1].contiguous(memory_format=torch.channels_last)
        assert torch.equal(aux["ul_photometric"].view(torch.int32), ul.view(torch.int32))
    for k in ("score_1", "score_2", "mask_1", "mask_2", "pred_sup_1", "pred_ul_2"):
        assert torch.equal(on[1][1][k], off[1][1][k])
    _same(on, off)


@pytest.mark.parametrize("recipe", RECIPES)
def test_defaults_distort_the_clean_batch_and_nothing_upstream(recipe):
    from vq_seg_amd.data import augmentations as A
    on, off = _run(recipe, "on"), _run(recipe, None)
    assert on[3] == [1, 1]
    for it, (out, aux) in enumerate(zip(on[0], on[1])):
        assert all(bool(torch.isfinite(v).all()) for v in out.values())
        rows = A.step_photometric(2, 42, 0, it, "sample", **A.PHOTOMETRIC_DEFAULTS)      # the documented draw: (seed, rank, iteration)
        assert aux["photometric_params"] == rows and isinstance(aux["photometric_params"], list)
        ul = _batches()[it][1].contiguous(memory_format=torch.channels_last)
        assert aux["ul_photometric"].is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(aux["ul_photometric"], A.photometric(ul, rows))
        assert "ul_mixed" not in aux
    assert any(r != A.IDENTITY_PHOTOMETRIC for aux in on[1] for r in aux["photometric_params"])      # something was distorted
    assert not torch.equal(on[1][0]["ul_photometric"], _batches()[0][1])
    for k in ("score_1", "score_2", "pred_sup_1"):                              # the pseudo-label forwards and the labelled forward of step 0
        assert torch.equal(on[1][0][k], off[1][0][k])
    print({k: (float(on[0][0][k]), float(off[0][0][k])) for k in ("loss", "cps_loss", "prototype_loss")})
    assert not torch.equal(on[0][0]["loss"], off[0][0]["loss"])                 # the unlabelled training forwards saw other images
    assert torch.equal(on[0][0]["lr"], off[0][0]["lr"])


@pytest.mark.parametrize("recipe", RECIPES)
def test_cutmix_mixes_the_distorted_images_with_its_own_boxes(recipe):
    from vq_seg_amd.data import augmentations as A
    both, only_mix = _run(recipe, "on", 0.25), _run(recipe, None, 0.25)
    assert both[3] == [1, 1]
    for it in range(2):
        a, b = both[1][it], only_mix[1][it]
        assert a["boxes"] == b["boxes"]                                         # the photometric rows draw from a key of their own
        assert torch.equal(a["ul_photometric"], _run(recipe, "on")[1][it]["ul_photometric"])      # the same clean batch, the same rows
        assert torch.equal(a["ul_mixed"], A.mix_boxes(a["ul_photometric"], a["boxes"]))
        assert a["photometric_params"] == A.step_photometric(2, 42, 0, it, "sample")
    for k in ("score_1_mixed", "score_2_mixed"):                                # step 0: the score maps are mixed, never distorted
        assert torch.equal(both[1][0][k], only_mix[1][0][k])


@pytest.mark.parametrize("recipe", RECIPES)
def test_same_seed_same_steps_on_one_stream_or_two(recipe):
    first = _run(recipe, "on", 0.25)
    _same(first, _steps(_trainer(recipe, "on", 0.25), _batches()))                            # a second trainer, same seed
    _same(first, _steps(_trainer(recipe, "on", 0.25, two_streams=False), _batches()))         # one stream == two streams


@pytest.mark.parametrize("recipe", RECIPES)
def test_resume_after_the_first_step_is_bit_exact(recipe, tmp_path):
    whole = _run(recipe, "on")
    batches = _batches()
    a = _trainer(recipe, "on")
    _steps(a, batches[:1])
    path = str(tmp_path / "ck.pth")
    a.save_checkpoint(path)
    b = _trainer(recipe, "on")
    b.load_checkpoint(path)
    assert b.iter == 1
    outs, auxes, state, _c = _steps(b, batches[1:])
    assert auxes[0]["photometric_params"] == whole[1][1]["photometric_params"]   # from the iteration counter
    _same((outs, None, state), (whole[0][1:], None, whole[2]))


def test_superpixels_are_those_of_the_distorted_batch():
    """_superpixels' contract: SLIC of the batch as the training forwards receive it"""
    from vq_seg_amd.utils.superpixel import slic
    tr = _trainer("v1", "on", superpixel_mean=36)
    (l_in, l_tg), ul = _batches()[0]
    tr.step(l_in, l_tg, ul)
    torch.cuda.synchronize()
    aux = tr.aux
    assert aux["photometric_params"][0] != aux["photometric_params"][1]
    assert torch.equal(aux["superpixels_ul"], slic(aux["ul_photometric"].float(), 36))
    assert torch.equal(aux["superpixels_l"], slic(l_in, 36))
    assert not torch.equal(aux["superpixels_ul"], slic(ul, 36))                 # the distortion shows in the map
