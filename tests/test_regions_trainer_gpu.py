"""CPSConfig.pseudo_min_area on the GPU (64 x 64, batch 2 + 2, 64 codes, bf16 autocast, `keep_aux` -- the set-up of
tests/test_superpixel_trainer_gpu.py): in the mask each network hands to the other, a connected region of one class smaller than the
threshold becomes 255.  `mask_k` equals the reference filter (tests/region_cases.py) of `mask_k_unfiltered` exactly, in both recipes;
with the option None the step launches nothing of it, never enters nnf.filter_regions and is bit-identical to a trainer built without
the new fields."""
import functools

import numpy as np
import pytest
import torch

from tests import region_cases as rc
from tests.test_superpixel_trainer_gpu import _model, _state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MIN_AREA = 8


def _trainer(recipe="v1", **kw):
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer
    return CPSTrainer(CPSConfig(model=_model(recipe), recipe=recipe, total_iters=8, amp_dtype=torch.bfloat16, keep_aux=True, **kw), DEV)


@functools.lru_cache(maxsize=None)
def _batch():
    from vq_seg_amd.trainer import SyntheticCropWeed
    lab, ul = SyntheticCropWeed(64, 2, DEV, seed=5), SyntheticCropWeed(64, 2, DEV, seed=6)
    return lab.labelled(), ul.unlabelled()


@pytest.mark.parametrize("recipe,conn,kw", [("v1", 4, {}), ("v2", 8, dict(confidence_threshold=0.4))], ids=["v1-4", "v2-8"])
def test_masks_are_the_reference_filter_of_the_unfiltered_masks(recipe, conn, kw):
    tr = _trainer(recipe, pseudo_min_area=MIN_AREA, pseudo_connectivity=conn, **kw)
    (l_in, l_tg), ul = _batch()
    out = tr.step(l_in, l_tg, ul)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in out.values()), out
    assert "_unfiltered" not in tr.aux
    for k in (1, 2):
        mask, raw = tr.aux[f"mask_{k}"], tr.aux[f"mask_{k}_unfiltered"]
        assert mask.dtype == raw.dtype and tuple(mask.shape) == (4, 64, 64)
        want = rc.remove_small(raw.cpu().numpy(), MIN_AREA, conn, (255,), 255)
        changed = int((want != raw.cpu().numpy()).sum())
        print(f"{recipe} mask_{k}: {changed} of {want.size} pixels became 255")
        assert np.array_equal(mask.cpu().numpy(), want)
        assert changed > 0                                      # an untrained network's masks have specks: the option is not ignored
        assert bool((mask != 255).any())


def test_option_off_launches_nothing_of_it_and_is_bit_identical(monkeypatch):
    from vq_seg_amd import nnf
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer

    def never(*a, **k):
        raise AssertionError("nnf.filter_regions was entered with pseudo_min_area None")
    names, real = [], nnf._launch
    monkeypatch.setattr(nnf, "_launch", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    monkeypatch.setattr(nnf, "filter_regions", never)
    (l_in, l_tg), ul = _batch()
    runs = []
    for kw in (dict(), dict(pseudo_min_area=None, pseudo_connectivity=8)):
        tr = CPSTrainer(CPSConfig(model=_model(), recipe="v1", total_iters=8, amp_dtype=torch.bfloat16, keep_aux=True, **kw), DEV)
        out = {k: v.detach().clone() for k, v in tr.step(l_in, l_tg, ul).items()}
        assert "mask_1_unfiltered" not in tr.aux and "mask_2_unfiltered" not in tr.aux
        runs.append((out, _state(tr)))
    assert names and not [n for n in names if n.startswith("vqseg_region_") and n != "vqseg_region_graph_f"]
    (oa, sa), (ob, sb) = runs
    assert all(torch.equal(oa[k], ob[k]) for k in oa)
    assert len(sa) == len(sb) and all(torch.equal(x, y) for x, y in zip(sa, sb))
    monkeypatch.undo()
    names.clear()
    monkeypatch.setattr(nnf, "_launch", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    _trainer(pseudo_min_area=MIN_AREA).step(l_in, l_tg, ul)
    assert sum(n.startswith("vqseg_region_roots_") for n in names) == 2 and sum(n.startswith("vqseg_region_filter_") for n in names) == 2
