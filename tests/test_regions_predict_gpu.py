"""Predictor(min_area=...) and Predictor.instances on the GPU: the class map after the area filter equals the reference filter
(tests/region_cases.py) of the map the same Predictor gives without the option -- plain, dense-CRF and tiled mode -- the confidence is
untouched, the instance table is the reference table of the filtered map, and render / evaluate.test_loop see the filtered labels.
Exact integer equality throughout."""
import numpy as np
import pytest
import torch

from tests import predict_cases as P
from tests import region_cases as rc
from tests import slic_cases as sc
from tests import synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MIN_AREA = 6


def _images():
    """smooth images with pixel noise on top: the 1 x 1 stub's class maps are blobs with specks"""
    x = sc.smooth(77, 2, 64, 64)
    noise = np.random.default_rng(3).random(x.shape).astype(np.float32)
    return torch.from_numpy(np.clip(x + 0.5 * (noise - 0.5), 0.0, 1.0).astype(np.float32))


def _stub():
    return P.Stub(3, seed=4).to(DEV).eval()


@pytest.mark.parametrize("mode,conn,fill", [(dict(), 4, 0), (dict(), 8, "neighbour"), (dict(crf=2), 4, "neighbour"),
                                            (dict(window=32), 4, 2), (dict(tta=("none", "hflip")), 8, 0)],
                         ids=["plain-4-0", "plain-8-neighbour", "crf", "window", "two-views"])
def test_filtered_class_maps_equal_the_reference_filter(mode, conn, fill):
    """plain, refined (the dense CRF, two iterations: its kernels add in a fixed order, so two calls agree bit for bit), tiled, and two
    test-time views"""
    from vq_seg_amd.predict import Predictor
    from vq_seg_amd.utils.crf import DenseCRF
    x, stub = _images(), _stub()
    if "crf" in mode:
        mode = dict(crf=DenseCRF(iter_max=mode["crf"]))
    base = Predictor(stub, 3, device=DEV, **mode)(x, want_confidence=True)
    got = Predictor(stub, 3, device=DEV, min_area=MIN_AREA, min_area_fill=fill, connectivity=conn, **mode)(x, want_confidence=True)
    want = rc.remove_small(base.label.cpu().numpy(), MIN_AREA, conn, (), fill)
    assert got.label.dtype == torch.uint8 and np.array_equal(got.label.cpu().numpy(), want)
    changed = int((want != base.label.cpu().numpy()).sum())
    print(f"{mode} {conn} {fill}: the filter changed {changed} of {want.size} pixels")
    assert changed > 0                                          # min_area= is not ignored
    assert torch.equal(got.confidence, base.confidence)         # the network's top probability, also where the class changed


def test_superpixels_mode_is_filtered_too():
    """the pooled probabilities come from float atomics whose last bits differ between two calls, so this mode is not compared with a
    second call: with a constant fill of 0, every region of another class that is left has at least min_area pixels"""
    from vq_seg_amd.predict import Predictor
    x, stub = _images(), _stub()
    got = Predictor(stub, 3, device=DEV, superpixels=36, min_area=40, min_area_fill=0)(x).label.cpu().numpy()
    roots = rc.roots(got, 4, (0,))
    areas = rc.areas(roots)
    assert (got != 0).any() and int(areas[areas > 0].min()) >= 40
    plain = Predictor(stub, 3, device=DEV, superpixels=36)(x).label.cpu().numpy()
    small = rc.areas(rc.roots(plain, 4, (0,)))
    assert int(small[small > 0].min()) < 40                     # there was something to remove


def test_region_ignore_keeps_a_class_out_of_the_filter():
    from vq_seg_amd.predict import Predictor
    x, stub = _images(), _stub()
    base = Predictor(stub, 3, device=DEV)(x).label.cpu().numpy()
    got = Predictor(stub, 3, device=DEV, min_area=MIN_AREA, min_area_fill=0, region_ignore=(2,))(x).label.cpu().numpy()
    assert np.array_equal(got, rc.remove_small(base, MIN_AREA, 4, (2,), 0)) and np.array_equal(got == 2, base == 2)


@pytest.mark.parametrize("classes", [None, (1, 2), (2,)], ids=["all", "crop-weed", "weed"])
def test_instances_are_the_reference_table_of_the_filtered_map(classes):
    from vq_seg_amd.predict import Predictor
    x, stub = _images(), _stub()
    p = Predictor(stub, 3, device=DEV, min_area=MIN_AREA, connectivity=8)
    pred, plants = p.instances(x, classes=classes, capacity=512)
    label = pred.label.cpu().numpy()
    assert np.array_equal(label, p(x).label.cpu().numpy())
    ignore = () if classes is None else tuple(c for c in range(3) if c not in classes)
    roots = rc.roots(label, 8, ignore)
    ids, counts = rc.ids(roots)
    table, moments = rc.table(label, roots, ids, 512)
    assert 0 < int(counts.max()) <= 512
    assert np.array_equal(plants.count.cpu().numpy(), counts) and np.array_equal(plants.value.cpu().numpy(), table[..., 0])
    assert np.array_equal(plants.area.cpu().numpy(), table[..., 1]) and np.array_equal(plants.bbox.cpu().numpy(), table[..., 2:6])
    assert np.array_equal(plants.root.cpu().numpy(), table[..., 6])
    assert np.array_equal(plants.centroid.cpu().numpy(), moments.astype(np.float64) / np.maximum(table[..., 1], 1).astype(np.float64)[..., None])
    for k in range(label.shape[0]):
        n = int(counts[k])
        assert int(plants.area[k, :n].min()) >= MIN_AREA or classes is None      # (class 0 is the fill: its regions may be small only if they count)
        if classes is not None:
            assert set(plants.value[k, :n].tolist()) <= set(classes)


def test_render_trainer_surface_and_scoring_see_the_filtered_labels():
    from vq_seg_amd.evaluate import test_loop
    from vq_seg_amd.predict import Predictor, predict_batches
    from vq_seg_amd.utils.visualize import GAP, render_sheet
    x, stub = _images(), _stub()
    p = Predictor(stub, 3, device=DEV, min_area=MIN_AREA, min_area_fill="neighbour")
    label = p(x).label
    sheet = p.render(x)
    want = render_sheet(["image", "pred", ("fill", GAP), "mix_pred"], x.to(DEV), label, None, size=(64, 64), palette=None, alpha=0.4, half=False,
                        num_classes=3)
    assert sheet.dtype == torch.uint8 and torch.equal(sheet, want)
    assert not torch.equal(sheet, Predictor(stub, 3, device=DEV).render(x))
    (only,) = list(predict_batches(stub, [x], 3, device=DEV, min_area=MIN_AREA, min_area_fill="neighbour"))
    assert torch.equal(only.label, label)
    # scoring: min_area 1 removes nothing and gives the fused loop's numbers; a real threshold gives the filtered map's accuracy
    target = synth.blob_labels(22, 2, 64, cell=8)
    plain = test_loop(stub, [(x, target)], 3, device=DEV, fused=True)
    assert test_loop(stub, [(x, target)], 3, device=DEV, fused=True, min_area=1) == plain
    scored = test_loop(stub, [(x, target)], 3, device=DEV, fused=True, min_area=MIN_AREA, min_area_fill="neighbour")
    acc = (label.cpu() == target).double().mean(dim=(1, 2)).mean()
    assert scored["test_acc"] == float(acc) and scored != plain
