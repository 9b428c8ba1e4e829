"""evaluate.test_loop(fused=True, boundary=...) on the GPU, on the 1 x 1 stub network and the noisy smooth images of
tests/test_regions_predict_gpu.py: with boundary=None the dict is what it was and no boundary launch is made; with it, the new keys
equal a BoundaryMeasurement fed with Predictor(...).label on the same batches -- plain, with min_area, tiled and with two views -- and
the counts behind them equal the plain restatement of tests/boundary_cases.py."""
import numpy as np
import pytest
import torch

from tests import boundary_cases as bc
from tests import predict_cases as P
from tests import slic_cases as sc
from tests import synth

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MIN_AREA = 6
KEYS = ("test_boundary_f1", "test_boundary_f1s", "test_boundary_iou", "test_boundary_ious", "test_hausdorff")


def _batches():
    """two batches of two images; a stripe of 255 in the second target: ignored pixels are not counted"""
    out = []
    for seed in (77, 78):
        x = sc.smooth(seed, 2, 64, 64)
        noise = np.random.default_rng(seed - 74).random(x.shape).astype(np.float32)
        img = torch.from_numpy(np.clip(x + 0.5 * (noise - 0.5), 0.0, 1.0).astype(np.float32))
        target = synth.blob_labels(seed - 55, 2, 64, cell=8).clone()
        if seed == 78:
            target[:, 20:24] = 255
        out.append((img, target))
    return out


def _stub():
    return P.Stub(3, seed=4).to(DEV).eval()


def _expected(stub, batches, boundary, **mode):
    from vq_seg_amd.measurement import BoundaryMeasurement
    from vq_seg_amd.predict import Predictor
    m = BoundaryMeasurement(3, **({} if boundary is True else boundary))
    p = Predictor(stub, 3, device=DEV, **mode)
    labels = []
    for img, target in batches:
        label = p(img, size=None if "window" in mode else tuple(target.shape[-2:])).label
        m.update(label, target.to(DEV))
        labels.append(label.cpu().numpy())
    return m, labels


@pytest.mark.parametrize("mode", [dict(), dict(min_area=MIN_AREA, min_area_fill="neighbour"), dict(window=32), dict(tta=("none", "hflip"))],
                         ids=["plain", "min_area", "window", "two-views"])
@pytest.mark.parametrize("boundary", [True, dict(tolerance=3.5, width=1, ignore=(255,))], ids=["defaults", "dict"])
def test_boundary_keys_equal_the_measurement_on_the_predictors_labels(mode, boundary):
    from vq_seg_amd import nnf
    from vq_seg_amd.evaluate import test_loop
    stub, batches = _stub(), _batches()
    before = nnf.BOUNDARY_CALLS
    base = test_loop(stub, batches, 3, device=DEV, fused=True, **mode)
    assert nnf.BOUNDARY_CALLS == before and not any(k in base for k in KEYS)
    assert test_loop(stub, batches, 3, device=DEV, fused=True, boundary=None, **mode) == base and nnf.BOUNDARY_CALLS == before
    got = test_loop(stub, batches, 3, device=DEV, fused=True, boundary=boundary, **mode)
    assert nnf.BOUNDARY_CALLS == before + len(batches)
    assert {k: v for k, v in got.items() if k not in KEYS} == base                # the region scores are what they were
    m, labels = _expected(stub, batches, boundary, **mode)
    r = m.result()
    assert r["images"] == 4
    assert got["test_boundary_f1"] == r["boundary_f1"] and got["test_boundary_iou"] == r["boundary_iou"] and got["test_hausdorff"] == r["hausdorff"]
    assert got["test_boundary_f1s"] == np.round(r["boundary_f1s"], 5).tolist() and got["test_boundary_ious"] == np.round(r["boundary_ious"], 5).tolist()
    assert 0.0 < got["test_boundary_f1"] < 1.0 and 0.0 < got["test_boundary_iou"] < 1.0 and got["test_hausdorff"] > 0.0
    # the counts behind the keys are the restatement's on the same label maps
    tol, width = (2.0, 2.0) if boundary is True else (boundary["tolerance"], boundary["width"])
    want = np.concatenate([bc.counts(label, target.numpy(), 3, bc.squared(tol), bc.squared(width), (255,)) for label, (_, target) in zip(labels, batches)])
    assert np.array_equal(m.table(), want)
    mean, per = bc.nanmean_classes(bc.scores(want)["f1"])
    assert got["test_boundary_f1"] == pytest.approx(mean, rel=1e-15)

