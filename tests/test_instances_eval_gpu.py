"""evaluate.test_loop(fused=True, panoptic=...) and CPSTrainer.evaluate(panoptic=...) on the GPU, on the 1 x 1 stub network and the
batches of tests/test_boundary_eval_gpu.py: with panoptic=None the dict is what it was and no instance launch is made; with it, the new
keys equal an InstanceMeasurement fed with Predictor(...).label on the same batches through the CPU form -- plain and with min_area --
and the counts behind them equal the brute-force restatement of tests/instance_cases.py."""
import numpy as np
import pytest
import torch

from tests import instance_cases as ic
from tests.test_boundary_eval_gpu import DEV, MIN_AREA, _batches, _stub

pytestmark = pytest.mark.gpu

KEYS = ("test_pq", "test_sq", "test_rq", "test_pqs", "test_sqs", "test_rqs", "test_count_error", "test_panoptic_overflowed")


def _expected(model, batches, panoptic, amp_dtype=None, **mode):
    """(an InstanceMeasurement fed through the CPU form, the label maps)"""
    from vq_seg_amd.measurement import InstanceMeasurement
    from vq_seg_amd.predict import Predictor
    m = InstanceMeasurement(3, **({} if panoptic is True else panoptic))
    p = Predictor(model, 3, device=DEV, amp_dtype=amp_dtype, **mode)
    labels = []
    for img, target in batches:
        label = p(img.to(DEV), size=tuple(target.shape[-2:])).label.cpu()
        m.update(label, target.cpu())
        labels.append(label.numpy())
    return m, labels


def _same_keys(got, r):
    for key in ("pq", "sq", "rq"):
        assert np.array_equal(np.float64(got["test_" + key]), np.float64(r[key]), equal_nan=True), key
        assert np.array_equal(np.float64(got["test_" + key + "s"]), np.round(r[key + "s"], 5), equal_nan=True), key
    assert np.array_equal(np.float64(got["test_count_error"]), np.float64(r["count_error"]), equal_nan=True)
    assert got["test_panoptic_overflowed"] == r["overflowed"]


@pytest.mark.parametrize("mode", [dict(), dict(min_area=MIN_AREA, min_area_fill="neighbour")], ids=["plain", "min_area"])
@pytest.mark.parametrize("panoptic", [True, dict(things=(1, 2), void=(255,), connectivity=8, capacity=512)], ids=["defaults", "dict"])
def test_panoptic_keys_equal_the_measurement_on_the_predictors_labels(mode, panoptic):
    from vq_seg_amd import nnf
    from vq_seg_amd.evaluate import test_loop
    stub, batches = _stub(), _batches()
    before = nnf.INSTANCE_CALLS
    base = test_loop(stub, batches, 3, device=DEV, fused=True, **mode)
    assert nnf.INSTANCE_CALLS == before and not any(k in base for k in KEYS)
    assert test_loop(stub, batches, 3, device=DEV, fused=True, panoptic=None, **mode) == base and nnf.INSTANCE_CALLS == before
    got = test_loop(stub, batches, 3, device=DEV, fused=True, panoptic=panoptic, **mode)
    assert nnf.INSTANCE_CALLS == before + len(batches)
    assert {k: v for k, v in got.items() if k not in KEYS} == base and set(got) == set(base) | set(KEYS)
    m, labels = _expected(stub, batches, panoptic, **mode)
    assert nnf.INSTANCE_CALLS == before + len(batches)                          # the CPU form made no launch
    r = m.result()
    assert r["images"] == 4
    _same_keys(got, r)
    # the counts behind the keys are the restatement's on the same label maps
    conn, capacity = (4, 1024) if panoptic is True else (panoptic["connectivity"], panoptic["capacity"])
    tallies, ious, overs = [], [], []
    for label, (_img, target) in zip(labels, batches):
        pid, pc, ptab = ic.side(label, (1, 2), conn, capacity)
        gid, gc, gtab = ic.side(target.numpy(), (1, 2), conn, capacity)
        w = ic.match_from(pid, gid, target.numpy(), ptab, gtab, pc, gc, (255,), capacity, 3)
        tallies.append(w["tally"]), ious.append(w["iou_sum"]), overs.append(w["overflow"])
    want = ic.scores(np.concatenate(tallies), np.concatenate(ious), np.concatenate(overs), (1, 2))
    assert np.array_equal(r["table"], np.concatenate(tallies).astype(np.int64).sum(axis=0)) and int(r["table"][:, 3].sum()) > 0
    for key in ("pq", "sq", "rq", "count_error"):
        assert np.array_equal(np.float64(got["test_" + key]), np.float64(want[key]), equal_nan=True), key
    assert got["test_panoptic_overflowed"] == int(np.concatenate(overs).sum())


def test_an_overflowing_capacity_is_reported():
    from vq_seg_amd.evaluate import test_loop
    stub, batches = _stub(), _batches()
    got = test_loop(stub, batches, 3, device=DEV, fused=True, panoptic=dict(capacity=1))
    r = _expected(stub, batches, dict(capacity=1))[0].result()
    assert got["test_panoptic_overflowed"] == r["overflowed"] > 0
    _same_keys(got, r)


def test_trainer_evaluate_passes_panoptic_through():
    from tests.test_predict_model_gpu import trainer
    from vq_seg_amd import nnf
    from vq_seg_amd.evaluate import test_loop
    from vq_seg_amd.trainer import SyntheticCropWeed
    tr = trainer()
    data = SyntheticCropWeed(64, 2, DEV, seed=7, cell=8)
    batches = [data.labelled() for _ in range(2)]
    panoptic = dict(connectivity=8, capacity=2048)
    before = nnf.INSTANCE_CALLS
    plain = tr.evaluate(batches, fused=True)
    assert nnf.INSTANCE_CALLS == before and not any(k in plain for k in KEYS)
    got = tr.evaluate(batches, fused=True, panoptic=panoptic)
    assert nnf.INSTANCE_CALLS == before + 2
    again = test_loop(tr.models[0], batches, 3, device=DEV, amp_dtype=torch.bfloat16, fused=True, panoptic=panoptic)
    assert set(got) == set(again) and all(np.array_equal(np.float64(got[k]), np.float64(v), equal_nan=True) for k, v in again.items())
    assert {k: v for k, v in got.items() if k not in KEYS} == plain
    r = _expected(tr.models[0], batches, panoptic, amp_dtype=torch.bfloat16)[0].result()
    _same_keys(got, r)
    with pytest.raises(ValueError, match="panoptic needs fused=True"):
        tr.evaluate(batches, panoptic=True)
