"""Panoptic quality on the CPU: the restatement of tests/instance_cases.py against an independent dense IoU matrix from
scipy.ndimage.label, the torch-op form of vq_seg_amd.utils.instances against the restatement on every case (exact integers, float64
scores equal), the entry forms, InstanceMeasurement over two updates, and the argument checks that need no device."""
import numpy as np
import pytest
import torch

from tests import instance_cases as ic
from vq_seg_amd import _hip, nnf
from vq_seg_amd.utils import instances

TABLES = ("match", "inter", "union", "void", "matched", "tally", "overflow")


def test_no_case_overflows_but_the_overflow_cases():
    for name in ic.NAMES:
        _things, _void, capacity, overflows = ic.settings(name)
        for conn in (4, 8):
            ref = ic.reference(name, conn)
            assert bool(ref["overflow"].any()) == overflows, (name, conn)
            if not overflows:
                assert int(ref["pred_count"].max()) <= capacity and int(ref["gt_count"].max()) <= capacity, (name, conn)
    ref = ic.reference("lattice-exact", 4)
    assert int(ref["gt_count"][0]) == ic.settings("lattice-exact")[2] == 561 and int(ref["gt_id"].max()) == 560       # ids cross 255 / 256 and 511 / 512
    assert int(ic.reference("lattice-gt-over", 4)["gt_count"][0]) == ic.settings("lattice-gt-over")[2] + 1
    assert int(ic.reference("lattice-pred-over", 4)["pred_count"][0]) == ic.settings("lattice-pred-over")[2] + 1
    over = ic.reference("batch-lattice-over", 8)
    whole = ic.reference("batch-lattice", 8)
    assert over["overflow"].tolist() == [0, 1, 0] and int(over["tally"][1].sum()) == 0 and float(over["iou_sum"][1].sum()) == 0.0
    for k in (0, 2):                                          # the neighbours of the overflowed image are not disturbed
        assert np.array_equal(over["tally"][k], whole["tally"][k]) and np.array_equal(over["iou_sum"][k], whole["iou_sum"][k])
        assert np.array_equal(over["match"][k], whole["match"][k, :719])


def test_the_cases_hold_what_they_are_named_for():
    t = lambda name: ic.reference(name, 4)["tally"][0].tolist()
    assert t("exact-half") == [[0] * 5, [0, 1, 1, 1, 1], [1, 0, 0, 1, 1]]          # 2 * inter == union: no match; one pixel above: a match
    ref = ic.reference("exact-half", 4)
    assert ref["inter"][0, :2].tolist() == [0, 201] and ref["union"][0, :2].tolist() == [0, 401]
    assert t("split2")[1] == [1, 1, 0, 2, 1] and t("split3")[1] == [0, 3, 1, 3, 1] and t("merged")[1] == [1, 0, 1, 1, 2]
    assert t("wrong-class") == [[0] * 5, [0, 0, 1, 0, 1], [1, 1, 0, 2, 1]]
    assert t("mostly-void")[1] == [0, 2, 0, 3, 0] and ic.reference("mostly-void", 4)["void"][0, :3].tolist() == [60, 50, 30]
    assert t("void-trim") == [[0] * 5, [1, 0, 0, 1, 1], [0, 1, 1, 1, 1]] and ic.reference("void-trim", 4)["union"][0, 0] == 100
    nothing = ic.reference("nothing-33x65", 8)
    assert int(nothing["tally"].sum()) == 0 and all(np.isnan(nothing["scores"][k]) for k in ("pq", "sq", "rq"))
    assert t("things2-67x131")[1] == [0] * 5 and sum(t("things2-67x131")[2]) > 0 and sum(t("things012-33x65")[0]) > 0
    assert int(ic.reference("checkerboard-33x65", 4)["gt_count"][0]) > 1000 and int(ic.reference("checkerboard-33x65", 8)["gt_count"][0]) == 1


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", ["shift1-33x65", "shift3-67x131", "void-trim", "mostly-void", "lattice-exact", "things012-33x65", "batch"])
def test_restatement_equals_a_dense_iou_matrix_from_scipy(name, conn):
    ndimage = pytest.importorskip("scipy.ndimage")
    ref = ic.reference(name, conn)
    things, void, capacity, _over = ic.settings(name)
    structure = np.ones((3, 3), dtype=int) if conn == 8 else None

    def label(v):
        """(ids in first-pixel order, value per id): scipy labels per class, renumbered by rising first pixel over all classes"""
        parts = []
        for c in things:
            lab, n = ndimage.label(v == c, structure=structure)
            for k in range(1, n + 1):
                mask = lab == k
                parts.append((int(np.flatnonzero(mask)[0]), c, mask))
        parts.sort(key=lambda x: x[0])
        ids = np.full(v.shape, -1, dtype=np.int64)
        for k, (_first, _c, mask) in enumerate(parts):
            ids[mask] = k
        return ids, [c for _first, c, _mask in parts]

    for k in range(ref["pred"].shape[0]):
        p, t = ref["pred"][k], ref["target"][k]
        pid, pv = label(p)
        gid, gv = label(t)
        assert np.array_equal(pid, ref["pred_id"][k]) and np.array_equal(gid, ref["gt_id"][k])
        is_void = np.isin(t, void)
        tp = fn = 0
        want_match = np.full(capacity, -1)
        for g in range(len(gv)):
            partners = []
            for q in range(len(pv)):
                inter = int(((gid == g) & (pid == q)).sum())
                union = int(((pid == q) & ~is_void).sum()) + int((gid == g).sum()) - inter
                if pv[q] == gv[g] and inter / union > 0.5:
                    partners.append(q)
            assert len(partners) <= 1
            if partners:
                want_match[g], tp = partners[0], tp + 1
            else:
                fn += 1
        assert np.array_equal(want_match, ref["match"][k])
        assert tp == int(ref["tally"][k, :, 0].sum()) and fn == int(ref["tally"][k, :, 2].sum())


def _check(got_stats, got_match, ref, things):
    for key in TABLES:
        g = {"tally": got_stats.table, "overflow": got_stats.overflow}.get(key)
        g = getattr(got_match, key) if g is None else g
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        assert g.dtype == np.int32 and np.array_equal(g, ref[key]), f"{key} differs"
    iou = got_stats.iou_sum
    iou = iou.cpu().numpy() if torch.is_tensor(iou) else iou
    assert iou.dtype == np.float64 and np.array_equal(iou, ref["iou_sum"])
    for key in ("pq", "sq", "rq", "count_error"):
        assert np.array_equal(np.float64(getattr(got_stats, key)), np.float64(ref["scores"][key]), equal_nan=True), key
    for side, rid, rcount, rtab in ((got_match.pred, "pred_id", "pred_count", "pred_table"), (got_match.target, "gt_id", "gt_count", "gt_table")):
        assert np.array_equal(np.asarray(side.count.cpu() if torch.is_tensor(side.count) else side.count), ref[rcount])
        assert np.array_equal(np.asarray(side.area.cpu() if torch.is_tensor(side.area) else side.area), ref[rtab][..., 1])
        assert np.array_equal(np.asarray(side.value.cpu() if torch.is_tensor(side.value) else side.value), ref[rtab][..., 0])


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", ic.NAMES)
def test_torch_form_equals_the_restatement(name, conn):
    ref = ic.reference(name, conn)
    things, void, capacity, _over = ic.settings(name)
    p, t = torch.from_numpy(ref["pred"].copy()), torch.from_numpy(ref["target"].copy())
    kw = dict(things=things, void=void, connectivity=conn, capacity=capacity)
    _check(instances.panoptic_stats(p, t, ic.NUM_CLASSES, **kw), instances.match_regions(p, t, ic.NUM_CLASSES, **kw), ref, things)


def test_numpy_single_map_and_int64_entry_forms():
    ref = ic.reference("batch", 8)
    things, void, capacity, _over = ic.settings("batch")
    kw = dict(void=void, connectivity=8, capacity=capacity)
    pred, target = ref["pred"].copy(), ref["target"].copy()
    s = instances.panoptic_stats(pred, target, ic.NUM_CLASSES, **kw)
    m = instances.match_regions(pred, target, ic.NUM_CLASSES, **kw)
    assert isinstance(s.table, np.ndarray) and isinstance(m.match, np.ndarray) and isinstance(m.pred.area, np.ndarray)
    _check(s, m, ref, things)
    p64, t64 = torch.from_numpy(pred).long(), torch.from_numpy(target).long()
    _check(instances.panoptic_stats(p64, t64, ic.NUM_CLASSES, **kw), instances.match_regions(p64, t64, ic.NUM_CLASSES, **kw), ref, things)
    one = instances.panoptic_stats(pred[0], target[0], ic.NUM_CLASSES, **kw)                               # (H, W): no batch axis comes back
    assert one.table.shape == (ic.NUM_CLASSES, 5) and one.overflow.shape == () and np.array_equal(one.table, ref["tally"][0])
    assert np.array_equal(one.iou_sum, ref["iou_sum"][0])
    alone = ic.scores(ref["tally"][:1], ref["iou_sum"][:1], ref["overflow"][:1], things)
    assert 0 < alone["pq"] < 1 and one.pq == alone["pq"] and instances.panoptic_quality(pred[0], target[0], ic.NUM_CLASSES, **kw) == alone["pq"]


def test_measurement_over_two_updates_equals_one_call_on_the_concatenation():
    from vq_seg_amd import measurement
    assert measurement.InstanceMeasurement is instances.InstanceMeasurement
    ref = ic.reference("batch", 4)
    things, void, capacity, _over = ic.settings("batch")
    meas = instances.InstanceMeasurement(ic.NUM_CLASSES, void=void, connectivity=4, capacity=capacity)
    assert np.isnan(meas.result()["pq"]) and meas.result()["images"] == 0
    meas.update(ref["pred"][:1].copy(), ref["target"][:1].copy())
    meas.update(torch.from_numpy(ref["pred"][1:].copy()), torch.from_numpy(ref["target"][1:].copy()))
    r = meas.result()
    want = ref["scores"]
    for key in ("pq", "sq", "rq", "count_error"):
        assert r[key] == want[key], key
    for key in ("pqs", "sqs", "rqs", "count_errors"):
        assert np.array_equal(r[key], want[key], equal_nan=True), key
    assert r["images"] == 3 and r["overflowed"] == 0 and np.array_equal(r["table"], ref["tally"].astype(np.int64).sum(axis=0))
    over = instances.InstanceMeasurement(ic.NUM_CLASSES, capacity=719)
    ref = ic.reference("batch-lattice-over", 4)
    over.update(ref["pred"].copy(), ref["target"].copy())
    r = over.result()
    assert r["overflowed"] == 1 and r["images"] == 3 and r["pq"] == ref["scores"]["pq"] and r["count_error"] == ref["scores"]["count_error"]


def test_argument_validation():
    p = np.zeros((4, 4), dtype=np.uint8)
    bad = [
        (dict(num_classes=0), "num_classes must be an integer in 1..255"),
        (dict(num_classes=256), "num_classes must be an integer in 1..255"),
        (dict(things=(3,)), "things must be distinct classes in 0..2"),
        (dict(things=(1, 1)), "things must be distinct classes"),
        (dict(void=(1,)), "a void value cannot be a thing class"),
        (dict(void=(1, 2, 3, 4, 5)), "0 to 4 integers"),
        (dict(connectivity=6), "connectivity must be 4 or 8"),
        (dict(capacity=0), "capacity must be an integer in 1..65535"),
        (dict(capacity=65536), "capacity must be an integer in 1..65535"),
        (dict(capacity=True), "capacity must be an integer in 1..65535"),
    ]
    for kw, msg in bad:
        kw = dict(dict(num_classes=3), **kw)
        with pytest.raises(ValueError, match=msg):
            instances.panoptic_stats(p, p, **kw)
        with pytest.raises(ValueError, match=msg):
            instances.InstanceMeasurement(**kw)
    with pytest.raises(ValueError, match="one shape"):
        instances.match_regions(p, np.zeros((4, 5), dtype=np.uint8), 3)
    with pytest.raises(ValueError, match="two numpy arrays or two tensors"):
        instances.match_regions(p, torch.zeros(4, 4, dtype=torch.uint8), 3)
    with pytest.raises(ValueError, match="an integer map"):
        instances.match_regions(p.astype(np.float32), p, 3)
    assert not nnf.instance_supported(torch.zeros(1, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint8))


def test_nnf_checks_arguments_before_it_touches_a_device():
    """types, shapes and sizes first; a CPU tensor with everything else right reaches the library's device error"""
    E = _hip.HipLibraryError
    b, h, w, cap = 2, 5, 7, 8
    ids = torch.zeros(b, h, w, dtype=torch.int32)
    target = torch.zeros(b, h, w, dtype=torch.uint8)
    table = torch.zeros(b, cap, 8, dtype=torch.int32)
    rows = torch.zeros(b, cap, dtype=torch.int32)
    counts = torch.zeros(b, dtype=torch.int32)
    before = nnf.INSTANCE_CALLS
    with pytest.raises(E, match="pred_ids must be int32"):
        nnf.instance_overlap(ids.long(), ids, target, table, table)
    with pytest.raises(E, match="gt_ids must have the values' shape"):
        nnf.instance_overlap(ids, ids[:, :4], target, table, table)
    with pytest.raises(E, match="values must be uint8 or int32 or int64"):
        nnf.instance_overlap(ids, ids, target.to(torch.int16), table, table)
    with pytest.raises(E, match=r"pred_table must be a int32 tensor \(2, 8, 8\)"):
        nnf.instance_overlap(ids, ids, target, table[:, :4], table)
    with pytest.raises(ValueError, match="capacity must be an integer in 1..65535"):
        nnf.instance_overlap(ids, ids, target, table, table, capacity=0)
    with pytest.raises(ValueError, match="0 to 4 integers"):
        nnf.instance_overlap(ids, ids, target, table, table, void=(1, 2, 3, 4, 5))
    with pytest.raises(E, match="no CPU fallback"):
        nnf.instance_overlap(ids, ids, target, table, table)
    with pytest.raises(ValueError, match="num_classes must be an integer in 1..255"):
        nnf.instance_tally(rows, rows, rows, table, table, counts, counts, 256)
    with pytest.raises(E, match=r"inter must be a int32 tensor \(2, 8\)"):
        nnf.instance_tally(rows, rows.long(), rows, table, table, counts, counts, 3)
    with pytest.raises(E, match=r"gt_counts must be an int32 tensor \(2,\)"):
        nnf.instance_tally(rows, rows, rows, table, table, counts, counts[:1], 3)
    with pytest.raises(E, match="no CPU fallback"):
        nnf.instance_tally(rows, rows, rows, table, table, counts, counts, 3)
    assert nnf.INSTANCE_CALLS == before
    L = _hip.lib()
    assert [L.vqseg_instance_vote_bits(c) for c in (0, 1, 2, 3, 4, 1023, 1024, 65535, 65536)] == [0, 1, 2, 2, 3, 10, 11, 16, 0]
    assert L.vqseg_instance_vote_i32(None, None, None, 1, 1, 4, 4, 8, 1, 255, 0, 0, 0, None, None, None) == -1 and b"null" in L.vqseg_last_error()
    assert L.vqseg_instance_overlap_i32(None, None, None, None, 1, 4, 4, 8, None, None, None) == -1
    assert L.vqseg_instance_match_i32(None, None, None, None, None, None, 1, 8, None, None, None, None, None) == -1
    assert L.vqseg_instance_tally_i32(None, None, None, None, None, None, None, None, None, 1, 8, 3, None, None, None, None) == -1


def test_test_loop_and_evaluate_check_panoptic_without_a_device():
    from vq_seg_amd.evaluate import test_loop
    model = torch.nn.Conv2d(3, 3, 1)
    with pytest.raises(ValueError, match="panoptic needs fused=True"):
        test_loop(model, [], 3, panoptic=True)
    with pytest.raises(ValueError, match="panoptic is None, True or a dict of things, void, connectivity and capacity"):
        test_loop(model, [], 3, fused=True, panoptic=dict(tolerance=2))
    with pytest.raises(ValueError, match="panoptic is None, True or a dict"):
        test_loop(model, [], 3, fused=True, panoptic=1)
    with pytest.raises(ValueError, match="capacity must be an integer in 1..65535"):
        test_loop(model, [], 3, fused=True, panoptic=dict(capacity=0))
    with pytest.raises(ValueError, match="a void value cannot be a thing class"):
        test_loop(model, [], 3, fused=True, panoptic=dict(void=(2,)))
    import inspect
    from vq_seg_amd.trainer import CPSTrainer
    assert inspect.signature(CPSTrainer.evaluate).parameters["panoptic"].default is None
    assert inspect.signature(test_loop).parameters["panoptic"].default is None
