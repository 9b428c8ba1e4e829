"""The instance kernels (csrc/instance_kernels.hip) against the brute-force restatement of tests/instance_cases.py: match, inter, union,
void, matched, the tally, iou_sum and the overflow flag on every case, for both connectivities and both element types -- exact equality,
nothing has a tolerance.  Then what equality on one call cannot show: two calls, an image alone against the image in its batch, the
guard bands of tests/extent.py around every entry point, and id maps with entries that are no ids."""
import numpy as np
import pytest
import torch

from tests import extent as E
from tests import instance_cases as ic
from vq_seg_amd import _hip, nnf
from vq_seg_amd.utils import instances

pytestmark = pytest.mark.gpu

DTYPES = {"u8": torch.uint8, "i32": torch.int32}
KEYS = ("match", "inter", "union", "void", "matched", "tally", "iou_sum", "overflow")


def dev():
    return torch.device("cuda:0")


def same(t, want):
    return np.array_equal(t.cpu().numpy(), want)


def everything(p, t, name, conn):
    things, void, capacity, _over = ic.settings(name)
    kw = dict(things=things, void=void, connectivity=conn, capacity=capacity)
    m = instances.match_regions(p, t, ic.NUM_CLASSES, **kw)
    s = instances.panoptic_stats(p, t, ic.NUM_CLASSES, **kw)
    out = dict(match=m.match, inter=m.inter, union=m.union, void=m.void, matched=m.matched, overflow=m.overflow, tally=s.table, iou_sum=s.iou_sum,
               pred_count=m.pred.count, gt_count=m.target.count, pred_area=m.pred.area, gt_area=m.target.area)
    return out, s


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", ic.NAMES)
def test_kernels_equal_the_restatement(name, conn, dtype):
    ref = ic.reference(name, conn)
    p = torch.from_numpy(ref["pred"].copy()).to(DTYPES[dtype]).to(dev())
    t = torch.from_numpy(ref["target"].copy()).to(DTYPES[dtype]).to(dev())
    assert nnf.instance_supported(p, t)
    before = nnf.INSTANCE_CALLS
    got, stats = everything(p, t, name, conn)
    assert nnf.INSTANCE_CALLS == before + 2
    for key in KEYS:
        assert got[key].is_cuda and got[key].dtype == (torch.float64 if key == "iou_sum" else torch.int32), key
        assert same(got[key], ref[key]), f"{key} differs: {int((got[key].cpu().numpy() != ref[key]).sum())} entries"
    assert same(got["pred_count"], ref["pred_count"]) and same(got["gt_count"], ref["gt_count"])
    assert same(got["pred_area"], ref["pred_table"][..., 1]) and same(got["gt_area"], ref["gt_table"][..., 1])
    for key in ("pq", "sq", "rq", "count_error"):
        assert np.array_equal(np.float64(getattr(stats, key)), np.float64(ref["scores"][key]), equal_nan=True), key


def test_int64_maps_and_the_public_surface_take_the_kernels():
    ref = ic.reference("batch", 8)
    things, void, capacity, _over = ic.settings("batch")
    p, t = torch.from_numpy(ref["pred"].copy()).long().to(dev()), torch.from_numpy(ref["target"].copy()).long().to(dev())
    before = nnf.INSTANCE_CALLS
    meas = instances.InstanceMeasurement(ic.NUM_CLASSES, void=void, connectivity=8, capacity=capacity)
    meas.update(p, t)
    assert nnf.INSTANCE_CALLS == before + 1
    r = meas.result()
    assert r["pq"] == ref["scores"]["pq"] and r["sq"] == ref["scores"]["sq"] and r["rq"] == ref["scores"]["rq"]
    assert np.array_equal(r["table"], ref["tally"].astype(np.int64).sum(axis=0))
    assert instances.panoptic_quality(p, t, ic.NUM_CLASSES, void=void, connectivity=8, capacity=capacity) == ref["scores"]["pq"]
    assert nnf.INSTANCE_CALLS == before + 2
    # an element type the kernels do not take: the torch-op form on the device, the same numbers, no kernel call
    s16 = instances.panoptic_stats(p.to(torch.int16), t.to(torch.int16), ic.NUM_CLASSES, void=void, connectivity=8, capacity=capacity)
    assert nnf.INSTANCE_CALLS == before + 2 and s16.table.is_cuda and same(s16.table, ref["tally"]) and same(s16.iou_sum, ref["iou_sum"])


@pytest.mark.parametrize("name", ["batch-lattice", "random-130x130", "shift-130x130"])
def test_two_calls_agree_bit_for_bit(name):
    p, t = (torch.from_numpy(x.copy()).to(dev()) for x in ic.case(name))
    (a, sa), (b, sb) = everything(p, t, name, 8), everything(p, t, name, 8)
    for key in a:
        assert E.same_bits(a[key], b[key]), key
    assert np.array_equal(np.float64([sa.pq, sa.sq, sa.rq]).view(np.int64), np.float64([sb.pq, sb.sq, sb.rq]).view(np.int64))


@pytest.mark.parametrize("name", ["batch-lattice", "batch-lattice-over"])
@pytest.mark.parametrize("conn", [4, 8])
def test_an_image_alone_equals_the_image_in_its_batch(conn, name):
    p, t = (torch.from_numpy(x.copy()).to(torch.int32).to(dev()) for x in ic.case(name))
    whole, _ = everything(p, t, name, conn)
    for k in range(p.shape[0]):
        alone, _ = everything(p[k:k + 1].contiguous(), t[k:k + 1].contiguous(), name, conn)
        for key in whole:
            assert E.same_bits(alone[key][0], whole[key][k]), (key, k)


# ------------------------------------------------------------------------------------------------------------------------------
# guard bands (tests/extent.py): every entry point at its smallest and at ragged cases, called through the library itself
# ------------------------------------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr()


def _void4(void):
    return list(void) + [0] * (4 - len(void))


def _chain(L, ref, pred_id, gt_id, target, capacity, void, what):
    """the four entry points in a row under the three surroundings; every launch's outputs feed the next as plain inputs.  Returns the
    outputs of the guarded (0xff) run."""
    b, h, w = pred_id.shape
    nb = int(L.vqseg_instance_vote_bits(capacity))
    ptab, gtab = torch.from_numpy(ref["pred_table"].copy()), torch.from_numpy(ref["gt_table"].copy())
    pcount, gcount = torch.from_numpy(ref["pred_count"].copy()), torch.from_numpy(ref["gt_count"].copy())
    sync = torch.cuda.synchronize
    out = {}
    spec = dict(pred_id=E.In(pred_id, align=4), gt_id=E.In(gt_id, align=4), target=E.In(target, align=target.element_size()),
                votes=E.Out((b, capacity, nb), torch.int32, align=4), void=E.Out((b, capacity), torch.int32, align=4))
    _, a, _ = E.run_case(spec, lambda t: L.vqseg_instance_vote_i32(_p(t["pred_id"]), _p(t["gt_id"]), _p(t["target"]), target.element_size(), b, h, w,
                                                                   capacity, len(void), *_void4(void), _p(t["votes"]), _p(t["void"]), _stream()),
                         dev(), sync, f"instance_vote {what}")
    votes, out["void"] = a["votes"].clone(), a["void"].clone()
    spec = dict(pred_id=E.In(pred_id, align=4), gt_id=E.In(gt_id, align=4), votes=E.In(votes.cpu(), align=4), gt_table=E.In(gtab, align=4),
                cand=E.Out((b, capacity), torch.int32, align=4), inter=E.Out((b, capacity), torch.int32, align=4))
    _, a, _ = E.run_case(spec, lambda t: L.vqseg_instance_overlap_i32(_p(t["pred_id"]), _p(t["gt_id"]), _p(t["votes"]), _p(t["gt_table"]), b, h, w,
                                                                      capacity, _p(t["cand"]), _p(t["inter"]), _stream()),
                         dev(), sync, f"instance_overlap {what}")
    cand, inter = a["cand"].clone(), a["inter"].clone()
    assert int(cand.min()) >= -1 and int(cand.max()) < capacity                 # range-checked: an id or -1
    spec = dict(cand=E.In(cand.cpu(), align=4), void=E.In(out["void"].cpu(), align=4), pred_table=E.In(ptab, align=4), gt_table=E.In(gtab, align=4),
                pred_count=E.In(pcount, align=4), gt_count=E.In(gcount, align=4), inter=E.InOut(inter.cpu(), align=4),
                match=E.Out((b, capacity), torch.int32, align=4), union=E.Out((b, capacity), torch.int32, align=4),
                matched=E.Out((b, capacity), torch.int32, align=4))
    _, a, _ = E.run_case(spec, lambda t: L.vqseg_instance_match_i32(_p(t["cand"]), _p(t["void"]), _p(t["pred_table"]), _p(t["gt_table"]),
                                                                    _p(t["pred_count"]), _p(t["gt_count"]), b, capacity, _p(t["inter"]), _p(t["match"]),
                                                                    _p(t["union"]), _p(t["matched"]), _stream()),
                         dev(), sync, f"instance_match {what}")
    for key in ("match", "inter", "union", "matched"):
        out[key] = a[key].clone()
    c = ic.NUM_CLASSES
    spec = dict(match=E.In(out["match"].cpu(), align=4), matched=E.In(out["matched"].cpu(), align=4), inter=E.In(out["inter"].cpu(), align=4),
                union=E.In(out["union"].cpu(), align=4), void=E.In(out["void"].cpu(), align=4), pred_table=E.In(ptab, align=4),
                gt_table=E.In(gtab, align=4), pred_count=E.In(pcount, align=4), gt_count=E.In(gcount, align=4),
                tally=E.Out((b, c, 5), torch.int32, align=4), iou_sum=E.Out((b, c), torch.float64, align=8), overflow=E.Out((b,), torch.int32, align=4))
    _, a, _ = E.run_case(spec, lambda t: L.vqseg_instance_tally_i32(_p(t["match"]), _p(t["matched"]), _p(t["inter"]), _p(t["union"]), _p(t["void"]),
                                                                    _p(t["pred_table"]), _p(t["gt_table"]), _p(t["pred_count"]), _p(t["gt_count"]), b,
                                                                    capacity, c, _p(t["tally"]), _p(t["iou_sum"]), _p(t["overflow"]), _stream()),
                         dev(), sync, f"instance_tally {what}")
    for key in ("tally", "iou_sum", "overflow"):
        out[key] = a[key].clone()
    return out


EXTENT = [("one-1x1", 4, "u8"), ("void-trim", 4, "i32"), ("split3", 8, "u8"), ("lattice-exact", 8, "u8"), ("batch-lattice-over", 4, "i32")]


@pytest.mark.parametrize("name,conn,dtype", EXTENT)
def test_extent_of_every_entry_point(name, conn, dtype):
    L = _hip.lib()
    ref = ic.reference(name, conn)
    _things, void, capacity, _over = ic.settings(name)
    target = torch.from_numpy(ref["target"].copy()).to(DTYPES[dtype])
    got = _chain(L, ref, torch.from_numpy(ref["pred_id"].copy()), torch.from_numpy(ref["gt_id"].copy()), target, capacity, void, f"{name} {dtype}")
    for key in KEYS:
        assert same(got[key], ref[key]), key


def test_ids_handed_in_are_never_used_as_indices():
    """id maps with entries < -1 and >= capacity: those pixels belong to no region (the restatement on the same maps), the bands stay intact"""
    L = _hip.lib()
    name, conn = "shift3-67x131", 8
    ref = ic.reference(name, conn)
    _things, void, capacity, _over = ic.settings(name)
    g = np.random.default_rng(13)
    wild = np.array([capacity, capacity + 1, 65535, 65536, 2 ** 31 - 1, -2, -2 ** 31, 1 << 20], dtype=np.int64)
    pred_id, gt_id = ref["pred_id"].copy(), ref["gt_id"].copy()
    hits = {}
    for key, ids in (("pred", pred_id), ("gt", gt_id)):
        member = np.nonzero(ids.reshape(-1) >= 0)[0]
        hits[key] = g.choice(member, size=150, replace=False)
        ids.reshape(-1)[hits[key]] = g.choice(wild, size=150).astype(np.int32)
    want = ic.match_from(pred_id, gt_id, ref["target"], ref["pred_table"], ref["gt_table"], ref["pred_count"], ref["gt_count"], void, capacity,
                         ic.NUM_CLASSES)
    assert not np.array_equal(want["inter"], ref["inter"])                       # the wild entries took pixels away
    got = _chain(L, ref, torch.from_numpy(pred_id), torch.from_numpy(gt_id), torch.from_numpy(ref["target"].copy()), capacity, void, "wild ids")
    for key in KEYS:
        assert same(got[key], want[key]), key
