"""The region kernels (csrc/region_kernels.hip) against the plain union-find of tests/region_cases.py: roots, ids, counts, areas,
table, moments and both filter fills on every case, for both connectivities and both element types -- exact integer equality, nothing
has a tolerance.  Then what equality on one call cannot show: overflowing tables, two calls, an image alone against the image in its
batch, the guard bands of tests/extent.py around every entry point, and root / id maps with entries that are no indices."""
import numpy as np
import pytest
import torch

from tests import extent as E
from tests import region_cases as rc
from vq_seg_amd import _hip, nnf
from vq_seg_amd.utils import regions

pytestmark = pytest.mark.gpu

DTYPES = {"u8": torch.uint8, "i32": torch.int32}


def dev():
    return torch.device("cuda:0")


def same(t, want):
    return np.array_equal(t.cpu().numpy(), want)


def everything(v, conn, capacity=rc.CAPACITY):
    roots = nnf.region_roots(v, conn, rc.IGNORE)
    ids, counts = nnf.region_ids(roots)
    areas = nnf.region_areas(roots)
    table, moments = nnf.region_table(v, roots, ids, counts, capacity)
    fill0 = nnf.filter_regions(v, rc.MIN_AREA, conn, rc.IGNORE, fill=0)
    neighbour = nnf.filter_regions(v, rc.MIN_AREA, conn, rc.IGNORE, fill="neighbour")
    return dict(roots=roots, ids=ids, counts=counts, areas=areas, table=table, moments=moments, fill0=fill0, neighbour=neighbour)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", rc.CASES)
def test_kernels_equal_the_reference(name, conn, dtype):
    ref = rc.reference(name, conn)
    v = torch.from_numpy(ref["values"].copy()).to(DTYPES[dtype]).to(dev())
    assert nnf.regions_supported(v)
    got = everything(v, conn)
    for key in ("roots", "ids", "counts", "areas", "table", "moments"):
        assert got[key].dtype == (torch.int64 if key == "moments" else torch.int32), key
        assert same(got[key], ref[key]), f"{key} differs: {int((got[key].cpu().numpy() != ref[key]).sum())} entries"
    for key in ("fill0", "neighbour"):
        assert got[key].dtype == v.dtype and same(got[key], ref[key].astype(got[key].cpu().numpy().dtype)), key


def test_int64_maps_and_the_public_surface_take_the_kernels():
    ref = rc.reference("batch", 8)
    v = torch.from_numpy(ref["values"].copy()).long().to(dev())
    before = nnf.REGION_CALLS
    out = regions.remove_small_regions(v, rc.MIN_AREA, 8, rc.IGNORE, fill="neighbour")
    assert nnf.REGION_CALLS == before + 1 and out.dtype == torch.int64 and same(out, ref["neighbour"].astype(np.int64))
    ids, counts = regions.label_regions(v, 8, rc.IGNORE)
    assert ids.is_cuda and same(ids, ref["ids"]) and same(counts, ref["counts"])
    r = regions.region_table(v, 8, rc.IGNORE, capacity=rc.CAPACITY)
    t = ref["table"]
    assert same(r.count, ref["counts"]) and same(r.value, t[..., 0]) and same(r.area, t[..., 1]) and same(r.bbox, t[..., 2:6]) and same(r.root, t[..., 6])
    assert same(r.centroid, ref["moments"].astype(np.float64) / np.maximum(t[..., 1], 1).astype(np.float64)[..., None])
    # an element type the kernels do not take: the torch-op form on the device, the same numbers
    ids16, counts16 = regions.label_regions(v.to(torch.int16), 8, rc.IGNORE)
    assert same(ids16, ref["ids"]) and same(counts16, ref["counts"])


@pytest.mark.parametrize("conn", [4, 8])
def test_a_table_that_overflows_keeps_counts_and_ids(conn):
    ref = rc.reference("batch", conn)
    v = torch.from_numpy(ref["values"].copy()).to(dev())
    got = everything(v, conn, capacity=2)
    assert int(ref["counts"].min()) > 2
    assert same(got["counts"], ref["counts"]) and same(got["ids"], ref["ids"])
    assert same(got["table"], ref["table"][:, :2]) and same(got["moments"], ref["moments"][:, :2])
    one = torch.from_numpy(rc.case("constant-33x65").copy()).to(dev())         # fewer regions than rows: the rest stays zero
    t, m = everything(one, conn, capacity=3)["table"], everything(one, conn, capacity=3)["moments"]
    assert t[0, 0].tolist() == [1, 33 * 65, 0, 0, 32, 64, 0, 0] and int(t[0, 1:].abs().sum()) == 0 and int(m[0, 1:].abs().sum()) == 0
    assert m[0, 0].tolist() == [65 * (32 * 33 // 2), 33 * (64 * 65 // 2)]


@pytest.mark.parametrize("name", ["batch", "random59-130x130", "spiral-130x130"])
def test_two_calls_agree_bit_for_bit(name):
    v = torch.from_numpy(rc.case(name).copy()).to(dev())
    a, b = everything(v, 8), everything(v, 8)
    for key in a:
        assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize("conn", [4, 8])
def test_an_image_alone_equals_the_image_in_its_batch(conn):
    v = torch.from_numpy(rc.case("batch").copy()).to(torch.int32).to(dev())
    whole = everything(v, conn)
    for k in range(v.shape[0]):
        alone = everything(v[k:k + 1].contiguous(), conn)
        for key in whole:
            assert torch.equal(alone[key][0], whole[key][k]), (key, k)


# ------------------------------------------------------------------------------------------------------------------------------
# guard bands (tests/extent.py): every entry point at its smallest and at a ragged case, called through the library itself
# ------------------------------------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr()


def _maps(name, conn):
    ref = rc.reference(name, conn)
    return ref, torch.from_numpy(ref["values"].copy())


EXTENT = [("constant-1x1", 4), ("random59-33x65", 8), ("batch", 8)]


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name,conn", EXTENT)
def test_extent_roots(name, conn, dtype):
    L = _hip.lib()
    ref, v = _maps(name, conn)
    b, h, w = v.shape
    fn = getattr(L, f"vqseg_region_roots_{dtype}")
    spec = dict(values=E.In(v.to(DTYPES[dtype]), align=1), parent=E.Out((b, h, w), torch.int32, align=4, compare=0),
                root=E.Out((b, h, w), torch.int32, align=4))
    _, a, _ = E.run_case(spec, lambda t: fn(_p(t["values"]), b, h, w, conn, 1, 255, 0, 0, 0, _p(t["parent"]), _p(t["root"]), _stream()),
                         dev(), torch.cuda.synchronize, f"region_roots_{dtype} {name}")
    assert same(a["root"], ref["roots"])


@pytest.mark.parametrize("name,conn", EXTENT)
def test_extent_ids_areas_table_filter(name, conn):
    L = _hip.lib()
    ref, v = _maps(name, conn)
    b, h, w = v.shape
    nblk = int(L.vqseg_region_ids_partials(h, w))
    root, ids, area = (torch.from_numpy(ref[k].copy()) for k in ("roots", "ids", "areas"))
    spec = dict(root=E.In(root, align=4), partial=E.Out((b, nblk), torch.int32, align=4, compare=0), id=E.Out((b, h, w), torch.int32, align=4),
                count=E.Out((b,), torch.int32, align=4))
    _, a, _ = E.run_case(spec, lambda t: L.vqseg_region_ids_i32(_p(t["root"]), b, h, w, _p(t["partial"]), _p(t["id"]), _p(t["count"]), _stream()),
                         dev(), torch.cuda.synchronize, f"region_ids {name}")
    assert same(a["id"], ref["ids"]) and same(a["count"], ref["counts"])
    spec = dict(root=E.In(root, align=4), area=E.Out((b, h, w), torch.int32, align=4))
    _, a, _ = E.run_case(spec, lambda t: L.vqseg_region_areas_i32(_p(t["root"]), b, h, w, _p(t["area"]), _stream()),
                         dev(), torch.cuda.synchronize, f"region_areas {name}")
    assert same(a["area"], ref["areas"])
    for cap in (1, rc.CAPACITY):
        for vals in (v, v.to(torch.int32)):
            spec = dict(values=E.In(vals, align=1), root=E.In(root, align=4), id=E.In(ids, align=4), table=E.Out((b, cap, 8), torch.int32, align=4),
                        moments=E.Out((b, cap, 2), torch.int64, align=8))
            _, a, _ = E.run_case(spec, lambda t: L.vqseg_region_table_i32(_p(t["values"]), vals.element_size(), _p(t["root"]), _p(t["id"]), b, h, w,
                                                                          cap, _p(t["table"]), _p(t["moments"]), _stream()),
                                 dev(), torch.cuda.synchronize, f"region_table {name} capacity {cap}")
            assert same(a["table"], ref["table"][:, :cap]) and same(a["moments"], ref["moments"][:, :cap])
    for dtype, tdt in DTYPES.items():
        fn = getattr(L, f"vqseg_region_filter_{dtype}")
        for neighbour, key in ((0, "fill0"), (1, "neighbour")):
            spec = dict(values=E.In(v.to(tdt), align=1), root=E.In(root, align=4), area=E.In(area, align=4), out=E.Out((b, h, w), tdt, align=1))
            _, a, _ = E.run_case(spec, lambda t: fn(_p(t["values"]), _p(t["root"]), _p(t["area"]), b, h, w, rc.MIN_AREA, neighbour, 0, _p(t["out"]),
                                                    _stream()), dev(), torch.cuda.synchronize, f"region_filter_{dtype} {name} {key}")
            assert same(a["out"], ref[key].astype(a["out"].cpu().numpy().dtype))


def test_maps_handed_in_are_never_used_as_indices():
    """roots / ids with entries outside [0, h w) / [0, capacity): those pixels count as ignored, the bands stay intact"""
    L = _hip.lib()
    ref, v = _maps("random59-33x65", 8)
    b, h, w = v.shape
    n = h * w
    g = np.random.default_rng(9)
    root = ref["roots"].copy()
    flat = root.reshape(-1)
    member = np.nonzero((flat >= 0) & (flat != np.arange(n)))[0]                 # pixels that are not roots: the trees stay intact
    hit = g.choice(member, size=200, replace=False)
    flat[hit] = g.choice(np.array([n, n + 1, 2 ** 31 - 1, -2, -2 ** 31, 1 << 20], dtype=np.int64), size=200).astype(np.int32)
    want_ids, want_counts = rc.ids(root)
    want_areas = rc.areas(root)
    nblk = int(L.vqseg_region_ids_partials(h, w))
    rt = torch.from_numpy(root)
    spec = dict(root=E.In(rt, align=4), partial=E.Out((b, nblk), torch.int32, align=4, compare=0), id=E.Out((b, h, w), torch.int32, align=4),
                count=E.Out((b,), torch.int32, align=4))
    _, a, _ = E.run_case(spec, lambda t: L.vqseg_region_ids_i32(_p(t["root"]), b, h, w, _p(t["partial"]), _p(t["id"]), _p(t["count"]), _stream()),
                         dev(), torch.cuda.synchronize, "region_ids with wild roots")
    assert same(a["id"], want_ids) and same(a["count"], want_counts) and (want_ids.reshape(-1)[hit] == -1).all()
    spec = dict(root=E.In(rt, align=4), area=E.Out((b, h, w), torch.int32, align=4))
    _, a, _ = E.run_case(spec, lambda t: L.vqseg_region_areas_i32(_p(t["root"]), b, h, w, _p(t["area"]), _stream()),
                         dev(), torch.cuda.synchronize, "region_areas with wild roots")
    assert same(a["area"], want_areas)
    ids = want_ids.copy()
    wild = g.choice(n, size=200, replace=False)
    ids.reshape(-1)[wild] = g.choice(np.array([rc.CAPACITY, 2 ** 31 - 1, -5, -2 ** 31], dtype=np.int64), size=200).astype(np.int32)
    want_table, want_moments = rc.table(ref["values"], root, ids, rc.CAPACITY)
    spec = dict(values=E.In(v, align=1), root=E.In(rt, align=4), id=E.In(torch.from_numpy(ids), align=4),
                table=E.Out((b, rc.CAPACITY, 8), torch.int32, align=4), moments=E.Out((b, rc.CAPACITY, 2), torch.int64, align=8))
    _, a, _ = E.run_case(spec, lambda t: L.vqseg_region_table_i32(_p(t["values"]), 1, _p(t["root"]), _p(t["id"]), b, h, w, rc.CAPACITY,
                                                                  _p(t["table"]), _p(t["moments"]), _stream()),
                         dev(), torch.cuda.synchronize, "region_table with wild roots and ids")
    # a region whose root pixel lost its id has no value / ymin / root column to compare: the rows of the others are exact
    lost = np.unique(want_ids.reshape(-1)[np.intersect1d(wild, np.nonzero(ref["roots"].reshape(-1) == np.arange(n))[0])])
    keep = np.setdiff1d(np.arange(rc.CAPACITY), lost[lost >= 0])
    assert len(keep) > rc.CAPACITY - 200
    assert np.array_equal(a["table"].cpu().numpy()[:, keep], want_table[:, keep])
    assert np.array_equal(a["moments"].cpu().numpy()[:, keep], want_moments[:, keep])
    for neighbour, fill in ((0, 0), (1, "neighbour")):
        want = rc.filter(ref["values"], root, want_areas, rc.MIN_AREA, fill)
        spec = dict(values=E.In(v, align=1), root=E.In(rt, align=4), area=E.In(torch.from_numpy(want_areas), align=4), out=E.Out((b, h, w), torch.uint8, align=1))
        _, a, _ = E.run_case(spec, lambda t: L.vqseg_region_filter_u8(_p(t["values"]), _p(t["root"]), _p(t["area"]), b, h, w, rc.MIN_AREA, neighbour,
                                                                      0, _p(t["out"]), _stream()), dev(), torch.cuda.synchronize,
                             f"region_filter_u8 with wild roots, fill {fill}")
        assert same(a["out"], want)
