"""Connected regions on the CPU: the plain union-find of tests/region_cases.py against scipy.ndimage.label, the torch-op form of
vq_seg_amd.utils.regions against that reference on every case, and the argument checks of nnf / Predictor / CPSConfig, which raise
before any device is touched.  Every comparison is exact integer equality."""
import numpy as np
import pytest
import torch

from tests import region_cases as rc
from vq_seg_amd import _hip, nnf
from vq_seg_amd.utils import regions

BINARY = [n for n in rc.CASES if n.split("-")[0] in ("random59", "checkerboard", "serpentine", "spiral", "diagonal", "antidiagonal", "comb", "constant")]
DTYPES = {"u8": torch.uint8, "i32": torch.int32, "i64": torch.int64}


def test_the_case_table_is_what_the_suites_say_it_is():
    assert len(rc.CASES) == len(rc.PATTERNS) * len(rc.SHAPES) + 1
    assert rc.case("batch").shape == rc.BATCH_SHAPE
    v = rc.case("batch")
    assert (v[0, -1] == v[1, 0]).all()                          # the last row of image 0 and the first of image 1 carry one value
    for conn in (4, 8):
        for name in ("serpentine-130x130", "spiral-130x130", "spiral-67x131", "comb-33x65"):
            ref = rc.reference(name, conn)
            ones = ref["table"][0, :int(ref["counts"][0])]
            assert (ones[:, 0] != 0).sum() == 1, name           # one region of the pattern's value, through the whole image
    h = 130
    assert int(rc.reference("diagonal-130x130", 8)["counts"][0]) == 2 and int(rc.reference("diagonal-130x130", 4)["counts"][0]) == h + 2
    assert int(rc.reference("antidiagonal-130x130", 8)["counts"][0]) == 2 and int(rc.reference("antidiagonal-130x130", 4)["counts"][0]) == h + 2
    assert int(rc.reference("ignored-33x65", 4)["counts"][0]) == 0 and (rc.reference("ignored-33x65", 4)["roots"] == -1).all()
    assert int(rc.reference("constant-130x130", 4)["counts"][0]) == 1
    assert int(rc.reference("checkerboard-130x130", 4)["counts"][0]) == 130 * 130 > rc.CAPACITY


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", BINARY)
def test_reference_is_scipys_labelling(name, conn):
    ndimage = pytest.importorskip("scipy.ndimage")
    v = (rc.case(name)[0] == 1).astype(np.uint8) if not name.startswith("comb") else (rc.case(name)[0] == 2).astype(np.uint8)
    structure = np.ones((3, 3), dtype=int) if conn == 8 else None
    want, n = ndimage.label(v, structure=structure)
    got, counts = rc.ids(rc.roots(v[None], conn, ignore=(0,)))
    assert int(counts[0]) == n
    assert np.array_equal(got[0] + 1, want)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", rc.CASES)
def test_torch_form_equals_the_reference(name, conn):
    ref = rc.reference(name, conn)
    v = torch.from_numpy(ref["values"].copy())
    roots = regions.roots_torch(v, conn, rc.IGNORE)
    assert roots.dtype == torch.int32 and np.array_equal(roots.numpy(), ref["roots"])
    ids, counts = regions.ids_torch(roots)
    assert np.array_equal(ids.numpy(), ref["ids"]) and np.array_equal(counts.numpy(), ref["counts"])
    assert np.array_equal(regions.areas_torch(roots).numpy(), ref["areas"])
    table, moments = regions.table_torch(v, roots, ids, rc.CAPACITY)
    assert table.dtype == torch.int32 and moments.dtype == torch.int64
    assert np.array_equal(table.numpy(), ref["table"]) and np.array_equal(moments.numpy(), ref["moments"])


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("name", rc.CASES)
def test_public_surface_on_cpu_tensors(name, conn, dtype):
    ref = rc.reference(name, conn)
    v = torch.from_numpy(ref["values"].copy()).to(DTYPES[dtype])
    ids, counts = regions.label_regions(v, conn, rc.IGNORE)
    assert ids.dtype == torch.int32 and np.array_equal(ids.numpy(), ref["ids"]) and np.array_equal(counts.numpy(), ref["counts"])
    for fill, key in ((0, "fill0"), ("neighbour", "neighbour")):
        out = regions.remove_small_regions(v, rc.MIN_AREA, conn, rc.IGNORE, fill=fill)
        assert out.dtype == v.dtype and np.array_equal(out.numpy(), ref[key].astype(out.numpy().dtype)), (fill,)
    r = regions.region_table(v, conn, rc.IGNORE, capacity=rc.CAPACITY)
    t = ref["table"]
    assert np.array_equal(r.count.numpy(), ref["counts"]) and np.array_equal(r.value.numpy(), t[..., 0]) and np.array_equal(r.area.numpy(), t[..., 1])
    assert np.array_equal(r.bbox.numpy(), t[..., 2:6]) and np.array_equal(r.root.numpy(), t[..., 6])
    want = ref["moments"].astype(np.float64) / np.maximum(t[..., 1], 1).astype(np.float64)[..., None]
    assert r.centroid.dtype == torch.float64 and np.array_equal(r.centroid.numpy(), want)


def test_numpy_maps_single_images_and_overflowing_tables():
    ref = rc.reference("random50-33x65", 8)
    v = ref["values"][0]
    ids, count = regions.label_regions(v, 8, rc.IGNORE)
    assert isinstance(ids, np.ndarray) and ids.shape == v.shape and np.array_equal(ids, ref["ids"][0]) and int(count) == int(ref["counts"][0])
    out = regions.remove_small_regions(v, rc.MIN_AREA, 8, rc.IGNORE, fill="neighbour")
    assert isinstance(out, np.ndarray) and out.dtype == np.uint8 and np.array_equal(out, ref["neighbour"][0])
    r, ids2 = regions.region_table(v, 8, rc.IGNORE, capacity=2, return_ids=True)
    assert int(r.count) == int(ref["counts"][0]) > 2 and np.array_equal(ids2, ref["ids"][0])
    assert np.array_equal(r.area, ref["table"][0, :2, 1]) and np.array_equal(r.root, ref["table"][0, :2, 6])
    few = regions.region_table(rc.case("constant-2x2")[0], capacity=5)
    assert int(few.count) == 1 and few.area.tolist() == [4, 0, 0, 0, 0] and few.centroid.tolist()[0] == [0.5, 0.5] and few.bbox.tolist()[0] == [0, 0, 1, 1]


def test_enforce_connectivity_keeps_a_label_map_a_label_map():
    g = np.random.default_rng(5)
    labels = np.repeat(np.repeat(np.arange(12, dtype=np.int32).reshape(3, 4), 8, axis=0), 8, axis=1)[None].copy()      # a 3 x 4 grid of 8 x 8 cells
    at = g.integers(0, 24, size=(20, 2))
    labels[0, at[:, 0], at[:, 1] + 4] = 11                      # stray pixels of label 11 elsewhere
    out = regions.enforce_connectivity(torch.from_numpy(labels), 4)
    assert out.dtype == torch.int32 and set(np.unique(out.numpy())) <= set(range(12))
    assert np.array_equal(out.numpy(), rc.remove_small(labels, 4, 4, (), "neighbour"))
    _, counts = regions.label_regions(out)
    _, before = regions.label_regions(labels)
    assert int(counts[0]) < int(before[0])


def test_nnf_refuses_wrong_arguments_before_touching_a_device():
    E = _hip.HipLibraryError
    u8 = torch.zeros(1, 4, 4, dtype=torch.uint8)
    i32 = torch.zeros(1, 4, 4, dtype=torch.int32)
    assert not nnf.regions_supported(u8) and not nnf.regions_supported(None)
    for bad in (3, 6, True, "4", None):
        with pytest.raises(ValueError, match="connectivity must be 4 or 8"):
            nnf.region_roots(u8, connectivity=bad)
    for bad in ((1, 2, 3, 4, 5), (1.5,), (2 ** 31,), "ab", (True,)):
        with pytest.raises(ValueError, match="ignore must be"):
            nnf.region_roots(u8, ignore=bad)
    with pytest.raises(E, match=r"values must be a \(B, H, W\) tensor"):
        nnf.region_roots(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(E, match="values must be uint8 or int32 or int64, got torch.float32"):
        nnf.region_roots(torch.zeros(1, 4, 4))
    with pytest.raises(E, match="sides of 1..4096"):
        nnf.region_roots(torch.zeros(1, 1, 4097, dtype=torch.uint8))
    with pytest.raises(E, match="sides of 1..4096"):
        nnf.region_roots(torch.zeros(1, 0, 4, dtype=torch.uint8))
    with pytest.raises(E, match="roots must be int32, got torch.int64"):
        nnf.region_ids(i32.long())
    with pytest.raises(E, match="roots must be int32"):
        nnf.region_areas(u8)
    with pytest.raises(E, match="ids must have the values' shape"):
        nnf.region_table(u8, i32, torch.zeros(1, 4, 5, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 4)
    with pytest.raises(E, match="counts must be an int32 tensor"):
        nnf.region_table(u8, i32, i32, torch.zeros(2, dtype=torch.int32), 4)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="capacity must be a positive integer"):
            nnf.region_table(u8, i32, i32, torch.zeros(1, dtype=torch.int32), bad)
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="min_area must be an integer >= 0"):
            nnf.filter_regions(u8, bad)
    for bad in (256, -1, "left", 1.0, True):
        with pytest.raises(ValueError, match="fill must be 'neighbour' or an integer"):
            nnf.filter_regions(u8, 2, fill=bad)
    with pytest.raises(ValueError, match="fill must be 'neighbour' or an integer"):
        nnf.filter_regions(i32, 2, fill=2 ** 31)
    # everything right on CPU tensors: the device error surfaces, from every wrapper
    for call in (lambda: nnf.region_roots(u8), lambda: nnf.region_roots(i32.long(), 8, (255,)), lambda: nnf.region_ids(i32),
                 lambda: nnf.region_areas(i32), lambda: nnf.region_table(u8, i32, i32, torch.zeros(1, dtype=torch.int32), 4),
                 lambda: nnf.filter_regions(u8, 2), lambda: nnf.filter_regions(i32, 2, fill="neighbour"),
                 lambda: nnf.filter_regions_from(u8, i32, i32, 2)):
        with pytest.raises(E, match="no CPU fallback"):
            call()


def test_the_entry_points_refuse_bad_arguments_without_a_device():
    L = _hip.lib()
    one = 1                                                         # any non-null address: refused before it is looked at
    assert L.vqseg_region_roots_u8(None, 1, 4, 4, 4, 0, 0, 0, 0, 0, None, None, None) == -1 and b"null" in L.vqseg_last_error()
    assert L.vqseg_region_roots_u8(one, 1, 4, 4, 4, 0, 0, 0, 0, 0, one, one, None) == -1 and b"two buffers" in L.vqseg_last_error()
    assert L.vqseg_region_roots_i32(one, 1, 4, 4, 6, 0, 0, 0, 0, 0, one, 2, None) == -1 and b"connectivity" in L.vqseg_last_error()
    assert L.vqseg_region_roots_i32(one, 1, 4, 4, 8, 5, 0, 0, 0, 0, one, 2, None) == -1 and b"ignored values" in L.vqseg_last_error()
    assert L.vqseg_region_roots_u8(one, 65536, 4, 4, 4, 0, 0, 0, 0, 0, one, 2, None) == -1 and b"65535" in L.vqseg_last_error()
    assert L.vqseg_region_roots_u8(one, 1, 4097, 4, 4, 0, 0, 0, 0, 0, one, 2, None) == -1 and b"4096" in L.vqseg_last_error()
    assert L.vqseg_region_roots_u8(one, 1, 4, 0, 4, 0, 0, 0, 0, 0, one, 2, None) == -1 and b"positive" in L.vqseg_last_error()
    assert L.vqseg_region_ids_i32(one, 1, 4, 4, one, one, one, None) == -1 and b"two buffers" in L.vqseg_last_error()
    assert L.vqseg_region_ids_i32(one, 0, 4, 4, one, 2, one, None) == -1
    assert L.vqseg_region_ids_partials(4096, 4096) == 16384 and L.vqseg_region_ids_partials(1, 1) == 1 and L.vqseg_region_ids_partials(33, 65) == 3
    assert L.vqseg_region_ids_partials(0, 4) == 0 and L.vqseg_region_ids_partials(4, 4097) == 0
    assert L.vqseg_region_table_i32(one, 2, one, one, 1, 4, 4, 4, one, one, None) == -1 and b"value_bytes" in L.vqseg_last_error()
    assert L.vqseg_region_table_i32(one, 1, one, one, 1, 4, 4, 0, one, one, None) == -1 and b"capacity" in L.vqseg_last_error()
    assert L.vqseg_region_areas_i32(one, 1, 4, 4, None, None) == -1 and b"null" in L.vqseg_last_error()
    assert L.vqseg_region_filter_u8(one, one, one, 1, 4, 4, 2, 0, 256, 2, None) == -1 and b"0..255" in L.vqseg_last_error()
    assert L.vqseg_region_filter_u8(one, one, one, 1, 4, 4, 2, 2, 0, 2, None) == -1 and b"neighbour" in L.vqseg_last_error()
    assert L.vqseg_region_filter_i32(one, one, one, 1, 4, 4, 2, 0, 0, one, None) == -1 and b"out of place" in L.vqseg_last_error()


def test_predictor_and_config_refuse_bad_region_options():
    from vq_seg_amd.predict import Predictor
    from vq_seg_amd.trainer import CPSConfig
    net = torch.nn.Conv2d(3, 3, 1)
    for kw, msg in ((dict(min_area=-1), "min_area must be an integer >= 0"), (dict(min_area=2.5), "min_area"),
                    (dict(min_area=4, min_area_fill=256), "fill must be"), (dict(min_area=4, min_area_fill="nearest"), "fill must be"),
                    (dict(connectivity=6), "connectivity must be 4 or 8"), (dict(region_ignore=(0, 1, 2, 3, 4)), "ignore must be")):
        with pytest.raises(ValueError, match=msg):
            Predictor(net, 3, **kw)
    p = Predictor(net, 3)
    assert p.min_area is None and p.connectivity == 4 and p.region_ignore == () and p.min_area_fill == 0
    x = torch.zeros(1, 2, 2, dtype=torch.uint8)
    assert p._filtered(x) is x                                      # off: the map itself
    with pytest.raises(ValueError, match="classes are ids in 0..2"):
        Predictor(net, 3, min_area=4).instances(torch.zeros(1, 3, 8, 8), classes=(1, 3))
    model = {"name": "unet", "params": {}}
    assert CPSConfig(model=model).pseudo_min_area is None and CPSConfig(model=model).pseudo_connectivity == 4
    assert CPSConfig(model=model, pseudo_min_area=64, pseudo_connectivity=8).pseudo_min_area == 64
    for kw, msg in ((dict(pseudo_min_area=-3), "pseudo_min_area"), (dict(pseudo_min_area=1.5), "pseudo_min_area"),
                    (dict(pseudo_min_area=True), "pseudo_min_area"), (dict(pseudo_connectivity=5), "pseudo_connectivity")):
        with pytest.raises(ValueError, match=msg):
            CPSConfig(model=model, **kw)
    from vq_seg_amd.evaluate import test_loop
    with pytest.raises(ValueError, match="min_area needs fused=True"):
        test_loop(net, [], 3, min_area=4)
    with pytest.raises(ValueError, match="min_area_fill must be a class id or 'neighbour'"):
        test_loop(net, [], 3, fused=True, min_area=4, min_area_fill=255)
