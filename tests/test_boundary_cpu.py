"""Boundary metrics on the CPU: the plain restatement of tests/boundary_cases.py against scipy.ndimage.distance_transform_edt, the
torch-op form of vq_seg_amd.utils.boundary against the restatement on every case, the score conventions on a hand-made table,
BoundaryMeasurement over two batches, and the argument checks of nnf / utils.boundary / test_loop, which raise before any device is
touched.  Every comparison of counts and distances is exact integer equality."""
import numpy as np
import pytest
import torch

from tests import boundary_cases as bc
from vq_seg_amd import _hip, nnf
from vq_seg_amd.utils import boundary

NAN = float("nan")


def test_the_case_table_is_what_the_suites_say_it_is():
    assert len(bc.CASES) == 10 * len(bc.SHAPES) + 1 and bc.pair("batch")[0].shape == (3, 40, 72)
    assert [bc.squared(t) for t, _ in bc.SETTINGS] == [0, 1, 4, 12]                     # floor(3.5^2) = 12, not 13
    ref = bc.reference("checkerboard-17x65")
    assert np.array_equal(ref["bg"][0, 0] + ref["bg"][0, 1], np.ones((17, 65), dtype=np.uint8))          # every pixel is a boundary
    ref = bc.reference("constant-33x130")
    assert not ref["bg"].any() and (ref["dg"] == bc.EDT_NONE).all()
    assert (bc.reference_counts("ignored-33x130", 2, 3)[..., :6] == 0).all() and (bc.reference_counts("ignored-33x130", 2, 3)[..., 6:] == -1).all()
    s, d = bc.seed_plane("lone-first")
    assert d[256, 258] == 256 ** 2 + 258 ** 2 == 132100 and d[0, 0] == 0
    s, d = bc.seed_plane("lone-last")
    assert d[0, 0] == 132100


def test_boundary_definition_on_a_hand_made_map():
    v = np.array([[[0, 0, 1, 1],
                   [0, 255, 1, 7],
                   [0, 0, 0, 1]]], dtype=np.uint8)
    b = bc.boundaries(v, 2, (255,))
    # class 0: (0, 1) touches the 1 at (0, 2); (1, 0) touches only the ignored pixel; (2, 2) touches the 1s above and beside it
    assert b[0, 0].tolist() == [[0, 1, 0, 0], [0, 0, 0, 0], [0, 0, 1, 0]]
    # class 1: (1, 2) has an ignored neighbour to its left and a 0 below; (0, 3) has the 7 below: a value >= C makes a boundary
    assert b[0, 1].tolist() == [[0, 0, 1, 1], [0, 0, 1, 0], [0, 0, 0, 1]]
    assert not bc.boundaries(np.full((1, 4, 4), 1, dtype=np.uint8), 2).any()            # the image border makes none


@pytest.mark.parametrize("name", bc.CASES)
def test_restatement_is_scipys_transform(name):
    from scipy import ndimage
    ref = bc.reference(name)
    for seeds, d2 in ((ref["bp"], ref["dp"]), (ref["bg"], ref["dg"])):
        for idx in np.ndindex(*seeds.shape[:2]):
            if seeds[idx].any():
                want = np.rint(ndimage.distance_transform_edt(seeds[idx] == 0) ** 2).astype(np.int64)
                assert np.array_equal(d2[idx], want), (name, idx)
            else:
                assert (d2[idx] == bc.EDT_NONE).all(), (name, idx)


@pytest.mark.parametrize("name", sorted(bc.SEED_PLANES))
def test_restatement_is_scipys_transform_on_the_seed_planes(name):
    from scipy import ndimage
    s, d = bc.seed_plane(name)
    assert np.array_equal(d, np.rint(ndimage.distance_transform_edt(s == 0) ** 2).astype(np.int64))


@pytest.mark.parametrize("name", bc.CASES)
def test_torch_form_equals_the_restatement(name):
    ref = bc.reference(name)
    p, t = torch.from_numpy(ref["pred"].copy()), torch.from_numpy(ref["target"].copy())
    bp, bg = boundary.boundaries_torch(p, bc.NUM_CLASSES, bc.IGNORE), boundary.boundaries_torch(t, bc.NUM_CLASSES, bc.IGNORE)
    assert bp.dtype == torch.uint8 and np.array_equal(bp.numpy(), ref["bp"]) and np.array_equal(bg.numpy(), ref["bg"])
    dp = boundary.edt_sq_torch(bp)
    assert dp.dtype == torch.int32 and np.array_equal(dp.numpy(), ref["dp"]) and np.array_equal(boundary.edt_sq_torch(bg).numpy(), ref["dg"])
    for tol, width in bc.SETTINGS:
        got = boundary.counts_torch(p, t, bc.NUM_CLASSES, bc.squared(tol), bc.squared(width), bc.IGNORE)
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), bc.reference_counts(name, tol, width)), (tol, width)


@pytest.mark.parametrize("name", sorted(bc.SEED_PLANES))
def test_torch_form_on_the_seed_planes(name):
    s, d = bc.seed_plane(name)
    assert np.array_equal(boundary.edt_sq_torch(torch.from_numpy(s.copy())).numpy(), d)
    assert np.array_equal(boundary.distance_transform(s.copy(), squared=True), d)


def test_public_surface_on_cpu_tensors_and_numpy_arrays():
    ref = bc.reference("batch")
    want = bc.reference_counts("batch", 2, 3)
    sc = bc.scores(want)
    for conv in (lambda a: a.copy(), lambda a: torch.from_numpy(a.copy()), lambda a: torch.from_numpy(a.copy()).long()):
        p, t = conv(ref["pred"]), conv(ref["target"])
        st = boundary.boundary_stats(p, t, 3, tolerance=2, width=3)
        assert type(st.table) is type(p) and np.array_equal(np.asarray(st.table), want)
        for key in ("f1", "precision", "recall", "iou", "hausdorff"):
            assert getattr(st, key).dtype == np.float64 and np.array_equal(getattr(st, key), sc[key], equal_nan=True), key
        assert np.array_equal(np.asarray(boundary.class_boundaries(p, 3)), ref["bp"])
    assert np.array_equal(boundary.boundary_f1(ref["pred"].copy(), ref["target"].copy(), 3, 2.0), bc.scores(bc.reference_counts("batch", 2, 2))["f1"])
    w1 = bc.counts(ref["pred"], ref["target"], 3, 1, 1, bc.IGNORE)
    assert np.array_equal(boundary.boundary_iou(ref["pred"].copy(), ref["target"].copy(), 3, 1.0), bc.scores(w1)["iou"])
    assert np.array_equal(boundary.hausdorff_distance(ref["pred"].copy(), ref["target"].copy(), 3), sc["hausdorff"])
    one = boundary.boundary_stats(ref["pred"][1].copy(), ref["target"][1].copy(), 3, 2, 3)                # an (H, W) map: no batch axis
    assert one.table.shape == (3, 8) and np.array_equal(one.table, want[1]) and np.array_equal(one.f1, sc["f1"][1])
    # width=None is the tolerance; the default ignore is (255,)
    assert np.array_equal(boundary.boundary_stats(ref["pred"].copy(), ref["target"].copy(), 3, 3.5).table, bc.reference_counts("batch", 3.5, 3.5))
    d = boundary.distance_transform(torch.tensor([[0, 0, 1], [0, 0, 0]], dtype=torch.uint8))
    assert d.dtype == torch.float32 and torch.equal(d, torch.tensor([[2.0, 1.0, 0.0], [5.0 ** 0.5, 2.0 ** 0.5, 1.0]]))
    none = boundary.distance_transform(np.zeros((2, 3, 3), dtype=bool))
    assert isinstance(none, np.ndarray) and np.isinf(none).all()
    assert (boundary.distance_transform(np.zeros((3, 3), dtype=np.uint8), squared=True) == boundary.EDT_NONE).all()
    assert boundary.boundary_tolerance(966, 1296) == 12 and boundary.boundary_tolerance(10, 10) == 1
    assert boundary.boundary_tolerance(512, 512, 0.01) == round(0.01 * 512 * 2 ** 0.5)


def test_score_conventions_on_a_hand_made_table():
    table = np.array([[[0, 0, 0, 0, 0, 0, -1, -1],              # neither map has a boundary of the class: F, HD undefined; no band: IoU undefined
                       [4, 0, 0, 0, 3, 6, -1, -1],              # only the prediction has one: F = 0, HD undefined
                       [0, 0, 5, 0, 0, 2, -1, -1],              # only the target has one: F = 0; bands that do not meet: IoU = 0
                       [4, 0, 5, 0, 1, 4, 9, 16],               # both, no hit: P + R == 0 -> F = 0; HD = sqrt(16)
                       [4, 2, 5, 5, 2, 4, 25, 2]]], dtype=np.int32)      # P = 1/2, R = 1: F = 2/3; HD = 5
    s = boundary.scores_from_table(table)
    assert np.array_equal(s.f1, [[NAN, 0.0, 0.0, 0.0, 2 * 0.5 * 1.0 / 1.5]], equal_nan=True)
    assert np.array_equal(s.precision, [[NAN, 0.0, NAN, 0.0, 0.5]], equal_nan=True)
    assert np.array_equal(s.recall, [[NAN, NAN, 0.0, 0.0, 1.0]], equal_nan=True)
    assert np.array_equal(s.iou, [[NAN, 0.5, 0.0, 0.25, 0.5]], equal_nan=True)
    assert np.array_equal(s.hausdorff, [[NAN, NAN, NAN, 4.0, 5.0]], equal_nan=True)
    ref = bc.scores(table)
    for key in ("f1", "precision", "recall", "iou", "hausdorff"):
        assert np.array_equal(getattr(s, key), ref[key], equal_nan=True), key
    assert torch.is_tensor(boundary.scores_from_table(torch.from_numpy(table)).table)
    # means skip NaN; a class that is NaN for every image is left out; the mean of nothing is NaN
    x = np.array([[NAN, 0.5, 1.0], [NAN, NAN, 0.0]])
    mean, per = boundary.mean_over_classes(x)
    assert np.array_equal(per, [NAN, 0.5, 0.5], equal_nan=True) and mean == 0.5
    assert bc.nanmean_classes(x)[0] == 0.5
    mean, per = boundary.mean_over_classes(np.full((2, 3), NAN))
    assert np.isnan(mean) and np.isnan(per).all()


def test_measurement_over_two_batches_equals_one_call_on_their_concatenation():
    from vq_seg_amd.measurement import BoundaryMeasurement
    assert BoundaryMeasurement is boundary.BoundaryMeasurement
    ref = bc.reference("batch")
    p, t = torch.from_numpy(ref["pred"].copy()), torch.from_numpy(ref["target"].copy())
    two = BoundaryMeasurement(3, tolerance=2, width=3)
    two.update(p[:2], t[:2])
    two.update(p[2:], t[2:])
    one = BoundaryMeasurement(3, tolerance=2, width=3)
    one.update(p, t)
    assert np.array_equal(two.table(), bc.reference_counts("batch", 2, 3)) and np.array_equal(one.table(), two.table())
    a, b = one.result(), two.result()
    sc = bc.scores(bc.reference_counts("batch", 2, 3))
    assert a["images"] == b["images"] == 3
    for key, src in (("boundary_f1", "f1"), ("boundary_iou", "iou"), ("hausdorff", "hausdorff")):
        mean, per = bc.nanmean_classes(sc[src])
        assert a[key] == b[key] and np.array_equal(a[key + "s"], b[key + "s"], equal_nan=True)
        assert a[key] == pytest.approx(mean, rel=1e-15) and np.allclose(a[key + "s"], per, rtol=1e-15, atol=0, equal_nan=True)
    empty = BoundaryMeasurement(3).result()
    assert empty["images"] == 0 and np.isnan(empty["boundary_f1"]) and np.isnan(empty["hausdorff"])


def test_new_symbols_are_exported_and_bound():
    L = _hip.lib()
    for name in ("vqseg_boundary_seeds_u8", "vqseg_boundary_seeds_i32", "vqseg_boundary_edt_rows_u8", "vqseg_boundary_edt_cols_i32",
                 "vqseg_boundary_counts_i32"):
        assert name in _hip.SYMBOLS and hasattr(L, name), name
    assert nnf.EDT_NONE == boundary.EDT_NONE == bc.EDT_NONE == 2 ** 31 - 1 and nnf.BOUNDARY_CALLS >= 0
    for name in ("class_boundaries", "edt_sq", "boundary_counts"):
        assert callable(getattr(nnf, name)), name
    # 2 C int32 planes per image stay under 512 MiB
    assert nnf.boundary_chunk(3, 512, 512) * 2 * 3 * 512 * 512 * 4 < 512 << 20 <= (nnf.boundary_chunk(3, 512, 512) + 1) * 2 * 3 * 512 * 512 * 4
    assert nnf.boundary_chunk(32, 2048, 2048) == 1 and nnf.boundary_chunk(1, 1, 1) == 1 << 19


def test_nnf_refuses_wrong_arguments_before_touching_a_device():
    E = _hip.HipLibraryError
    u8 = torch.zeros(1, 4, 4, dtype=torch.uint8)
    i64 = torch.zeros(1, 4, 4, dtype=torch.int64)
    assert not nnf.boundaries_supported(u8) and not nnf.boundaries_supported(None)
    for bad in (0, 33, 2.0, True, None):
        with pytest.raises(ValueError, match="num_classes must be an integer in 1..32"):
            nnf.class_boundaries(u8, bad)
        with pytest.raises(ValueError, match="num_classes must be an integer in 1..32"):
            nnf.boundary_counts(u8, u8, bad, 4, 4)
    for bad in ((1, 2, 3, 4, 5), (1.5,), (2 ** 31,), "ab", (True,)):
        with pytest.raises(ValueError, match="ignore must be"):
            nnf.class_boundaries(u8, 3, ignore=bad)
        with pytest.raises(ValueError, match="ignore must be"):
            nnf.boundary_counts(u8, u8, 3, 4, 4, ignore=bad)
    for bad in (-1, 1.5, True, 2 ** 31 - 1):
        with pytest.raises(ValueError, match="tol_sq must be an integer"):
            nnf.boundary_counts(u8, u8, 3, bad, 4)
        with pytest.raises(ValueError, match="width_sq must be an integer"):
            nnf.boundary_counts(u8, u8, 3, 4, bad)
    with pytest.raises(E, match=r"labels must be a \(B, H, W\) tensor"):
        nnf.class_boundaries(torch.zeros(4, 4, dtype=torch.uint8), 3)
    with pytest.raises(E, match="labels must be uint8 or int32 or int64, got torch.float32"):
        nnf.class_boundaries(torch.zeros(1, 4, 4), 3)
    with pytest.raises(E, match="sides of 1..2048"):
        nnf.class_boundaries(torch.zeros(1, 1, 2049, dtype=torch.uint8), 3)
    with pytest.raises(E, match="target must be uint8 or int32 or int64, got torch.int16"):
        nnf.boundary_counts(u8, u8.to(torch.int16), 3, 4, 4)
    with pytest.raises(E, match="target must have the values' shape"):
        nnf.boundary_counts(u8, torch.zeros(1, 4, 5, dtype=torch.uint8), 3, 4, 4)
    with pytest.raises(E, match="seeds must be uint8 or bool, got torch.int32"):
        nnf.edt_sq(torch.zeros(4, 4, dtype=torch.int32))
    with pytest.raises(E, match=r"seeds must be a \(..., H, W\) tensor"):
        nnf.edt_sq(torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(E, match="sides of 1..2048"):
        nnf.edt_sq(torch.zeros(2049, 1, dtype=torch.uint8))
    with pytest.raises(E, match="at least one plane"):
        nnf.edt_sq(torch.zeros(0, 4, 4, dtype=torch.uint8))
    # everything right on CPU tensors: the device error surfaces, from every wrapper, and the counter stays
    before = nnf.BOUNDARY_CALLS
    for call in (lambda: nnf.class_boundaries(u8, 3), lambda: nnf.class_boundaries(i64, 32, (255,)), lambda: nnf.edt_sq(u8),
                 lambda: nnf.edt_sq(torch.zeros(2, 3, 4, 4, dtype=torch.bool)), lambda: nnf.boundary_counts(u8, i64, 3, 4, 12, (255,))):
        with pytest.raises(E, match="no CPU fallback"):
            call()
    assert nnf.BOUNDARY_CALLS == before


def test_the_entry_points_refuse_bad_arguments_without_a_device():
    L = _hip.lib()
    one = 1                                                         # any non-null address: refused before it is looked at
    assert L.vqseg_boundary_seeds_u8(None, 1, 4, 4, 3, 0, 0, 0, 0, 0, one, None) == -1 and b"null" in L.vqseg_last_error()
    assert L.vqseg_boundary_seeds_u8(one, 1, 2049, 4, 3, 0, 0, 0, 0, 0, one, None) == -1 and b"2048" in L.vqseg_last_error()
    assert L.vqseg_boundary_seeds_i32(one, 1, 4, 4, 33, 0, 0, 0, 0, 0, one, None) == -1 and b"1..32" in L.vqseg_last_error()
    assert L.vqseg_boundary_seeds_i32(one, 1, 4, 4, 3, 5, 0, 0, 0, 0, one, None) == -1 and b"ignored values" in L.vqseg_last_error()
    assert L.vqseg_boundary_seeds_u8(one, (1 << 19) // 2 + 1, 4, 4, 2, 0, 0, 0, 0, 0, one, None) == -1 and b"2^19" in L.vqseg_last_error()
    assert L.vqseg_boundary_edt_rows_u8(one, 1, 4, 4, None, one, None) == -1 and b"null" in L.vqseg_last_error()
    assert L.vqseg_boundary_edt_rows_u8(one, 0, 4, 4, one, one, None) == -1 and b"positive" in L.vqseg_last_error()
    assert L.vqseg_boundary_edt_cols_i32(one, one, 1, 4, 2049, one, None) == -1 and b"2048" in L.vqseg_last_error()
    assert L.vqseg_boundary_edt_cols_i32(one, one, (1 << 19) + 1, 4, 4, one, None) == -1 and b"2^19" in L.vqseg_last_error()
    assert L.vqseg_boundary_counts_i32(one, 2, one, 1, one, one, one, one, 1, 4, 4, 3, 4, 4, 0, 0, 0, 0, 0, one, None) == -1 and \
        b"pred_bytes" in L.vqseg_last_error()
    assert L.vqseg_boundary_counts_i32(one, 1, one, 4, one, one, one, one, 1, 4, 4, 3, -1, 4, 0, 0, 0, 0, 0, one, None) == -1 and \
        b"tol_sq" in L.vqseg_last_error()
    assert L.vqseg_boundary_counts_i32(one, 1, one, 4, one, one, one, one, 1, 4, 4, 3, 4, 2 ** 31 - 1, 0, 0, 0, 0, 0, one, None) == -1
    assert L.vqseg_boundary_counts_i32(one, 1, one, 4, one, one, one, None, 1, 4, 4, 3, 4, 4, 0, 0, 0, 0, 0, one, None) == -1 and \
        b"null" in L.vqseg_last_error()


def test_utils_and_test_loop_refuse_bad_boundary_options():
    from vq_seg_amd.evaluate import test_loop
    u8 = np.zeros((1, 4, 4), dtype=np.uint8)
    for kw, msg in ((dict(tolerance=-1), "tolerance must be"), (dict(tolerance=float("nan")), "tolerance must be"),
                    (dict(tolerance=1e6), "tolerance must be"), (dict(width="2"), "width must be"), (dict(ignore=(1, 2, 3, 4, 5)), "ignore must be")):
        with pytest.raises(ValueError, match=msg):
            boundary.boundary_stats(u8, u8, 3, **kw)
        with pytest.raises(ValueError, match=msg):
            boundary.BoundaryMeasurement(3, **kw)
    with pytest.raises(ValueError, match="num_classes must be an integer in 1..32"):
        boundary.BoundaryMeasurement(33)
    with pytest.raises(ValueError, match="one shape"):
        boundary.boundary_stats(u8, np.zeros((1, 4, 5), dtype=np.uint8), 3)
    with pytest.raises(ValueError, match="an integer map"):
        boundary.boundary_stats(u8.astype(np.float32), u8, 3)
    with pytest.raises(ValueError, match="uint8 or bool mask"):
        boundary.distance_transform(np.zeros((4, 4), dtype=np.int32))
    net = torch.nn.Conv2d(3, 3, 1)
    with pytest.raises(ValueError, match="boundary needs fused=True"):
        test_loop(net, [], 3, boundary=True)
    with pytest.raises(ValueError, match="boundary needs fused=True"):
        test_loop(net, [], 3, boundary=dict(tolerance=3))
    with pytest.raises(ValueError, match="boundary is None, True or a dict"):
        test_loop(net, [], 3, fused=True, boundary=dict(tol=3))
    with pytest.raises(ValueError, match="boundary is None, True or a dict"):
        test_loop(net, [], 3, fused=True, boundary=2.0)
    with pytest.raises(ValueError, match="tolerance must be"):
        test_loop(net, [], 3, fused=True, boundary=dict(tolerance=-2))
    import inspect

    from vq_seg_amd.trainer import CPSTrainer
    assert inspect.signature(CPSTrainer.evaluate).parameters["boundary"].default is None
    assert inspect.signature(test_loop).parameters["boundary"].default is None
