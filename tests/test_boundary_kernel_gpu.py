"""The boundary kernels (csrc/boundary_kernels.hip) against the plain restatement of tests/boundary_cases.py: boundaries, squared
distances and the count table on every case and every tolerance / width setting, for uint8 and int64 maps -- exact integer equality,
nothing has a tolerance.  Then what equality on one call cannot show: two calls, an image alone against the image in its batch, the
chunked path, and the guard bands of tests/extent.py around each of the four launches."""
import numpy as np
import pytest
import torch

from tests import boundary_cases as bc
from tests import extent as E
from vq_seg_amd import _hip, nnf
from vq_seg_amd.utils import boundary

pytestmark = pytest.mark.gpu

DTYPES = {"u8": torch.uint8, "i64": torch.int64}
C = bc.NUM_CLASSES


def dev():
    return torch.device("cuda:0")


def same(t, want):
    return np.array_equal(t.cpu().numpy(), want)


def differing(t, want):
    return f"{int((t.cpu().numpy() != want).sum())} entries differ"


def maps(name, dtype=torch.uint8):
    ref = bc.reference(name)
    return ref, torch.from_numpy(ref["pred"].copy()).to(dtype).to(dev()), torch.from_numpy(ref["target"].copy()).to(dtype).to(dev())


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name", bc.CASES)
def test_kernels_equal_the_restatement(name, dtype):
    ref, p, t = maps(name, DTYPES[dtype])
    assert nnf.boundaries_supported(p)
    bp, bg = nnf.class_boundaries(p, C, bc.IGNORE), nnf.class_boundaries(t, C, bc.IGNORE)
    assert bp.dtype == torch.uint8 and same(bp, ref["bp"]) and same(bg, ref["bg"]), "boundaries: " + differing(bp, ref["bp"])
    dp, dg = nnf.edt_sq(bp), nnf.edt_sq(bg)
    assert dp.dtype == torch.int32 and tuple(dp.shape) == tuple(bp.shape)
    assert same(dp, ref["dp"]), "dp: " + differing(dp, ref["dp"])
    assert same(dg, ref["dg"]), "dg: " + differing(dg, ref["dg"])
    for tol, width in bc.SETTINGS:
        table = nnf.boundary_counts(p, t, C, bc.squared(tol), bc.squared(width), bc.IGNORE)
        want = bc.reference_counts(name, tol, width)
        assert table.dtype == torch.int32 and same(table, want), f"table at {(tol, width)}: {table.cpu().numpy().tolist()} against {want.tolist()}"


@pytest.mark.parametrize("name", sorted(bc.SEED_PLANES))
def test_seed_planes(name):
    s, d = bc.seed_plane(name)
    got = nnf.edt_sq(torch.from_numpy(s.copy()).to(dev()))
    assert same(got, d), differing(got, d)
    if name == "lone-first":
        assert int(got[256, 258]) == 132100
    as_bool = nnf.edt_sq(torch.from_numpy(s.copy()).bool().to(dev())[None, None])          # bool, and two leading dimensions
    assert tuple(as_bool.shape) == (1, 1) + s.shape and same(as_bool[0, 0], d)


def test_planes_are_independent_and_an_empty_plane_reads_none():
    planes = np.stack([bc.seed_plane("first-and-last-row")[0], np.zeros((300, 5), dtype=np.uint8), bc.first_and_last_row(300, 5)[::-1].copy()])
    got = nnf.edt_sq(torch.from_numpy(planes).to(dev()))
    assert same(got, bc.edt_sq(planes)) and bool((got[1] == nnf.EDT_NONE).all())


def test_the_public_surface_takes_the_kernels():
    ref, p, t = maps("batch", torch.int64)
    before = nnf.BOUNDARY_CALLS
    st = boundary.boundary_stats(p, t, C, tolerance=2, width=3)
    assert nnf.BOUNDARY_CALLS == before + 1 and st.table.is_cuda and same(st.table, bc.reference_counts("batch", 2, 3))
    sc = bc.scores(bc.reference_counts("batch", 2, 3))
    for key in ("f1", "precision", "recall", "iou", "hausdorff"):
        assert np.array_equal(getattr(st, key), sc[key], equal_nan=True), key
    assert same(boundary.class_boundaries(p, C), ref["bp"])
    d = boundary.distance_transform(torch.from_numpy(ref["bg"].copy()).to(dev()), squared=True)
    assert d.is_cuda and same(d, ref["dg"])
    root = boundary.distance_transform(torch.from_numpy(ref["bg"].copy()).to(dev()))
    assert root.dtype == torch.float32 and same(root, np.sqrt(ref["dg"].astype(np.float32)))
    # an element type the kernels do not take: the torch-op form on the device, the same numbers
    st16 = boundary.boundary_stats(p.to(torch.int16), t.to(torch.int16), C, tolerance=2, width=3)
    assert nnf.BOUNDARY_CALLS == before + 1 and same(st16.table, bc.reference_counts("batch", 2, 3))
    m = boundary.BoundaryMeasurement(C, tolerance=2, width=3)
    m.update(p[:1], t[:1])
    m.update(p[1:], t[1:])
    assert np.array_equal(m.table(), bc.reference_counts("batch", 2, 3))


@pytest.mark.parametrize("name", ["batch", "random41v50-67x259", "spiral-67x259"])
def test_two_calls_agree_bit_for_bit(name):
    _, p, t = maps(name)
    for _ in range(2):
        a = (nnf.class_boundaries(p, C, bc.IGNORE), nnf.edt_sq(nnf.class_boundaries(p, C, bc.IGNORE)), nnf.boundary_counts(p, t, C, 4, 9, bc.IGNORE))
        b = (nnf.class_boundaries(p, C, bc.IGNORE), nnf.edt_sq(nnf.class_boundaries(p, C, bc.IGNORE)), nnf.boundary_counts(p, t, C, 4, 9, bc.IGNORE))
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_an_image_alone_equals_the_image_in_its_batch(monkeypatch):
    _, p, t = maps("batch")
    whole = nnf.boundary_counts(p, t, C, 4, 9, bc.IGNORE)
    whole_d = nnf.edt_sq(nnf.class_boundaries(p, C, bc.IGNORE))
    for k in range(p.shape[0]):
        alone = nnf.boundary_counts(p[k:k + 1].contiguous(), t[k:k + 1].contiguous(), C, 4, 9, bc.IGNORE)
        assert torch.equal(alone[0], whole[k]), k
        assert torch.equal(nnf.edt_sq(nnf.class_boundaries(p[k:k + 1].contiguous(), C, bc.IGNORE))[0], whole_d[k]), k
    # the chunked path: a workspace limit that admits two images per chunk gives the same table
    monkeypatch.setattr(nnf, "BOUNDARY_WORKSPACE_BYTES", 2 * (2 * C * 40 * 72 * 4) + 1)
    assert nnf.boundary_chunk(C, 40, 72) == 2
    assert torch.equal(nnf.boundary_counts(p, t, C, 4, 9, bc.IGNORE), whole)


# ------------------------------------------------------------------------------------------------------------------------------
# guard bands (tests/extent.py): each of the four launches, called through the library itself, on a ragged case
# ------------------------------------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr()


EXTENT = ["random41v50-1x1", "random41v50-67x259", "batch"]


@pytest.mark.parametrize("name", EXTENT)
def test_extent_seeds(name):
    L = _hip.lib()
    ref = bc.reference(name)
    v = torch.from_numpy(ref["target"].copy())
    b, h, w = v.shape
    for kind, tdt in (("u8", torch.uint8), ("i32", torch.int32)):
        fn = getattr(L, f"vqseg_boundary_seeds_{kind}")
        spec = dict(labels=E.In(v.to(tdt), align=1), seeds=E.Out((b, C, h, w), torch.uint8, align=1))
        _, a, _ = E.run_case(spec, lambda t: fn(_p(t["labels"]), b, h, w, C, 1, 255, 0, 0, 0, _p(t["seeds"]), _stream()),
                             dev(), torch.cuda.synchronize, f"boundary_seeds_{kind} {name}")
        assert same(a["seeds"], ref["bg"])


@pytest.mark.parametrize("name", EXTENT)
def test_extent_rows_and_columns(name):
    L = _hip.lib()
    ref = bc.reference(name)
    seeds = torch.from_numpy(ref["bg"].copy())
    b, c, h, w = seeds.shape
    planes = b * c
    spec = dict(seeds=E.In(seeds, align=1), g=E.Out((planes, h, w), torch.int16, align=2), row_has=E.Out((planes, h), torch.uint8, align=1))
    _, a, _ = E.run_case(spec, lambda t: L.vqseg_boundary_edt_rows_u8(_p(t["seeds"]), planes, h, w, _p(t["g"]), _p(t["row_has"]), _stream()),
                         dev(), torch.cuda.synchronize, f"boundary_edt_rows {name}")
    has = ref["bg"].reshape(planes, h, w).any(axis=2)
    assert same(a["row_has"], has.astype(np.uint8))
    g = a["g"].cpu().numpy().view(np.uint16).astype(np.int64)
    assert (g[~has] == 0xffff).all()
    xs = np.arange(w)
    for pl, y in zip(*np.nonzero(has)):                                      # the distance along the row, by brute force
        at = np.nonzero(ref["bg"].reshape(planes, h, w)[pl, y])[0]
        assert np.array_equal(g[pl, y], np.abs(xs[:, None] - at[None, :]).min(axis=1)), (pl, y)
    spec = dict(g=E.In(a["g"].cpu(), align=2), row_has=E.In(a["row_has"].cpu(), align=1), d2=E.Out((planes, h, w), torch.int32, align=4))
    _, a2, _ = E.run_case(spec, lambda t: L.vqseg_boundary_edt_cols_i32(_p(t["g"]), _p(t["row_has"]), planes, h, w, _p(t["d2"]), _stream()),
                          dev(), torch.cuda.synchronize, f"boundary_edt_cols {name}")
    assert same(a2["d2"].view(b, c, h, w), ref["dg"])


@pytest.mark.parametrize("name", EXTENT)
def test_extent_counts(name):
    L = _hip.lib()
    ref = bc.reference(name)
    b, c, h, w = ref["bp"].shape
    pred, target = torch.from_numpy(ref["pred"].copy()), torch.from_numpy(ref["target"].copy())
    for pt, tt in ((torch.uint8, torch.int32), (torch.int32, torch.uint8)):
        spec = dict(pred=E.In(pred.to(pt), align=1), target=E.In(target.to(tt), align=1), bp=E.In(torch.from_numpy(ref["bp"].copy()), align=1),
                    bg=E.In(torch.from_numpy(ref["bg"].copy()), align=1), dp=E.In(torch.from_numpy(ref["dp"].copy()), align=4),
                    dg=E.In(torch.from_numpy(ref["dg"].copy()), align=4), table=E.Out((b, c, 8), torch.int32, align=4))
        pb, tb = (1 if pt == torch.uint8 else 4), (1 if tt == torch.uint8 else 4)
        _, a, _ = E.run_case(spec, lambda t: L.vqseg_boundary_counts_i32(_p(t["pred"]), pb, _p(t["target"]), tb, _p(t["bp"]), _p(t["bg"]), _p(t["dp"]),
                                                                         _p(t["dg"]), b, h, w, c, 12, 12, 1, 255, 0, 0, 0, _p(t["table"]), _stream()),
                             dev(), torch.cuda.synchronize, f"boundary_counts {name}")
        assert same(a["table"], bc.reference_counts(name, 3.5, 3.5))
