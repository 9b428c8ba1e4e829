"""The panel-sheet kernel (vqseg_render_sheet_u8 through nnf.render_sheet / _hip.render_sheet) on the GPU against the fp64 restatement
of tests/visualize_cases.py, under the rule stated there: palette-row bytes equal, image / mix bytes one level off only where the oracle's
pre-floor value is within 1e-3 of an integer, and at most 1 % of a panel's values that near.  Every case is a few launches on a few
hundred pixels; the grid-stride case is one launch."""
import os

import numpy as np
import pytest
import torch

from tests import predict_cases as P
from tests import visualize_cases as VC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE = ["image", "target", "pred", "detail", "mix_pred", "mix_detail", ("fill", 6)]


def render(panels, size, c, image, pred, target, layout="nchw", half=False, alpha=0.4, fill=(1.0, 1.0, 1.0)):
    from vq_seg_amd import nnf
    return nnf.render_sheet(panels, size, c, VC.palette(c), image=P.lay(image.to(DEV), layout), pred=pred.to(DEV), target=target.to(DEV), fill=fill,
                            alpha=alpha, half=half).cpu().numpy()


def run_case(c, src, size, target_size, half, layouts=P.LAYOUTS):
    image, pred, target = VC.sources(c, src, size, target_size, special=True)
    for panels in [[k] for k in SINGLE] + [VC.FIVE]:
        needs_image = any(k in ("image", "mix_pred", "mix_detail") for k in panels)
        for layout in (layouts if needs_image else layouts[:1]):
            what = (c, src, size, target_size, half, layout, panels)
            fill = (1.0, 1.0, 1.0) if panels is VC.FIVE else (230 / 255, 0.25, 0.0)
            got = render(panels, size, c, image, pred, target, layout, half, fill=fill)
            value, exact = VC.oracle(panels, size, c, image.numpy(), pred.numpy(), target.numpy(), fill=fill, box2=half)
            VC.check(got, value, exact, what, panels, size[1], 2 if half else 1)


@pytest.mark.parametrize("c", [2, 3, 4])
@pytest.mark.parametrize("case", VC.SHAPES, ids=VC.IDS)
def test_every_panel_kind_and_the_five_panel_sheet(case, c):
    """targets containing 255 and a negative label, pred bytes >= C, a NaN and a value above 1 in the image; planar and channels_last"""
    from vq_seg_amd import _hip
    before = _hip.RENDER_SHEET_CALLS
    run_case(c, case[0], case[1], None, False)
    assert _hip.RENDER_SHEET_CALLS > before


@pytest.mark.parametrize("case", VC.SHAPES, ids=VC.IDS)
def test_target_at_its_own_size_is_brought_over_by_nearest_neighbour(case):
    run_case(3, case[0], case[1], VC.TARGET_OWN, False, layouts=P.LAYOUTS[:1])


@pytest.mark.parametrize("c", [2, 3, 4])
@pytest.mark.parametrize("case", VC.SHAPES, ids=VC.IDS)
def test_box2_is_the_mean_of_2x2_float_colours(case, c):
    """all three display sizes give even sheets (2 x 33 rows: a 2 x 2 block straddles the two images)"""
    run_case(c, case[0], case[1], None if c != 3 else VC.TARGET_OWN, True, layouts=P.LAYOUTS[c % 2:][:1])


def test_box2_blocks_that_straddle_two_panels():
    """an odd display width puts the panel edge inside a 2 x 2 block: each of its pixels takes its own panel's colour"""
    c, src, size = 3, (6, 10), (12, 21)
    image, pred, target = VC.sources(c, src, size, None, special=True)
    for panels in (["image", "mix_pred"], ["target", "detail"], ["pred", ("fill", 3), "mix_detail", "image"]):
        got = render(panels, size, c, image, pred, target, half=True)
        value, exact = VC.oracle(panels, size, c, image.numpy(), pred.numpy(), target.numpy(), box2=True)
        VC.check(got, value, exact, panels)


@pytest.mark.parametrize("half", [False, True], ids=["full", "box2"])
def test_canvas_as_a_view_of_a_larger_buffer(half):
    """pitch above the row bytes, the sheet at a byte offset of 1 (the byte-store path), panels that leave a hole and a margin: bytes outside
    the panels keep 0xAB, bytes inside equal the aligned run's, which equal the oracle's"""
    from vq_seg_amd import _hip
    c, (src, size) = 3, VC.SHAPES[1]
    wo = size[1]
    image, pred, target = (t.to(DEV) for t in VC.sources(c, src, size, None, special=True))
    hole, margin = 4, 2
    lay = [("mix_detail", wo + hole, wo), ("image", 0, wo)]                # given out of order: the entry point sorts
    cols = 2 * wo + hole + margin
    k = 2 if half else 1
    rows, ocols = VC.B * size[0] // k, cols // k
    pitch = 3 * ocols + 5
    buf = torch.full((1 + (rows + 1) * pitch,), 0xAB, dtype=torch.uint8, device=DEV)
    view = torch.as_strided(buf, (rows, ocols, 3), (pitch, 3, 1), 1)
    assert view.data_ptr() % 4 == 1
    _hip.render_sheet(view, lay, (VC.B,) + size, c, VC.palette(c), image=image, pred=pred, target=target, box2=half, cols=cols)
    apitch = (3 * ocols + 3) // 4 * 4                                       # the aligned run: base and pitch multiples of 4 (the 4-byte stores)
    dense = torch.as_strided(torch.full((rows * apitch,), 0xAB, dtype=torch.uint8, device=DEV), (rows, ocols, 3), (apitch, 3, 1), 0)
    assert dense.data_ptr() % 4 == 0 and dense.stride(0) % 4 == 0
    _hip.render_sheet(dense, lay, (VC.B,) + size, c, VC.palette(c), image=image, pred=pred, target=target, box2=half, cols=cols)
    got, aligned, raw = view.cpu().numpy(), dense.cpu().numpy(), buf.cpu().numpy()
    assert np.array_equal(got, aligned)
    inside = np.zeros((rows, ocols), dtype=bool)
    inside[:, :wo // k] = True
    inside[:, (wo + hole) // k:(2 * wo + hole) // k] = True
    assert (got[~inside] == 0xAB).all()
    untouched = np.ones(raw.shape, dtype=bool)                              # every byte of the buffer that is no panel pixel
    idx = 1 + np.arange(rows)[:, None, None] * pitch + np.arange(ocols)[None, :, None] * 3 + np.arange(3)[None, None, :]
    untouched[idx[inside]] = False
    assert (raw[untouched] == 0xAB).all()
    panels = ["image", ("fill", hole), "mix_detail", ("fill", margin)]
    value, exact = VC.oracle(panels, size, c, image.cpu().numpy(), pred.cpu().numpy(), target.cpu().numpy(), box2=half)
    VC.check(got[:, :wo // k], value[:, :wo // k], exact[:, :wo // k], "image panel")
    VC.check(got[:, (wo + hole) // k:(2 * wo + hole) // k], value[:, (wo + hole) // k:(2 * wo + hole) // k], exact[:, (wo + hole) // k:(2 * wo + hole) // k], "mix")


def test_grid_stride_loop():
    """nn_grid_cap = 256 under a sheet of 381 workgroups"""
    from vq_seg_amd import _hip
    c, src, size = 3, (16, 64), (160, 300)
    image, pred, target = VC.sources(c, src, size, None, special=True)
    before = _hip.lib().vqseg_set_option(b"nn_grid_cap", 256)
    try:
        got = render(VC.FIVE, size, c, image, pred, target)
    finally:
        _hip.lib().vqseg_set_option(b"nn_grid_cap", before)
    assert got.shape[0] * ((got.shape[1] + 3) // 4) > 256 * 256
    value, exact = VC.oracle(VC.FIVE, size, c, image.numpy(), pred.numpy(), target.numpy())
    VC.check(got, value, exact, "grid stride", VC.FIVE, size[1])


def test_entry_point_refuses_bad_arguments_on_the_gpu_too():
    from vq_seg_amd import _hip, nnf
    image, pred, target = (t.to(DEV) for t in VC.sources(3, (6, 10), (12, 20)))
    with pytest.raises(_hip.HipLibraryError, match="overlapping panels"):
        _hip.render_sheet(torch.zeros((24, 40, 3), dtype=torch.uint8, device=DEV), [("pred", 0, 20), ("pred", 19, 20)], (2, 12, 20), 3, VC.palette(3), pred=pred)
    with pytest.raises(_hip.HipLibraryError, match="needs the target"):
        nnf.render_sheet(["detail"], (12, 20), 3, VC.palette(3), pred=pred)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        nnf.render_sheet(["image", "pred"], (12, 20), 3, VC.palette(3), image=image.cpu(), pred=pred)


def test_reference_names_on_device_tensors_equal_the_golden_bytes():
    from vq_seg_amd.utils import visualize as V
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "visualize_ref.npz")))
    t = {k: torch.from_numpy(v).to(DEV) for k, v in g.items() if k in ("l_input", "ul_input", "pred", "ul_pred", "target")}
    w = 10
    exact = np.zeros((12, 60), dtype=bool)
    exact[:, w:3 * w + VC.GAP] = True                                      # target | pred | gap
    got = V.make_example_img(t["l_input"], t["target"], t["pred"], t["ul_input"], t["ul_pred"], resize_factor=None)
    VC.check(got, g["example"], exact, "make_example_img")
    full = g["example"]
    mean = (full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2]) / 4
    VC.check(V.make_example_img(t["l_input"], t["target"], t["pred"], t["ul_input"], t["ul_pred"]), mean, np.zeros((6, 30), dtype=bool), "half")
    VC.check(V.make_example_img(t["l_input"], t["target"], t["pred"], None, None), g["example_labelled"], exact[:, :3 * w], "labelled")
    for fn, names, cm in ((V.make_test_img, ("test_v1", "test_v2"), g["detail_colormap"][:3]),
                          (V.make_test_detailed_img, ("detail_v1", "detail_v2"), g["detail_colormap"])):
        v1, v2 = fn(t["l_input"], t["pred"], t["target"], colormap=cm)
        VC.check(v1, g[names[0]], exact[:, :3 * w], names[0])
        VC.check(v2, g[names[1]], np.zeros((12, w), dtype=bool), names[1])
    assert np.array_equal(V.pred_to_colormap(t["pred"], g["detail_colormap"][:3]), np.floor(g["pred_colormap"] * 255).astype(np.uint8))
