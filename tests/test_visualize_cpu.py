"""The visualisation path without a GPU: the numpy path of vq_seg_amd.utils.visualize against the reference's recorded float outputs
(tests/golden/visualize_ref.npz, written by tools/capture_visualize_golden.py; a byte is floor(x * 255), what plt.imsave writes) and
against the fp64 restatement of tests/visualize_cases.py, the 2 x 2 box mean of resize_factor=0.5, the argument errors, the PNG round
trip, the argument checks of vqseg_render_sheet_u8 (pure host code) and of its wrappers, and Predictor.render / CPSTrainer-free
test_loop(visualize=...) on a stub network."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import predict_cases as P
from tests import visualize_cases as VC
from vq_seg_amd import _hip, nnf
from vq_seg_amd.utils import visualize as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "visualize_ref.npz")))


def q(x):
    return np.floor(np.asarray(x, dtype=np.float64) * 255).astype(np.uint8)


def same_as_golden(got, want_float, what):
    """the numpy path follows the reference's float64 arithmetic expression by expression: its bytes are floor(golden * 255), and the
    rule of tests/visualize_cases.py (one level where the pre-floor value is within 1e-3 of an integer) is never needed"""
    assert got.dtype == np.uint8 and got.shape == want_float.shape, (what, got.dtype, got.shape)
    VC.check(got, want_float, np.zeros(want_float.shape[:-1], dtype=bool), what)
    assert np.array_equal(got, q(want_float)), what


def test_numpy_path_equals_the_reference_outputs(golden):
    g = golden
    same_as_golden(V.make_example_img(g["l_input"], g["target"], g["pred"], g["ul_input"], g["ul_pred"], resize_factor=None), g["example"], "example")
    same_as_golden(V.make_example_img(g["l_input"], g["target"], g["pred"], None, None), g["example_labelled"], "labelled only")
    for fn, names in ((V.make_test_img, ("test_v1", "test_v2")), (V.make_test_detailed_img, ("detail_v1", "detail_v2"))):
        cm = g["detail_colormap"] if fn is V.make_test_detailed_img else g["detail_colormap"][:3]
        v1, v2 = fn(g["l_input"], g["pred"], g["target"], colormap=cm)
        same_as_golden(v1, g[names[0]], names[0])
        same_as_golden(v2, g[names[1]], names[1])
    same_as_golden(V.pred_to_colormap(g["pred"], g["detail_colormap"][:3]), g["pred_colormap"], "pred_to_colormap")
    # CPU tensors take the same path as numpy arrays
    t = {k: torch.from_numpy(v) for k, v in g.items()}
    same_as_golden(V.make_example_img(t["l_input"], t["target"], t["pred"], t["ul_input"], t["ul_pred"], resize_factor=None), g["example"], "tensors")
    # the pieces
    assert np.array_equal(V.target_to_colormap(g["target"], g["detail_colormap"][:3]), q(g["detail_colormap"][:3][g["target"]]))
    wrong = np.argmax(g["pred"], axis=1) != g["target"]
    want = g["detail_colormap"][np.argmax(g["pred"], axis=1) + 3 * wrong]
    assert np.array_equal(V.pred_to_detailed_colormap(g["pred"], g["target"], g["detail_colormap"]), q(want))
    assert np.array_equal(V.batch_to_grid(g["l_input"]), g["l_input"].transpose(0, 2, 3, 1).reshape(-1, 10, 3))
    a, b = g["l_input"].transpose(0, 2, 3, 1)[0], g["detail_colormap"][g["target"][0]]
    assert np.array_equal(V.mix_input_pred(a, b), q(np.clip(a * (1 - 0.4) + b * 0.4, 0, 1)))
    assert V.DEFAULT_PALETTE.shape == (7, 3) and np.array_equal(V.DEFAULT_PALETTE[:6], g["detail_colormap"])
    assert q(V.DEFAULT_PALETTE)[4].tolist() == [230, 145, 56]     # in float64; float32(230 / 255) * 255 floors to 229


def test_resize_factor_half_is_the_2x2_box_mean(golden):
    g = golden
    full = g["example"]                                           # (12, 60, 3) float64
    mean = np.zeros((6, 30, 3))
    for i in range(6):
        for j in range(30):
            mean[i, j] = (full[2 * i, 2 * j] + full[2 * i, 2 * j + 1] + full[2 * i + 1, 2 * j] + full[2 * i + 1, 2 * j + 1]) / 4
    for factor in (0.5, "default"):
        kw = {} if factor == "default" else {"resize_factor": factor}
        got = V.make_example_img(g["l_input"], g["target"], g["pred"], g["ul_input"], g["ul_pred"], **kw)
        VC.check(got, mean, np.zeros((6, 30), dtype=bool), f"half {factor}")


def test_argument_errors(golden):
    g = golden
    args = (g["l_input"], g["target"], g["pred"], g["ul_input"], g["ul_pred"])
    for bad in (0.25, 1.0, 2):
        with pytest.raises(NotImplementedError, match="resize_factor"):
            V.make_example_img(*args, resize_factor=bad)
    odd = [a[:, ..., :5, :] for a in args]                        # 2 x 5 = 10 rows: even; one image of 5 rows: odd
    with pytest.raises(ValueError, match="even height and width"):
        V.make_example_img(*[a[:1] for a in odd])
    assert V.make_example_img(*odd).shape == (5, 30, 3)
    with pytest.raises(ValueError, match="one shape"):
        V.make_example_img(g["l_input"], g["target"], g["pred"], g["ul_input"][:1], g["ul_pred"][:1])
    with pytest.raises(ValueError, match="colormap"):
        V.pred_to_colormap(g["pred"], g["detail_colormap"][:2])
    with pytest.raises(ValueError, match="2..4"):
        V.default_palette(5)
    with pytest.raises(_hip.HipLibraryError, match="panel kinds"):
        V.render_sheet(["overlay"], g["l_input"])
    with pytest.raises(_hip.HipLibraryError, match="fill"):
        V.render_sheet([("fill", 0)], g["l_input"])
    with pytest.raises(ValueError, match="needs a source"):
        V.render_sheet(["image", "target"], g["l_input"])
    with pytest.raises(ValueError, match="display size"):
        V.render_sheet(["pred"], logits_or_label=g["target"], size=(3, 3))


def test_numpy_path_equals_the_restatement_on_special_values():
    """255 among the targets, a pred byte >= C, a NaN and a value above 1 in the image, a target at its own size, all seven kinds"""
    for c in (2, 3, 4):
        (src, size) = VC.SHAPES[0]
        image, pred, target = VC.sources(c, src, size, VC.TARGET_OWN, special=True)
        panels = ["image", "target", "pred", "detail", ("fill", 8), "mix_pred", "mix_detail"]
        for half in (False, True):
            got = V.render_sheet(panels, image, pred, target, size=size, num_classes=c, half=half).numpy()
            value, exact = VC.oracle(panels, size, c, image.numpy(), pred.numpy(), target.numpy(), box2=half)
            VC.check(got, value, exact, (c, half))


def test_near_integer_share_of_uniform_images_is_small():
    """the condition on the inputs that the GPU tests assert per panel: uniform float32 images put about 0.2 % of a panel's values within
    1e-3 of an integer; k / 255 images would put every one there"""
    g = torch.Generator().manual_seed(5)
    image = torch.rand((2, 3, 64, 64), generator=g).numpy()
    value, _ = VC.oracle(["image"], (128, 128), 3, image)
    share = VC.near_integer(value).mean()
    assert 0.0005 < share < 0.004, share
    grid = np.round(image * 255) / 255
    assert VC.near_integer(VC.oracle(["image"], (64, 64), 3, grid)[0]).mean() > 0.99


def test_save_img_round_trip(tmp_path, golden):
    from PIL import Image
    g = golden
    sheet = V.make_example_img(g["l_input"], g["target"], g["pred"], g["ul_input"], g["ul_pred"])
    V.save_img(str(tmp_path), "sheet.png", sheet)
    back = np.array(Image.open(tmp_path / "sheet.png"))
    assert back.dtype == np.uint8 and back.shape == sheet.shape and (back == sheet).all()
    V.save_img(str(tmp_path), "float.png", g["example"])          # the reference's float sheet: quantised as plt.imsave does
    assert (np.array(Image.open(tmp_path / "float.png")) == q(g["example"])).all()
    V.save_img_list(str(tmp_path), ["a.png", "b.png"], [sheet, sheet[:, :10]])
    assert (np.array(Image.open(tmp_path / "b.png")) == sheet[:, :10]).all()


# ---------------------------------------------------------------------------------------------------------------------------
# vqseg_render_sheet_u8: the argument checks are host code and run before anything touches a device
# ---------------------------------------------------------------------------------------------------------------------------
def test_render_sheet_entry_point_refuses_bad_arguments_without_a_gpu():
    L = _hip.lib()
    keep = []

    def arr(values, ctype):
        a = (ctype * len(values))(*values)
        keep.append(a)
        return ctypes.cast(a, ctypes.c_void_p)

    def call(c=3, kinds=(0, 1, 2), x0=(0, 20, 40), width=(20, 20, 20), b=2, ho=12, wo=20, rows=24, cols=60, box2=0, pitch=180, canvas=64,
             image=64, pred=64, target=64, n=None):
        pal_f, pal_u = arr([0.0] * 27, ctypes.c_float), arr([0] * 27, ctypes.c_uint8)
        return L.vqseg_render_sheet_u8(image or None, 3 * 6 * 10, 60, 1, 6, 10, pred or None, target or None, 12, 20, b, ho, wo, c, arr(kinds, ctypes.c_int),
                                       arr(x0, ctypes.c_int), arr(width, ctypes.c_int), len(kinds) if n is None else n, pal_f, pal_u, pal_f, pal_u,
                                       0.4, box2, canvas or None, pitch, rows, cols, None)

    for kw, msg in [
        (dict(canvas=0), b"null canvas"),
        (dict(kinds=(0, 7, 2)), b"panel kind"),
        (dict(kinds=(0, -1, 2)), b"panel kind"),
        (dict(c=1), b"2..4 classes"),
        (dict(c=5), b"2..4 classes"),
        (dict(kinds=(6,) * 9, x0=tuple(range(9)), width=(1,) * 9), b"1..8 panels"),
        (dict(n=0), b"1..8 panels"),
        (dict(x0=(0, 20, 41)), b"outside the canvas"),
        (dict(x0=(0, 19, 40)), b"overlapping panels"),
        (dict(x0=(40, 0, 19)), b"overlapping panels"),             # in any order
        (dict(image=0), b"needs the image"),
        (dict(kinds=(4,), x0=(0,), width=(20,), pred=0), b"needs pred"),
        (dict(kinds=(3,), x0=(0,), width=(20,), target=0), b"needs the target"),
        (dict(box2=1, b=1, ho=11, rows=11), b"even height and width"),
        (dict(box2=1, cols=61), b"even height and width"),
        (dict(box2=1, kinds=(6, 6), x0=(0, 4), width=(3, 2)), b"odd column"),
        (dict(pitch=179), b"pitch smaller"),
        (dict(box2=1, pitch=89), b"pitch smaller"),
        (dict(rows=25), b"rows must be b * ho"),
        (dict(width=(20, 19, 20)), b"wo wide"),
    ]:
        assert call(**kw) == -1, kw
        err = L.vqseg_last_error()
        assert msg in err and err.startswith(b"render_sheet:"), (kw, err)


def test_render_sheet_wrappers_check_before_the_device():
    E = _hip.HipLibraryError
    image, pred, target = VC.sources(3, (6, 10), (12, 20))
    pal = VC.palette(3)
    canvas = torch.zeros((24, 60, 3), dtype=torch.uint8)
    lay = [("image", 0, 20), ("target", 20, 20), ("pred", 40, 20)]
    with pytest.raises(E, match="no CPU fallback"):                # everything right but the device
        _hip.render_sheet(canvas, lay, (2, 12, 20), 3, pal, image=image, pred=pred, target=target)
    with pytest.raises(E, match="no CPU fallback"):
        nnf.render_sheet(["image", "target", "pred"], (12, 20), 3, pal, image=image, pred=pred, target=target)
    with pytest.raises(E, match="pred: expected torch.uint8"):
        _hip.render_sheet(canvas, lay, (2, 12, 20), 3, pal, image=image, pred=pred.long(), target=target)
    with pytest.raises(E, match="image: expected torch.float32"):
        _hip.render_sheet(canvas, lay, (2, 12, 20), 3, pal, image=image.double(), pred=pred, target=target)
    with pytest.raises(E, match="target: expected torch.int64"):
        _hip.render_sheet(canvas, lay, (2, 12, 20), 3, pal, image=image, pred=pred, target=target.int())
    with pytest.raises(E, match="pred must have the shape"):
        _hip.render_sheet(canvas, lay, (2, 12, 20), 3, pal, image=image, pred=pred[:, :11], target=target)
    with pytest.raises(E, match="needs a canvas of"):
        _hip.render_sheet(canvas[:, :59], lay, (2, 12, 20), 3, pal, image=image, pred=pred, target=target, cols=60)
    with pytest.raises(E, match="dense RGB bytes"):
        _hip.render_sheet(torch.zeros((24, 120, 3), dtype=torch.uint8)[:, ::2], lay, (2, 12, 20), 3, pal, image=image, pred=pred, target=target)
    with pytest.raises(E, match="canvas: expected a uint8"):
        _hip.render_sheet(canvas.float(), lay, (2, 12, 20), 3, pal, image=image, pred=pred, target=target)
    with pytest.raises(E, match="7 rows of 3"):
        _hip.render_sheet(canvas, lay, (2, 12, 20), 3, pal[:6], image=image, pred=pred, target=target)
    with pytest.raises(E, match="even height and width"):
        nnf.render_sheet(["pred"], (11, 20), 3, pal, pred=pred[:1, :11], half=True)
    with pytest.raises(E, match="out must have the shape"):
        nnf.render_sheet(["pred"], (12, 20), 3, pal, pred=pred, out=canvas)
    with pytest.raises(E, match="integer tensor"):
        nnf.render_sheet(["target"], (12, 20), 3, pal, target=target.float())
    assert nnf.sheet_layout(VC.FIVE, 20) == ([("image", 0, 20), ("target", 20, 20), ("pred", 40, 20), ("fill", 60, 20), ("mix_pred", 80, 20)], 100)


# ---------------------------------------------------------------------------------------------------------------------------
# the model level on a stub network (CPU tensors: the numpy path)
# ---------------------------------------------------------------------------------------------------------------------------
def test_predictor_render_and_the_test_loop_sink_on_a_stub():
    from vq_seg_amd.evaluate import test_loop
    from vq_seg_amd.predict import Predictor
    g = torch.Generator().manual_seed(3)
    images = torch.rand((2, 3, 8, 12), generator=g)
    target = torch.randint(0, 3, (2, 16, 24), generator=g)
    for models, tta in ((P.Stub(pool=2), ("none",)), ([P.Stub(pool=2), P.Stub(seed=1, pool=2)], ("none", "hflip"))):
        p = Predictor(models, 3, tta=tta)
        for m in p.models:
            m.train()
        sheet = p.render(images, target, size=(16, 24))
        assert all(m.training for m in p.models)
        label = p(images, size=(16, 24)).label
        value, exact = VC.oracle(VC.FIVE, (16, 24), 3, images.numpy(), label.numpy(), target.numpy())
        assert sheet.dtype == torch.uint8 and tuple(sheet.shape) == (32, 4 * 24 + 20, 3)
        VC.check(sheet.numpy(), value, exact, "Predictor.render")
        assert tuple(p.render(images, half=True).shape) == (8, (3 * 12 + 20) // 2, 3)     # no targets: no target panel
    model = P.Stub(pool=2)
    batches = [(images, target), (images.flip(0), target.flip(0))]
    seen = []
    plain = test_loop(model, batches, 3, fused=True)
    assert test_loop(model, batches, 3, fused=True, visualize=lambda i, v1, v2: seen.append((i, v1, v2))) == plain
    assert [s[0] for s in seen] == [0, 1]
    for _, v1, v2 in seen:
        assert v1.dtype == np.uint8 and v1.shape == (2 * 8, 3 * 12, 3) and v2.dtype == np.uint8 and v2.shape == (2 * 8, 12, 3)
    label = nnf.resize_argmax(model(images)[0], (8, 12))[0]
    value, exact = VC.oracle(["image", "target", "detail", "mix_detail"], (8, 12), 3, images.numpy(), label.numpy(), target.numpy())
    VC.check(np.concatenate(seen[0][1:], axis=1), value, exact, "test_loop sheets")
    with pytest.raises(ValueError, match="fused=True"):
        test_loop(model, batches, 3, visualize=lambda *a: None)
