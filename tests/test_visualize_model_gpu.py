"""The visualisation path at the model level on the GPU, with the tiny networks of tests/predict_cases.py: Predictor.render against
Predictor.__call__'s labels pushed through the fp64 restatement of tests/visualize_cases.py, CPSTrainer.example_image, and the
`visualize` sink of evaluate.test_loop / CPSTrainer.evaluate."""
import numpy as np
import pytest
import torch

from tests import predict_cases as P
from tests import visualize_cases as VC

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def batch(seed=3, n=2, hw=(16, 24), mask=(32, 48)):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((n, 3) + hw, generator=g).to(DEV), torch.randint(0, 3, (n,) + mask, generator=g).to(DEV)


@pytest.mark.parametrize("ensemble", [False, True], ids=["one-network", "two-networks-hflip"])
def test_predictor_render_is_its_labels_through_the_restatement(ensemble):
    from vq_seg_amd import _hip
    from vq_seg_amd.predict import Predictor
    images, target = batch()
    models = [P.Stub(pool=2).to(DEV), P.Stub(seed=1, pool=2).to(DEV)] if ensemble else P.Stub(pool=2).to(DEV)
    p = Predictor(models, 3, tta=("none", "hflip") if ensemble else ("none",))
    for m in p.models:
        m.train()
    size = (32, 48)
    before = _hip.RENDER_SHEET_CALLS
    sheet = p.render(images, target, size=size)
    assert _hip.RENDER_SHEET_CALLS == before + 1 and all(m.training for m in p.models)
    assert sheet.is_cuda and sheet.dtype == torch.uint8 and tuple(sheet.shape) == (64, 4 * 48 + VC.GAP, 3)
    label = p(images, size=size).label
    args = (images.cpu().numpy(), label.cpu().numpy(), target.cpu().numpy())
    value, exact = VC.oracle(VC.FIVE, size, 3, *args)
    VC.check(sheet.cpu().numpy(), value, exact, "render", VC.FIVE, size[1])
    half = p.render(images, target, size=size, half=True)
    value, exact = VC.oracle(VC.FIVE, size, 3, *args, box2=True)
    VC.check(half.cpu().numpy(), value, exact, "render half", VC.FIVE, size[1], 2)
    panels = ["image", "detail", "mix_detail"]
    value, exact = VC.oracle(panels, size, 3, *args)
    VC.check(p.render(images, target, size=size, panels=panels).cpu().numpy(), value, exact, "render detail", panels, size[1])
    assert tuple(p.render(images).shape) == (32, 3 * 24 + VC.GAP, 3)          # no targets: image | pred | gap | mix at the images' size


def test_trainer_example_image_and_the_evaluate_sink():
    from vq_seg_amd import _hip
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer
    images, target = batch(hw=(16, 24), mask=(16, 24))
    ul = batch(seed=4)[0]
    models = [P.Stub(pool=2).to(DEV), P.Stub(seed=1, pool=2).to(DEV)]
    tr = CPSTrainer(CPSConfig(model={"name": "stub"}, total_iters=8), DEV, models=models)
    models[0].train(), models[1].eval()
    flags = [[m.training for m in net.modules()] for net in models]
    before = _hip.RENDER_SHEET_CALLS
    sheet = tr.example_image(images, target, ul)
    assert _hip.RENDER_SHEET_CALLS == before + 2                               # the labelled panels, then the unlabelled mix
    assert flags == [[m.training for m in net.modules()] for net in models]
    assert isinstance(sheet, np.ndarray) and sheet.dtype == np.uint8 and sheet.shape == (2 * 16 // 2, (4 * 24 + 20) // 2, 3)
    size = (16, 24)
    sup = tr.predict(images, size=size).label.cpu().numpy()
    unsup = tr.predict(ul, size=size).label.cpu().numpy()
    left, _ = VC.oracle(["image", "target", "pred", ("fill", 20)], size, 3, images.cpu().numpy(), sup, target.cpu().numpy())
    right, _ = VC.oracle(["mix_pred"], size, 3, ul.cpu().numpy(), unsup)
    full = np.concatenate([left, right], axis=1)
    mean = (full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2]) / 4
    VC.check(sheet, mean, np.zeros(mean.shape[:2], dtype=bool), "example_image")
    assert tr.example_image(images, target, ul, index=1, half=False).shape == (32, 4 * 24 + 20, 3)
    assert flags == [[m.training for m in net.modules()] for net in models]
    # the sink of the scoring loop: one pair of sheets per batch at half the mask size, the same dict
    images, target = batch()
    batches = [(images, target), (images.flip(0), target.flip(0))]
    seen = []
    plain = tr.evaluate(batches, fused=True)
    calls = _hip.RENDER_SHEET_CALLS
    assert tr.evaluate(batches, fused=True) == plain and _hip.RENDER_SHEET_CALLS == calls           # without a sink: no launch
    assert tr.evaluate(batches, fused=True, visualize=lambda i, v1, v2: seen.append((i, v1, v2))) == plain
    assert _hip.RENDER_SHEET_CALLS == calls + 2 and [s[0] for s in seen] == [0, 1]
    size = (16, 24)
    for (_, v1, v2), (img, tgt) in zip(seen, batches):
        assert v1.dtype == np.uint8 and v1.shape == (2 * 16, 3 * 24, 3) and v2.dtype == np.uint8 and v2.shape == (2 * 16, 24, 3)
        label = tr.predict(img, size=size).label.cpu().numpy()
        panels = ["image", "target", "detail", "mix_detail"]
        value, exact = VC.oracle(panels, size, 3, img.cpu().numpy(), label, tgt.cpu().numpy())
        VC.check(np.concatenate([v1, v2], axis=1), value, exact, "test_loop sheets", panels, size[1])
