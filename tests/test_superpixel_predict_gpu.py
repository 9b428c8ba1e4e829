"""Predictor(superpixels=...): the view-averaged class probabilities are averaged over SLIC superpixels of the images at the
network's size, between the softmax and the arg-max.  The class maps are constant within each superpixel and equal the arg-max of
segment_mean64 (tests/slic_cases.py) of the unpooled probabilities, which the same Predictor without the option hands out
(`probabilities`).  Pixels whose top two pooled probabilities lie within 1e-6 of each other are excepted (the float32 sums and the
logarithm the labels are taken from can order them either way); they may be at most 0.5 % of the pixels."""
import numpy as np
import pytest
import torch

from tests import predict_cases as P
from tests import slic_cases as sc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _images():
    return torch.from_numpy(sc.smooth(77, 2, 64, 64))


@pytest.mark.parametrize("tta", [("none",), ("none", "hflip")], ids=["one-view", "two-views"])
def test_class_maps_are_the_argmax_of_the_pooled_probabilities(tta):
    from vq_seg_amd.predict import Predictor
    from vq_seg_amd.utils.superpixel import slic
    x = _images()
    stub = P.Stub(3, seed=4).to(DEV).eval()
    pred = Predictor(stub, 3, device=DEV, tta=tta, superpixels=36)(x, want_confidence=True)
    assert pred.label.dtype == torch.uint8 and tuple(pred.label.shape) == (2, 64, 64)
    labels = slic(x.to(DEV), 36)
    seg, got = labels.cpu().numpy(), pred.label.cpu().numpy()
    for n in range(2):
        for s_ in np.unique(seg[n]):
            assert np.unique(got[n][seg[n] == s_]).size == 1
    with torch.no_grad():
        prob = Predictor(stub, 3, device=DEV, tta=tta).probabilities(x.to(DEV)).cpu().numpy()
    pooled, _cnt = sc.segment_mean64(prob, seg, 36)
    top2 = np.sort(pooled, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 1e-6
    print(f"{tta}: {int((~clear).sum())} of {clear.size} pixels within 1e-6")
    assert (~clear).sum() <= 0.005 * clear.size
    assert np.array_equal(got[clear], pooled.argmax(axis=1)[clear])
    assert np.abs(pred.confidence.cpu().numpy() - pooled.max(axis=1)).max() <= 1e-5
    plain = Predictor(stub, 3, device=DEV, tta=tta)(x).label.cpu().numpy()
    assert (plain != got).any()                             # superpixels= is not ignored


def test_other_output_size_and_trainer_surface():
    from vq_seg_amd.predict import Predictor
    x = _images()
    stub = P.Stub(3, seed=4, pool=2).to(DEV).eval()          # logits at half the images' size: superpixels of the images brought there
    out = Predictor(stub, 3, device=DEV, superpixels=dict(num_components=16, iters=3))(x, size=(40, 48)).label
    assert tuple(out.shape) == (2, 40, 48) and out.dtype == torch.uint8 and int(out.max()) < 3


def test_window_or_crf_together_with_superpixels_raises():
    from vq_seg_amd.predict import Predictor
    stub = P.Stub(3, seed=4).to(DEV)
    with pytest.raises(ValueError, match="window"):
        Predictor(stub, 3, superpixels=36, window=32)
    with pytest.raises(ValueError, match="crf"):
        Predictor(stub, 3, superpixels=36, crf=True)
