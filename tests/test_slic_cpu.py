"""SLIC superpixels and superpixel-mean pooling without a GPU: the float64 oracle of tests/slic_cases.py against itself evaluated in
float32 and against the torch-op form of vq_seg_amd.utils.superpixel (what CPU tensors and unsupported inputs take), the pooling and
its gradient, the stated grids, and the option checks of CPSConfig and Predictor.

The near-tie rule and its cap are stated in tests/slic_cases.py.  "The oracle alone stays within the cap" is checked as: the oracle's
own loop run on float32-rounded intermediates (Lab and centres rounded to float32 after every phase, as any float32 implementation
holds them) is compared with assign64 on those same values, phase by phase; what is counted is the pixels the rule has to excuse.
The number of pixels that are merely ELIGIBLE is printed, not bounded: the constant image of case 6 starts from exact ties on whole
rows and columns (9 % of its pixels), which every exact evaluation resolves the same way."""
import numpy as np
import pytest
import torch

from tests import slic_cases as sc


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_grids_are_the_stated_ones(name):
    from vq_seg_amd.utils.superpixel import superpixel_grid
    img, k, _m, want = sc.CASES[name]
    h, w = img.shape[-2:]
    gy, gx, s = sc.grid(h, w, k)
    assert superpixel_grid(h, w, k) == (gy, gx)
    assert want is None or (gy, gx) == want
    assert abs(s * s * k - h * w) < 1e-9 * h * w


def test_grid_of_the_training_shape_and_bad_counts():
    from vq_seg_amd.utils.superpixel import superpixel_grid
    assert superpixel_grid(512, 512, 1600) == (40, 40)
    assert superpixel_grid(64, 64, 36) == (6, 6)
    for bad in (0, -3, 65 * 64, 2.5, True):
        with pytest.raises(ValueError):
            superpixel_grid(64, 64, bad)


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_oracle_in_float32_stays_within_the_cap(name):
    img, k, m, _ = sc.CASES[name]
    b, _, h, w = img.shape
    gy, gx, s = sc.grid(h, w, k)
    lab = sc.lab64(img, np.float32)
    centers = sc.init_centers64(lab, gy, gx).astype(np.float32)
    worst = 0
    for it in range(5):
        index = sc.candidates64(lab, centers, gy, gx, m, s)[0]
        # the float32 evaluation: the same sums of squares with float32 operands and float32 roundings
        d32 = _dist32(lab, centers, gy, gx, m, s)
        got = np.take_along_axis(np.broadcast_to(index, d32.shape), np.argmin(d32, axis=1)[:, None], axis=1)[:, 0]
        n_exc, n_bad = sc.excused(got, lab, centers, gy, gx, m, s)
        _want, best, second = sc.assign64(lab, centers, gy, gx, m, s)
        eligible = int((second - best < sc.NEAR_TIE * np.maximum(best, np.finfo(np.float64).tiny)).sum())
        print(f"{name} iteration {it}: excused {n_exc}, violations {n_bad}, eligible {eligible} of {b * h * w} pixels")
        assert n_bad == 0
        worst = max(worst, n_exc)
        centers = sc.update64(lab, got, centers)[0].astype(np.float32)
    assert worst <= sc.CAP * b * h * w


def _dist32(lab, centers, gy, gx, m, s):
    f = np.float32
    lab, centers = lab.astype(f), centers.astype(f)
    b, _, h, w = lab.shape
    hi, hj = (np.arange(h) * gy) // h, (np.arange(w) * gx) // w
    ys, xs = np.arange(h, dtype=f)[:, None], np.arange(w, dtype=f)[None, :]
    m2s = f((m / s) ** 2)
    out = np.full((b, 9, h, w), np.inf, dtype=f)
    at = 0
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            ci, cj = hi + di, hj + dj
            ok = ((ci >= 0) & (ci < gy))[:, None] & ((cj >= 0) & (cj < gx))[None, :]
            c = centers[:, np.clip(ci, 0, gy - 1)[:, None] * gx + np.clip(cj, 0, gx - 1)[None, :]]
            d = ((lab[:, 0] - c[..., 0]) ** 2 + (lab[:, 1] - c[..., 1]) ** 2 + (lab[:, 2] - c[..., 2]) ** 2
                 + m2s * ((ys - c[..., 3]) ** 2 + (xs - c[..., 4]) ** 2))
            out[:, at] = np.where(ok, d, np.inf)
            at += 1
    return out


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_torch_form_matches_the_oracle_under_the_near_tie_rule(name):
    """phase by phase on identical float32 inputs, so that drift cannot compound: Lab, then every assign and update of four iterations"""
    from vq_seg_amd.utils import superpixel as sp
    img, k, m, _ = sc.CASES[name]
    b, _, h, w = img.shape
    gy, gx, s = sc.grid(h, w, k)
    lab = sp.rgb_to_lab(torch.from_numpy(img))
    assert lab.dtype == torch.float32
    err, own = np.abs(lab.numpy() - sc.lab64(img)).max(), np.abs(sc.lab64(img, np.float32) - sc.lab64(img)).max()
    print(f"{name}: Lab max abs error torch {err:.3e}, float32 numpy {own:.3e}")
    assert err <= 4 * own + 1e-5                            # (no bar is set for this form; a wrong constant shows as 1e-2 and more)
    weight = sp.nnf.slic_settings(h, w, k, m, 4)[2]
    centers = torch.from_numpy(sc.init_centers64(lab.numpy(), gy, gx).astype(np.float32))
    for it in range(4):
        got = sp._assign_torch(lab, centers, gy, gx, weight)
        n_exc, n_bad = sc.excused(got.numpy(), lab.numpy(), centers.numpy(), gy, gx, m, s)
        print(f"{name} iteration {it}: excused {n_exc}, violations {n_bad}")
        assert n_bad == 0 and n_exc <= sc.CAP * b * h * w
        new = sp._update_torch(lab, got, centers)
        want, _counts = sc.update64(lab.numpy(), got.numpy(), centers.numpy())
        assert (np.abs(new.numpy() - want) <= sc.update_bound(lab.numpy(), got.numpy(), gy * gx)).all()
        centers = new
    # the whole call: labels are the assignment against the returned centres, in range, int32
    labels, cent, g = sp.slic(torch.from_numpy(img), k, m, iters=4, return_centers=True)
    assert g == (gy, gx) and labels.dtype == torch.int32 and int(labels.min()) >= 0 and int(labels.max()) < gy * gx
    n_exc, n_bad = sc.excused(labels.numpy(), lab.numpy(), cent.numpy(), gy, gx, m, s)
    assert n_bad == 0 and n_exc <= sc.CAP * b * h * w
    assert torch.equal(sp.slic(torch.from_numpy(img), k, m, iters=4), labels)


def test_edge_case_keeps_the_two_sides_apart_and_constant_image_is_the_distance_partition():
    """case 5: dL^2 = 10^4 across column 17 against a spatial term of at most (10 / S)^2 * 2 * (2 S)^2 = 800; case 6: the Lab cost is
    zero, the partition is the distance-only one of the oracle (all its arithmetic is exact in float32)"""
    from vq_seg_amd.utils.superpixel import slic
    img, k, m, _ = sc.CASES["5-edge"]
    labels = slic(torch.from_numpy(img), k, m).numpy()[0]
    assert not set(labels[:, :17].reshape(-1)) & set(labels[:, 17:].reshape(-1))
    img, k, m, _ = sc.CASES["6-constant"]
    assert np.array_equal(slic(torch.from_numpy(img), k, m).numpy(), sc.slic64(img, k, m)[0])


def _pool_inputs(c, seed=3):
    rng = np.random.default_rng(seed)
    labels, k = sc.arbitrary_labels()
    x = (rng.standard_normal((2, c, 37, 53)) * 3.0).astype(np.float32)
    return x, labels, k


@pytest.mark.parametrize("c", [3, 32])
def test_superpixel_mean_on_cpu_tensors_meets_the_summation_bound(c):
    from vq_seg_amd.utils.superpixel import superpixel_mean
    x, labels, k = _pool_inputs(c)
    want, _cnt = sc.segment_mean64(x, labels, k)
    got = superpixel_mean(torch.from_numpy(x), torch.from_numpy(labels), k)
    assert got.dtype == torch.float32 and got.shape == x.shape
    assert (np.abs(got.numpy() - want) <= sc.mean_bound(x, labels, k)).all()
    out = labels == k                                       # the label outside [0, k) passes through unchanged, bit for bit
    assert out.sum() == 2 and np.array_equal(got.numpy().transpose(0, 2, 3, 1)[out], x.transpose(0, 2, 3, 1)[out])
    # SLIC labels of case 1, num_segments taken from the labels
    from vq_seg_amd.utils.superpixel import slic
    img = sc.CASES["1-odd-sides"][0]
    sl = slic(torch.from_numpy(img), 24)
    got = superpixel_mean(torch.from_numpy(x), sl)
    assert (np.abs(got.numpy() - sc.segment_mean64(x, sl.numpy(), 24)[0]) <= sc.mean_bound(x, sl.numpy(), 24)).all()


def test_superpixel_mean_gradcheck_and_self_adjointness():
    from vq_seg_amd.utils.superpixel import superpixel_mean
    g = torch.Generator().manual_seed(0)
    labels = torch.randint(0, 5, (2, 6, 7), generator=g)
    x = torch.randn(2, 3, 6, 7, dtype=torch.float64, generator=g, requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: superpixel_mean(t, labels, 5), (x,))
    up = torch.randn(2, 3, 6, 7, dtype=torch.float64, generator=g)
    (gx,) = torch.autograd.grad(superpixel_mean(x, labels, 5), x, up)
    assert torch.allclose(gx, superpixel_mean(up, labels, 5), rtol=0, atol=1e-14)
    once = superpixel_mean(x.detach(), labels, 5)
    assert torch.allclose(superpixel_mean(once, labels, 5), once, rtol=0, atol=1e-14)


def test_bad_arguments_raise():
    from vq_seg_amd.utils.superpixel import slic, superpixel_mean
    with pytest.raises(ValueError):
        slic(torch.rand(3, 8, 8), 4)
    with pytest.raises(ValueError):
        slic(torch.rand(1, 3, 8, 8), 4, iters=-1)
    with pytest.raises(ValueError):
        slic(torch.rand(1, 3, 8, 8), 4, compactness=-1.0)
    with pytest.raises(ValueError):
        superpixel_mean(torch.rand(1, 3, 8, 8), torch.zeros(1, 8, 9, dtype=torch.int32))
    with pytest.raises(ValueError):
        superpixel_mean(torch.rand(1, 3, 8, 8), torch.zeros(1, 8, 8))


def test_nnf_entry_points_refuse_cpu_tensors():
    from vq_seg_amd import _hip, nnf
    assert not nnf.slic_supported(torch.rand(1, 3, 8, 8)) and not nnf.segment_mean_supported(torch.rand(1, 3, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int32))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        nnf.slic(torch.rand(1, 3, 8, 8), 4)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        nnf.segment_mean(torch.rand(1, 3, 8, 8), torch.zeros(1, 8, 8, dtype=torch.int32), 4)


def _model():
    return {"name": "vqreptunet1x1", "params": {"encoder_name": "resnet50", "num_classes": 3, "depth": 5,
                                                "vq_cfg": {"num_embeddings": [0, 0, 64, 64, 64], "distance": "euclidean", "kmeans_init": True},
                                                "margin": 0.0, "scale": 1.0, "use_feature": False, "encoder_weights": None}}


def test_config_validates_the_superpixel_options():
    from vq_seg_amd.trainer import CPSConfig
    assert CPSConfig(model=_model()).superpixel_mean is None
    ok = CPSConfig(model=_model(), superpixel_mean=1600)
    assert (ok.superpixel_compactness, ok.superpixel_iters) == (10.0, 10)
    CPSConfig(model=_model(), recipe="v2", superpixel_mean=36, superpixel_iters=0)
    for bad in (dict(superpixel_mean=0), dict(superpixel_mean=-5), dict(superpixel_mean=2.5), dict(superpixel_mean=True),
                dict(superpixel_mean=36, superpixel_compactness=-1.0), dict(superpixel_mean=36, superpixel_compactness=float("nan")),
                dict(superpixel_mean=36, superpixel_iters=-1), dict(superpixel_mean=36, superpixel_iters=1.5),
                dict(superpixel_compactness=-1.0), dict(superpixel_iters=-2)):
        with pytest.raises(ValueError):
            CPSConfig(model=_model(), **bad)


def test_predictor_rejects_the_bad_combinations():
    from vq_seg_amd.predict import Predictor
    net = torch.nn.Conv2d(3, 3, 1)
    assert Predictor(net, 3).superpixels is None
    assert Predictor(net, 3, superpixels=36).superpixels == dict(num_components=36, compactness=10.0, iters=10)
    assert Predictor(net, 3, superpixels=dict(num_components=9, iters=2)).superpixels == dict(num_components=9, compactness=10.0, iters=2)
    with pytest.raises(ValueError, match="window"):
        Predictor(net, 3, superpixels=36, window=32)
    with pytest.raises(ValueError, match="crf"):
        Predictor(net, 3, superpixels=36, crf=True)
    for bad in (0, -1, True, dict(compactness=3.0), dict(num_components=4, colour=1), dict(num_components=4, iters=-1)):
        with pytest.raises((ValueError, TypeError)):
            Predictor(net, 3, superpixels=bad)


def test_predictor_pools_on_cpu_tensors_too():
    """the same slot on the CPU path: class maps constant within each superpixel of the image at the network's size"""
    from vq_seg_amd.predict import Predictor
    from vq_seg_amd.utils.superpixel import slic
    torch.manual_seed(0)
    net = torch.nn.Conv2d(3, 3, 3, padding=1)
    img = torch.from_numpy(sc.smooth(9, 2, 32, 32))
    out = Predictor(net, 3, superpixels=16)(img).label
    labels = slic(img, 16)
    for n in range(2):
        for s_ in labels[n].unique():
            assert out[n][labels[n] == s_].unique().numel() == 1
