"""The SLIC and segment-mean kernels (csrc/slic_kernels.hip) against the float64 numpy oracle of tests/slic_cases.py, phase by phase on
identical float32 inputs so that drift cannot compound across iterations.  The bars:

  Lab       max abs error against lab64 at most 4 x the max abs error of the same formulas in float32 numpy on the same pixels (the
            margin covers cbrt / pow implementations that differ by a few ulp and nothing more); both are printed.
  assign    labels equal assign64's under the near-tie rule and its 0.5 % cap (tests/slic_cases.py); the excused count is printed.
  update    centres equal update64's to n_k * 2^-23 * max|value| per cluster and component; an empty cluster bit for bit.
  pooling   segment_mean64 to n_k * 2^-23 * max|x| per segment and channel (any-order float32 summation, then one division)."""
import functools

import numpy as np
import pytest
import torch

from tests import slic_cases as sc

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAMES = sorted(sc.CASES)


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


@functools.lru_cache(maxsize=None)
def _phases(name):
    """the case's float32 Lab (float32 numpy of the oracle's formulas) and float32 centres after 0, 1 and 3 oracle iterations"""
    img, k, m, _ = sc.CASES[name]
    h, w = img.shape[-2:]
    gy, gx, s = sc.grid(h, w, k)
    lab = sc.lab64(img, np.float32)
    centers, kept = sc.init_centers64(lab, gy, gx), {}
    for it in range(4):
        if it in (0, 1, 3):
            kept[it] = centers.astype(np.float32)
        centers = sc.update64(lab, sc.assign64(lab, centers.astype(np.float32), gy, gx, m, s)[0], centers.astype(np.float32))[0]
    return lab, kept, (gy, gx, s)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_lab_and_initial_centres(name, layout):
    from vq_seg_amd import nnf
    img = sc.CASES[name][0]
    gy, gx, _s = _phases(name)[2]
    x = _t(img)
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
    lab, centers = nnf._slic_lab(x, gy, gx)
    torch.cuda.synchronize()
    want = sc.lab64(img)
    err, own = np.abs(lab.cpu().numpy() - want).max(), np.abs(sc.lab64(img, np.float32) - want).max()
    print(f"{name} {layout}: Lab max abs error kernel {err:.3e}, float32 numpy {own:.3e}")
    assert err <= 4 * own
    # the initial centres are the kernel's own Lab values at the seed pixels, bit for bit, and the seeds' coordinates
    assert np.array_equal(centers.cpu().numpy(), sc.init_centers64(lab.cpu().numpy(), gy, gx).astype(np.float32))


@pytest.mark.parametrize("name", NAMES)
def test_assign_equals_the_oracle_under_the_near_tie_rule(name):
    from vq_seg_amd import nnf
    _img, k, m, _ = sc.CASES[name]
    lab, kept, (gy, gx, s) = _phases(name)
    b, _, h, w = lab.shape
    weight = nnf.slic_settings(h, w, k, m, 0)[2]
    for it, centers in kept.items():
        got = nnf._slic_assign(_t(lab), _t(centers), gy, gx, weight)
        torch.cuda.synchronize()
        assert got.dtype == torch.int32
        n_exc, n_bad = sc.excused(got.cpu().numpy(), lab, centers, gy, gx, m, s)
        print(f"{name} centres after {it} iterations: excused {n_exc}, violations {n_bad} of {b * h * w} pixels")
        assert n_bad == 0 and n_exc <= sc.CAP * b * h * w


@pytest.mark.parametrize("name", NAMES)
def test_update_equals_the_oracle_and_keeps_an_empty_cluster(name):
    from vq_seg_amd import nnf
    _img, _k, m, _ = sc.CASES[name]
    lab, kept, (gy, gx, s) = _phases(name)
    k_eff = gy * gx
    labels = sc.assign64(lab, kept[1], gy, gx, m, s)[0]
    if k_eff > 1:                                           # force an empty cluster: hand its pixels to a neighbour (a 3 x 3 neighbour cell)
        labels = np.where(labels == k_eff - 1, k_eff - 2, labels)
    before = kept[1].copy()
    centers = _t(before)
    nnf._slic_update(_t(lab), _t(labels, torch.int32), centers, gy, gx)
    torch.cuda.synchronize()
    got = centers.cpu().numpy()
    want, counts = sc.update64(lab, labels, before)
    assert (np.abs(got - want) <= sc.update_bound(lab, labels, k_eff)).all()
    if k_eff > 1:
        assert (counts[:, k_eff - 1] == 0).all() and np.array_equal(got[:, k_eff - 1], before[:, k_eff - 1])


@pytest.mark.parametrize("name", NAMES)
def test_whole_call(name):
    from vq_seg_amd import nnf
    from vq_seg_amd.utils.superpixel import slic
    img, k, m, _ = sc.CASES[name]
    b, _, h, w = img.shape
    gy, gx, s = sc.grid(h, w, k)
    x = _t(img)
    labels, centers, g = slic(x, k, m, return_centers=True)
    again = nnf.slic(x.contiguous(memory_format=torch.channels_last), k, m)
    torch.cuda.synchronize()
    assert g == (gy, gx) and labels.dtype == torch.int32 and labels.shape == (b, h, w) and centers.shape == (b, gy * gx, 5)
    assert torch.equal(labels, again[0]) and torch.equal(centers, again[1])          # bit-identical from call to call (and layout to layout)
    got = labels.cpu().numpy()
    assert got.min() >= 0 and got.max() < gy * gx
    hi, hj = (np.arange(h) * gy) // h, (np.arange(w) * gx) // w
    gi, gj = got // gx, got % gx
    assert (np.abs(gi - hi[None, :, None]) <= 1).all() and (np.abs(gj - hj[None, None, :]) <= 1).all()      # one of the <= 9 clusters around home
    lab = nnf._slic_lab(x, gy, gx)[0].cpu().numpy()
    n_exc, n_bad = sc.excused(got, lab, centers.cpu().numpy(), gy, gx, m, s)
    print(f"{name}: labels against assign64(returned centres): excused {n_exc}, violations {n_bad} of {b * h * w} pixels")
    assert n_bad == 0 and n_exc <= sc.CAP * b * h * w


def test_case_5_no_superpixel_crosses_the_edge():
    """dL^2 = 10^4 across column 17 against a spatial term of at most (10 / S)^2 * 2 * (2 S)^2 = 800"""
    from vq_seg_amd.utils.superpixel import slic
    img, k, m, _ = sc.CASES["5-edge"]
    labels = slic(_t(img), k, m).cpu().numpy()[0]
    assert not set(labels[:, :17].reshape(-1)) & set(labels[:, 17:].reshape(-1))


def test_case_6_is_the_distance_only_partition():
    """the Lab cost is zero: labels equal the float64 loop's except at near-ties (against the oracle's own final centres)"""
    from vq_seg_amd.utils.superpixel import slic
    img, k, m, _ = sc.CASES["6-constant"]
    gy, gx, s = sc.grid(64, 64, k)
    want, centers, _g = sc.slic64(img, k, m)
    got = slic(_t(img), k, m).cpu().numpy()
    n_exc, n_bad = sc.excused(got, sc.lab64(img), centers, gy, gx, m, s)
    print(f"6-constant: differing pixels {int((got != want).sum())}, excused {n_exc}, violations {n_bad}")
    assert n_bad == 0 and n_exc <= sc.CAP * got.size


# ------------------------------------------------------------------------------------------------------------------- the pooling
@functools.lru_cache(maxsize=None)
def _label_maps():
    """name -> (labels int32 numpy (2, 37, 53), K): the SLIC labels of case 1 (float64 loop) and the adversarial arbitrary map"""
    img, k, m, _ = sc.CASES["1-odd-sides"]
    slic_labels, _c, (gy, gx) = sc.slic64(img, k, m, iters=3)
    return {"slic": (slic_labels.astype(np.int32), gy * gx), "arbitrary": sc.arbitrary_labels()}


@functools.lru_cache(maxsize=None)
def _values(c):
    return (np.random.default_rng(11 + c).standard_normal((2, c, 37, 53)) * 3.0).astype(np.float32)


@pytest.mark.parametrize("which", ["slic", "arbitrary"])
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("c", [3, 32])
def test_segment_mean_forward_backward_and_projection(c, layout, which):
    from vq_seg_amd import nnf
    labels, k = _label_maps()[which]
    x_np, up_np = _values(c), _values(c + 1)[:, :c]
    fmt = torch.channels_last if layout == "channels_last" else torch.contiguous_format
    x = _t(x_np).contiguous(memory_format=fmt).requires_grad_(True)
    lab = _t(labels)
    y = nnf.segment_mean(x, lab, k)
    assert y.stride() == x.stride() and y.dtype == torch.float32
    want, bound = sc.segment_mean64(x_np, labels, k)[0], sc.mean_bound(x_np, labels, k)
    got = y.detach().cpu().numpy()
    assert (np.abs(got - want) <= bound).all()
    # exactly constant within a segment, per image and channel
    for n in range(2):
        flat, at = got[n].reshape(c, -1), labels[n].reshape(-1)
        for s_ in np.unique(at[(at >= 0) & (at < k)]):
            seg = flat[:, at == s_]
            assert (seg.max(axis=1) == seg.min(axis=1)).all()
    out = labels == k                                       # a label outside [0, K): passes through unchanged, bit for bit
    if which == "arbitrary":
        assert out.sum() == 2 and np.array_equal(got.transpose(0, 2, 3, 1)[out], x_np.transpose(0, 2, 3, 1)[out])
        assert not (labels == 1).any() and (labels == 0).sum() == 2            # the unused index, the single-pixel segments
    # backward = the forward operator on the upstream gradient
    up = _t(np.ascontiguousarray(up_np))
    (gx,) = torch.autograd.grad(y, x, up)
    assert (np.abs(gx.cpu().numpy() - sc.segment_mean64(up_np, labels, k)[0]) <= sc.mean_bound(up_np, labels, k)).all()
    # a projection: pooling the pooled tensor changes nothing beyond the bound
    twice = nnf.segment_mean(y.detach(), lab, k).cpu().numpy()
    assert (np.abs(twice - got) <= sc.mean_bound(got, labels, k)).all()


def test_entry_points_refuse_bad_arguments():
    from vq_seg_amd import _hip, nnf
    E = _hip.HipLibraryError
    x = torch.rand(1, 3, 8, 8, device=DEV)
    with pytest.raises(ValueError):
        nnf.slic(x, 65)                                     # more components than pixels: a cell would be empty
    with pytest.raises(E):
        nnf.slic(x.double(), 4)
    with pytest.raises(E):
        nnf.segment_mean(x, torch.zeros(1, 8, 8, device=DEV), 4)
    with pytest.raises(E):
        nnf.segment_mean(x, torch.zeros(1, 8, 9, dtype=torch.int32, device=DEV), 4)
    lab, centers = nnf._slic_lab(x, 2, 2)
    with pytest.raises(E, match="grid"):
        nnf._slic_assign(lab, torch.zeros(1, 9 * 2, 5, device=DEV), 9, 2, 1.0)
