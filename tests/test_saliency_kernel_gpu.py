"""The RBD saliency kernels (vqseg_region_graph_f, vqseg_rbd_*_f; nnf._rbd_* and nnf.saliency_rbd) on the GPU, against the float64
restatement of tests/saliency_cases.py.

Every stage is given the SAME float32 inputs as the float32 torch-op form (utils.saliency, on CPU tensors) and the restatement, so
errors do not compound across stages.  Bars:
  region graph   counts, bnd and adj exact; means inside n_k * 2^-23 * max|value| (any-order float32 sums, DESIGN.md's bound of the
                 SLIC update); inactive rows 0.
  weights        4 x the float32 form's error plus one float32 ulp of the largest weight; +inf entries exactly where they belong.
  geodesic       (K_active - 1) * 2^-24 * max finite G: a path has at most K_active - 1 additions, each rounding once against a partial
                 sum <= max G; +inf entries exactly where they belong.
  w_bg, wCtr normalised, x, x normalised, the map:   4 x the float32 torch-op form's error against float64, plus 2^-23 (the rule of
                 tests/test_conf_ce_kernel_gpu.py).
The measured errors are printed; profiles/saliency/kernel_errors.txt keeps a run's."""
import functools

import numpy as np
import pytest
import torch

from tests import saliency_cases as sal

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAMES = sorted(sal.CASES) + sorted(sal.EXTRA)         # the table's cases, and K = 576 (the second trips of the strided loops)
PAR = (sal.SIGMA_CLR, sal.SIGMA_BNDCON, sal.SIGMA_SPA, sal.MU)


@functools.lru_cache(maxsize=None)
def yard(name):
    """the float32 torch-op form of a case on the CPU, every stage: the inputs the stages are given, and the yardstick"""
    from vq_seg_amd.utils.saliency import saliency_rbd_from_labels_torch, weights_torch
    lab, labels, grid = sal.make(name)
    out, parts = saliency_rbd_from_labels_torch(torch.from_numpy(lab.copy()), torch.from_numpy(labels.copy()), grid, return_parts=True)
    parts = dict(parts, sal=out, weights=weights_torch(parts["stats"], parts["adj"]))
    return {k: v.numpy() for k, v in parts.items()}


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                                     # a copy: the cases are read-only


def inputs(name):
    lab, labels, grid = sal.make(name)
    return dev(lab), dev(labels), grid


def check(what, got, ref, yardstick):
    got, ref = got.detach().cpu().double().numpy(), np.asarray(ref, dtype=np.float64)
    k_err, y_err = float(np.abs(got - ref).max()), float(np.abs(np.asarray(yardstick, dtype=np.float64) - ref).max())
    bar = 4 * y_err + 2.0 ** -23
    print(f"{what}: err kernel {k_err:.3e}, torch-op form {y_err:.3e}, bar {bar:.3e}")
    assert np.isfinite(got).all() and k_err <= bar, what


@pytest.mark.parametrize("name", NAMES)
def test_region_graph(name):
    from vq_seg_amd import nnf
    lab, labels, (gy, gx) = inputs(name)
    stats, adj = nnf._rbd_region_graph(lab, labels, gy, gx)
    ref = sal.reference(name)
    stats, adj = stats.cpu().numpy(), adj.cpu().numpy()
    assert stats.dtype == np.float32 and adj.dtype == np.uint8
    assert np.array_equal(adj, ref["adj"]) and np.array_equal(adj, adj.transpose(0, 2, 1))
    assert np.array_equal(stats[..., 5:], ref["stats"][..., 5:])                    # n, bnd and the pad: exact
    assert not stats[ref["stats"][..., 5] == 0].any()                              # inactive rows are 0
    lab_np, labels_np, _ = sal.make(name)
    h, w = labels_np.shape[1:]
    top = np.array([np.abs(lab_np[:, 0]).max(), np.abs(lab_np[:, 1]).max(), np.abs(lab_np[:, 2]).max(), h - 1, w - 1])
    bound = ref["stats"][..., 5:6] * 2.0 ** -23 * top
    err = np.abs(stats[..., :5].astype(np.float64) - ref["stats"][..., :5])
    print(f"{name}: means err {err.max():.3e}, smallest slack {(bound - err)[ref['stats'][..., 5] > 0].min():.3e}")
    assert (err <= bound).all()


@pytest.mark.parametrize("name", NAMES)
def test_weights(name):
    from vq_seg_amd import nnf
    y = yard(name)
    got = nnf._rbd_weights(dev(y["stats"]), dev(y["adj"])).cpu().numpy()
    ref = sal.weights64(y["stats"], y["adj"])
    assert np.array_equal(np.isinf(got), np.isinf(ref)) and (got[np.isinf(ref)] > 0).all()
    fin = np.isfinite(ref)
    k_err, y_err = np.abs(got[fin] - ref[fin]).max(), np.abs(y["weights"][fin].astype(np.float64) - ref[fin]).max()
    bar = 4 * y_err + float(np.spacing(np.float32(ref[fin].max())))
    print(f"{name}: weights err kernel {k_err:.3e}, torch-op form {y_err:.3e}, bar {bar:.3e}, largest {ref[fin].max():.4g}")
    assert k_err <= bar and np.array_equal(got, got.transpose(0, 2, 1))


@pytest.mark.parametrize("name", NAMES)
def test_geodesic(name):
    from vq_seg_amd import nnf
    y = yard(name)
    wgt = dev(y["weights"])
    got_t = nnf._rbd_geodesic(wgt)
    assert torch.equal(wgt, dev(y["weights"]))                                     # not in place unless asked
    got = got_t.cpu().numpy()
    ref = sal.geodesic64(y["weights"])
    assert not np.isnan(got).any() and np.array_equal(np.isinf(got), np.isinf(ref)) and (got[np.isinf(ref)] > 0).all()
    fin = np.isfinite(ref)
    bar = (sal.k_active(y["stats"]) - 1) * 2.0 ** -24 * ref[fin].max()
    err = np.abs(got[fin] - ref[fin]).max()
    print(f"{name}: geodesic err {err:.3e}, bar {bar:.3e}, max G {ref[fin].max():.4g}, K_active {sal.k_active(y['stats'])}")
    assert err <= bar
    assert np.array_equal(got, got.transpose(0, 2, 1))                             # the blocked phases keep the symmetry, bit for bit
    assert torch.equal(nnf._rbd_geodesic(wgt), got_t)
    assert torch.equal(nnf._rbd_geodesic(wgt[:1].contiguous())[0], got_t[0])       # an image's result does not depend on its companions


@pytest.mark.parametrize("name", NAMES)
def test_row_passes_and_solve(name):
    from vq_seg_amd import nnf
    y = yard(name)
    _lab, labels, (gy, gx) = sal.make(name)
    h, w = labels.shape[1:]
    g, stats, adj = dev(y["geodesic"]), dev(y["stats"]), dev(y["adj"])
    w_bg = nnf._rbd_background(g, stats, PAR[0], PAR[1])
    check(f"{name} w_bg", w_bg, sal.background64(y["geodesic"], y["stats"]), y["w_bg"])
    wctr = nnf._rbd_contrast(g, stats, dev(y["w_bg"]), h, w, PAR[2])
    ref_wctr = sal.contrast64(y["geodesic"], y["stats"], y["w_bg"], h, w)
    wn, x, xn = nnf._rbd_solve(g, stats, adj, dev(y["w_bg"]), wctr, PAR[0], PAR[3])
    # normalised wCtr of the kernel's own contrast pass, against the float64 one of the same inputs
    ref_wn = np.stack([sal.unit_range64(ref_wctr[n], y["stats"][n, :, 5] > 0) for n in range(ref_wctr.shape[0])])
    check(f"{name} wCtr normalised", wn, ref_wn, y["wctr_norm"])
    # the solve on the float32 form's wCtr
    wn2, x, xn = nnf._rbd_solve(g, stats, adj, dev(y["w_bg"]), dev(y["wctr"]), PAR[0], PAR[3])
    r_wn, r_x, r_xn = sal.solve64(y["geodesic"], y["stats"], y["adj"], y["w_bg"], y["wctr"])
    check(f"{name} x", x, r_x, y["x"])
    check(f"{name} x normalised", xn, r_xn, y["xnorm"])
    inactive = dev(y["stats"][..., 5] == 0)
    assert not bool(w_bg[inactive].any() or wctr[inactive].any() or wn[inactive].any() or x[inactive].any() or xn[inactive].any())
    if name == "constant":
        assert not bool(wn.any() or x.any() or xn.any())
    got = nnf._rbd_paint(xn, dev(labels), gy, gx)
    assert torch.equal(got, torch.gather(xn, 1, dev(labels).long().reshape(xn.shape[0], -1)).reshape(got.shape))


@pytest.mark.parametrize("name", NAMES)
def test_from_labels_end_to_end(name):
    from vq_seg_amd.utils.saliency import saliency_rbd_from_labels
    lab, labels, grid = inputs(name)
    got, parts = saliency_rbd_from_labels(lab, labels, grid, return_parts=True)
    assert got.dtype == torch.float32 and got.shape == labels.shape and "geodesic" in parts
    check(f"{name} map", got, sal.reference(name)["sal"], yard(name)["sal"])
    flat, at = got.cpu().numpy().reshape(got.shape[0], -1), labels.cpu().numpy().reshape(got.shape[0], -1)
    for n in range(flat.shape[0]):
        for s_ in np.unique(at[n]):
            part = flat[n][at[n] == s_]
            assert part.max() == part.min()                                        # exactly constant within a superpixel
        if name != "constant":
            assert flat[n].min() == 0.0 and flat[n].max() == 1.0
    if name in sal.EXTRA:
        assert sal.k_active(sal.reference(name)["stats"]) > 512
    if name == "constant":
        assert not bool(got.any())
    assert torch.equal(saliency_rbd_from_labels(lab, labels, grid), got)           # two calls: bit-identical
    alone = saliency_rbd_from_labels(lab[:1].contiguous(), labels[:1].contiguous(), grid)
    assert torch.equal(alone[0], got[0])                                           # alone or in a batch: bit-identical


@pytest.mark.parametrize("shape,k", [((2, 3, 64, 96), 40), ((3, 3, 50, 70), 120)])
def test_from_images_end_to_end(shape, k):
    from vq_seg_amd import nnf
    from vq_seg_amd.utils.saliency import saliency_rbd, saliency_rbd_from_labels
    gen = torch.Generator().manual_seed(shape[2])
    images = torch.rand(shape, generator=gen) * 0.3
    images[:, :, shape[2] // 4: shape[2] // 2, shape[3] // 3: shape[3] // 2] += torch.tensor([0.6, 0.1, 0.3])[None, :, None, None]
    images = images.to(DEV)
    got, parts = nnf.saliency_rbd(images, k, return_parts=True)
    labels, _centers, grid = nnf.slic(images, k)
    assert parts["grid"] == grid and torch.equal(parts["labels"], labels)
    assert torch.equal(got, saliency_rbd_from_labels(parts["lab"], labels, grid))
    assert torch.equal(saliency_rbd(images, k), got)
    assert torch.equal(saliency_rbd(images.contiguous(memory_format=torch.channels_last), k), got)
    assert float(got.min()) == 0.0 and float(got.max()) == 1.0 and not got.requires_grad


def test_refusals_before_a_device_is_touched(monkeypatch):
    from vq_seg_amd import _hip, nnf
    names, real = [], nnf._launch
    monkeypatch.setattr(nnf, "_launch", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    E = _hip.HipLibraryError
    with pytest.raises(E, match="at most 1024 superpixels"):
        nnf.saliency_rbd(torch.zeros(1, 3, 128, 128, device=DEV), 1100)
    with pytest.raises(E, match="float32"):
        nnf.saliency_rbd(torch.zeros(1, 3, 32, 32, device=DEV, dtype=torch.float16), 16)
    with pytest.raises(E, match="int32"):
        nnf.rbd_from_labels(torch.zeros(1, 3, 32, 32, device=DEV), torch.zeros(1, 32, 32, device=DEV, dtype=torch.int64), (4, 4))
    assert not names
    with pytest.raises(E, match="no CPU fallback"):
        nnf.saliency_rbd(torch.zeros(1, 3, 32, 32), 16)
    with pytest.raises(E):
        nnf.rbd_from_labels(torch.zeros(1, 3, 32, 32), torch.zeros(1, 32, 32, dtype=torch.int32), (4, 4))
    L = _hip.lib()
    assert L.vqseg_rbd_weights_f(None, None, 1, 1025, None, None) == -1 and b"null" in L.vqseg_last_error()
    big = torch.zeros(8, device=DEV)
    assert L.vqseg_rbd_geodesic_f(big.data_ptr(), 1, 1025, None) == -1 and b"1024" in L.vqseg_last_error()
    assert L.vqseg_rbd_background_f(big.data_ptr(), big.data_ptr(), 1, 1, 0.0, 1.0, big.data_ptr(), None) == -1
    assert b"sigma" in L.vqseg_last_error()
