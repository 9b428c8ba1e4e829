"""The photometric strong augmentation without a GPU: the float64 restatement (tests/photometric_cases.py) against independent
implementations of its two non-trivial steps (scipy's mirror correlation, colorsys), the taps, the draws and their generator key, the
CPU torch-op form against the restatement, identity rows, argument checks, the C entry point's own checks, and CPSConfig validation."""
import colorsys
import ctypes

import numpy as np
import pytest
import torch

from tests import photometric_cases as PC
from vq_seg_amd import _hip
from vq_seg_amd.data import (IDENTITY_PHOTOMETRIC, StrongPhotometric, draw_photometric, photometric, photometric_taps,
                             step_photometric, step_transforms)
from vq_seg_amd.data import augmentations as A


@pytest.mark.parametrize("sigma", [0.1, 0.7, 2.0])
def test_restated_blur_is_scipys_mirror_correlation_twice(sigma):
    from scipy.ndimage import correlate1d
    x = PC.images(1, 13, 19, seed=3)
    r, taps = PC.taps_of(sigma)
    got = PC.photometric64(x, [PC._row(sigma=sigma)])[0]
    want = correlate1d(correlate1d(x[0].astype(np.float64), taps.astype(np.float64), axis=2, mode="mirror"), taps.astype(np.float64), axis=1,
                       mode="mirror")
    assert r == int(np.ceil(3 * float(np.float32(sigma)))) and np.abs(got - want).max() < 1e-15


@pytest.mark.parametrize("hue", [-0.5, -0.25, 0.1, 0.25, 0.5])
def test_restated_hue_is_colorsys_pixel_by_pixel(hue):
    x = PC.images(1, 9, 11, seed=4)
    got = PC.photometric64(x, [PC._row(hue=hue)])[0]
    for y in range(9):
        for xx in range(11):
            h, s, v = colorsys.rgb_to_hsv(*(float(c) for c in x[0, :, y, xx]))
            want = colorsys.hsv_to_rgb((h + float(np.float32(hue))) % 1.0, s, v)
            assert np.abs(got[:, y, xx] - np.asarray(want)).max() < 1e-14, (y, xx, x[0, :, y, xx])


@pytest.mark.parametrize("sigma", [0.0, 1e-3, 0.1, 1 / 3, 0.34, 0.7, 1.0, 2.0, 8 / 3])
def test_taps_sum_to_one_and_are_symmetric(sigma):
    t = photometric_taps(sigma)
    r = int(np.ceil(3.0 * sigma))
    assert t.dtype == np.float32 and t.shape == (2 * r + 1,) and r <= 8
    assert np.array_equal(t, t[::-1])
    assert abs(float(t.astype(np.float64).sum()) - 1.0) <= 2.0 ** -23          # 1 ulp of 1.0
    assert (t > 0).any() and (t >= 0).all() and t.argmax() == r
    with pytest.raises(ValueError):
        photometric_taps(2.7)                                                   # R = 9


def test_step_photometric_is_a_pure_function_of_its_key_and_moves_nothing_else():
    step_boxes = A.step_boxes
    boxes, trans = step_boxes(4, 64, 64, 0.25, 42, 0, 3, "sample"), step_transforms(4, 42, 0, 3, "sample")
    # pinned from the code as it stood before key 2 existed: the boxes' three-element key and the transforms' key 1 did not move
    assert boxes == [(13, 32, 48, 21), (15, 8, 21, 48), (8, 16, 26, 39), (23, 22, 24, 41)]
    assert trans == ([7, 9, 1, 5], [84.13628480599871, 0.0, 0.0, 54.38247310522095])
    a = step_photometric(4, 42, 0, 3, "sample")
    assert a == step_photometric(4, 42, 0, 3, "sample") and len(a) == 4 and len(set(a)) == 4
    assert a != step_photometric(4, 42, 0, 4, "sample") and a != step_photometric(4, 42, 1, 3, "sample") and a != step_photometric(4, 43, 0, 3, "sample")
    assert step_boxes(4, 64, 64, 0.25, 42, 0, 3, "sample") == boxes and step_transforms(4, 42, 0, 3, "sample") == trans
    # the documented draw: eight uniforms per unit under the key [seed, rank, it, 2], whatever the outcome
    rng = np.random.default_rng([42, 0, 3, 2])
    for row in a:
        u = rng.random(8)
        b, c, sat, hue = (1 + (2 * u[1] - 1) * 0.5, 1 + (2 * u[2] - 1) * 0.5, 1 + (2 * u[3] - 1) * 0.5, (2 * u[4] - 1) * 0.25) if u[0] < 0.8 else (1, 1, 1, 0)
        assert row == (b, c, sat, hue, float(u[5] < 0.2), 0.1 + u[7] * 1.9 if u[6] < 0.5 else 0.0)
    # a sample's row does not depend on the others' outcome: other probabilities, same uniforms per position
    off = step_photometric(4, 42, 0, 3, "sample", blur_p=0.0)
    assert [r[:5] for r in off] == [r[:5] for r in a] and all(r[5] == 0.0 for r in off)
    one = step_photometric(4, 42, 0, 3, "batch")
    assert one == [a[0]] * 4
    rng = np.random.default_rng(5)
    draw_photometric(rng, jitter_p=0.0, gray_p=0.0, blur_p=0.0)
    assert rng.random() == np.random.default_rng(5).random(9)[8]                # eight consumed


def test_all_probabilities_zero_give_the_identity_row():
    rows = step_photometric(3, 1, 0, 0, "sample", jitter_p=0.0, gray_p=0.0, blur_p=0.0)
    assert rows == [IDENTITY_PHOTOMETRIC] * 3 and IDENTITY_PHOTOMETRIC == (1.0, 1.0, 1.0, 0.0, 0.0, 0.0)


@pytest.mark.parametrize("name", PC.CASE_NAMES)
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_cpu_form_is_within_the_bar_of_the_restatement(name, layout):
    x, rows, out64, _means, bar32 = PC.case(name)
    t = torch.from_numpy(x.copy())
    if layout == "channels_last":
        t = t.contiguous(memory_format=torch.channels_last)
    got = photometric(t, rows)
    assert got.dtype == torch.float32 and got.shape == t.shape and got.stride() == t.stride()
    cmax = max(abs(1.0 - float(np.float32(r[1]))) for r in rows)
    tol = 4 * bar32 + 2.0 ** -23 + cmax * 8 * 2.0 ** -24                        # (torch's pairwise f32 mean: a few ulp of a value in [0, 1])
    err = float(np.abs(got.numpy().astype(np.float64) - out64).max())
    assert err <= tol, (name, err, tol)


def test_identity_row_returns_the_input_bits():
    x = torch.from_numpy(PC.images(2, 7, 9, seed=1).copy())
    x[0, 0, 0, 0], x[0, 1, 0, 0], x[0, 2, 0, 0], x[1, 0, 3, 3] = 1.5, -0.25, -0.0, float("inf")
    got = photometric(x, [IDENTITY_PHOTOMETRIC, IDENTITY_PHOTOMETRIC])
    assert got is not x and torch.equal(got.view(torch.int32), x.view(torch.int32))
    mixed = photometric(x, [IDENTITY_PHOTOMETRIC, PC._row(b=0.5)])
    assert torch.equal(mixed[0].view(torch.int32), x[0].view(torch.int32)) and not torch.equal(mixed[1], x[1])


def test_bad_arguments_raise():
    x = torch.rand(2, 3, 7, 9)
    ok = [IDENTITY_PHOTOMETRIC] * 2
    with pytest.raises(ValueError, match="radius"):
        photometric(x, [PC._row(sigma=2.7)] * 2)                                # R = 9 > 8
    with pytest.raises(ValueError, match="min"):
        photometric(torch.rand(2, 3, 6, 9), [PC._row(sigma=2.0)] * 2)           # R = 6 > min(H, W) - 1 = 5
    with pytest.raises(ValueError, match="hue"):
        photometric(x, [PC._row(hue=0.51)] * 2)
    with pytest.raises(ValueError, match="float32"):
        photometric((x * 255).to(torch.uint8), ok)
    with pytest.raises(ValueError, match="float32"):
        photometric(x.double(), ok)
    with pytest.raises(ValueError, match="RGB"):
        photometric(torch.rand(2, 4, 7, 9), ok)
    with pytest.raises(ValueError, match="RGB"):
        photometric(torch.rand(3, 7, 9), ok)
    with pytest.raises(ValueError, match="row per sample"):
        photometric(x, ok[:1])
    with pytest.raises(ValueError, match="gray"):
        photometric(x, [PC._row(gray=0.5)] * 2)
    with pytest.raises(ValueError, match="finite"):
        photometric(x, [PC._row(b=float("nan"))] * 2)
    with pytest.raises(ValueError, match=">= 0"):
        photometric(x, [PC._row(sat=-0.1)] * 2)
    with pytest.raises(ValueError):
        step_photometric(2, 0, 0, 0, "pixel")
    with pytest.raises(ValueError):
        step_photometric(2, 0, 0, 0, sigma=(0.1, 3.0))
    with pytest.raises(ValueError):
        StrongPhotometric(hue=0.6)


def test_strong_photometric_draws_from_its_own_generator():
    x = torch.from_numpy(PC.images(3, 17, 20, seed=2).copy())
    state = np.random.get_state()[1].copy()
    a, b = StrongPhotometric(seed=11), StrongPhotometric(seed=11)
    ya, yb = a(x), b(x)
    assert torch.equal(ya, yb) and a.last_params == b.last_params and len(a.last_params) == 3
    assert torch.equal(ya, photometric(x, a.last_params))
    assert a(x) is not None and a.last_params != b.last_params                  # the generator advanced
    assert (np.random.get_state()[1] == state).all()                            # nothing from the global generator
    one = StrongPhotometric(seed=11, per="batch")
    one(x)
    assert one.last_params == [one.last_params[0]] * 3
    off = StrongPhotometric(jitter_p=0.0, gray_p=0.0, blur_p=0.0, seed=0)
    assert torch.equal(off(x), x) and off.last_params == [IDENTITY_PHOTOMETRIC] * 3


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """the C side's own checks, with host pointers that are never dereferenced as device memory (every call returns before a launch)"""
    L = _hip.lib()
    assert hasattr(L, "vqseg_photometric_f") and "vqseg_photometric_f" in _hip.SYMBOLS and "vqseg_photometric_mean_blocks" in _hip.SYMBOLS
    assert [L.vqseg_photometric_mean_blocks(p) for p in (1, 4096, 4097, 15360, 64 * 4096, 10 ** 8)] == [1, 1, 2, 4, 64, 64]
    assert L.vqseg_photometric_mean_blocks(0) < 0
    assert _hip.photometric_mean_run(15360) == 15 and _hip.photometric_mean_run(512 * 512) == 16 and _hip.photometric_mean_run(64) == 1
    buf = (ctypes.c_float * 16)()
    src, out = ctypes.addressof(buf), ctypes.addressof(buf) + 4

    def call(n=1, h=7, w=9, strides=(189, 63, 1), row=PC.IDENTITY, radius=0, taps=(1.0,) + (0.0,) * 8, s=src, o=out, partials=None):
        rows = np.asarray([row] * n, dtype=np.float32)
        rad = np.asarray([radius] * n, dtype=np.int32)
        tp = np.asarray([taps] * n, dtype=np.float32)
        return L.vqseg_photometric_f(s, o, n, h, w, *strides, rows.ctypes.data, rad.ctypes.data, tp.ctypes.data, partials, None, None)

    half = tuple(photometric_taps(2.0)[6:]) + (0.0, 0.0)
    bad = [dict(n=0), dict(h=0), dict(s=None), dict(o=src), dict(strides=(189, 63, 2)), dict(strides=(189, 1, 4)), dict(n=2, strides=(100, 63, 1)),
           dict(row=PC._row(hue=0.6)), dict(row=PC._row(gray=0.5)), dict(row=PC._row(b=float("inf"))), dict(row=PC._row(c=-1.0)),
           dict(row=PC._row(sigma=2.0), radius=0), dict(radius=1), dict(row=PC._row(sigma=2.0), radius=9, taps=half),
           dict(row=PC._row(sigma=2.0), radius=6, taps=half, h=6, strides=(162, 54, 1)),
           dict(row=PC._row(sigma=0.3), radius=1, taps=(0.5, 0.25, 0.25) + (0.0,) * 6), dict(row=PC._row(sigma=0.3), radius=1, taps=(2.0, 0.0) + (0.0,) * 7),
           dict(row=PC._row(c=0.5))]                                            # contrast without the partials workspace
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"photometric" in L.vqseg_last_error()
    x = torch.rand(1, 3, 7, 9)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        _hip.photometric(x, [PC.IDENTITY])


def test_config_fields_and_their_validation():
    from vq_seg_amd.trainer import CPSConfig
    cfg = CPSConfig(model={})
    assert cfg.hard_aug is None and cfg.hard_aug_per == "sample" and cfg.hard_aug_jitter == (0.5, 0.5, 0.5, 0.25) and cfg.hard_aug_jitter_p == 0.8
    assert cfg.hard_aug_gray_p == 0.2 and cfg.hard_aug_blur_p == 0.5 and cfg.hard_aug_sigma == (0.1, 2.0)
    assert CPSConfig(model={}, hard_aug="photometric", hard_aug_jitter=[0.4, 0.4, 0.4, 0.1]).hard_aug_jitter == (0.4, 0.4, 0.4, 0.1)
    for kw in (dict(hard_aug="colour"), dict(hard_aug_per="pixel"), dict(hard_aug_jitter=(0.5, 0.5, 0.5)), dict(hard_aug_jitter=(1.5, 0.5, 0.5, 0.25)),
               dict(hard_aug_jitter=(0.5, 0.5, 0.5, 0.6)), dict(hard_aug_jitter_p=1.5), dict(hard_aug_gray_p=-0.1), dict(hard_aug_blur_p=2),
               dict(hard_aug_sigma=(2.0, 0.1)), dict(hard_aug_sigma=(0.1, 3.0)), dict(hard_aug_sigma=(-0.1, 1.0))):
        with pytest.raises(ValueError):
            CPSConfig(model={}, **kw)
    assert A.PHOTOMETRIC_DEFAULTS == dict(jitter=cfg.hard_aug_jitter, jitter_p=0.8, gray_p=0.2, blur_p=0.5, sigma=cfg.hard_aug_sigma)
