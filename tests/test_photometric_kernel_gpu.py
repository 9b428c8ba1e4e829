"""The photometric kernels (vqseg_photometric_f) on the GPU against the float64 restatement of tests/photometric_cases.py.

Bar (the rule of tests/test_conf_ce_kernel_gpu.py): per case, the distance of the float32 restatement from the float64 one is measured;
the kernel is allowed 4 x that plus 2^-23 on values in [0, 1] -- the margin covers fma contraction and another order of operations -- and
cases with a contrast add |1 - c| times the bar of the mean.  The mean's bar is the a-priori error of the kernel's own summation order
for values in [0, 1]: (longest sequential run per thread + fold levels + 4) 2^-24, from the constants the wrapper exports.  Nothing is
measured against the kernel.  Exact properties: identity rows are bit copies, gray rows have three equal planes, the blur keeps a constant
and reproduces the taps on a one-hot image within 1 ulp; two calls, a sample alone or in a batch, and the two layouts agree bit for bit.
The measured maxima are printed (profiles/photometric/kernel_errors.txt keeps a run's)."""
import numpy as np
import pytest
import torch

from tests import photometric_cases as PC

pytestmark = pytest.mark.gpu

LAYOUTS = ["nchw", "channels_last"]


def _dev(x, layout="nchw"):
    t = torch.from_numpy(np.array(x, dtype=np.float32)).to("cuda:0")             # (a copy: the shared cases are read-only)
    return t.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else t


def _mean_bar(pixels):
    from vq_seg_amd import _hip
    return (_hip.photometric_mean_run(pixels) + _hip.PHOTOMETRIC_MEAN_FOLD_LEVELS + 4) * 2.0 ** -24


@pytest.mark.parametrize("name", PC.CASE_NAMES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_kernel_is_within_the_bar_of_the_float64_restatement(name, layout):
    from vq_seg_amd import _hip
    x, rows, out64, means64, bar32 = PC.case(name)
    t = _dev(x, layout)
    got, means = _hip.photometric(t, rows, return_means=True)
    assert got.dtype == torch.float32 and got.shape == t.shape and got.stride() == t.stride()
    pixels = x.shape[2] * x.shape[3]
    cs = np.asarray([float(np.float32(r[1])) for r in rows])
    mean_err = float(np.abs(means.cpu().numpy().astype(np.float64) - means64)[cs != 1.0].max()) if (cs != 1.0).any() else 0.0
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - out64).max())
    tol = 4 * bar32 + 2.0 ** -23 + float(np.abs(1.0 - cs).max()) * _mean_bar(pixels)
    print(f"photometric {name!r} {layout}: max |kernel - f64| = {err:.3e} (f32 restatement {bar32:.3e}, bar {tol:.3e}); "
          f"mean error {mean_err:.3e} (bar {_mean_bar(pixels):.3e})")
    assert mean_err <= _mean_bar(pixels)
    assert (means.cpu().numpy()[cs == 1.0] == 0).all()                          # not computed where no contrast asks for it
    assert err <= tol


@pytest.mark.parametrize("h,w", [(96, 160), (7, 9), (33, 130)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_mean_covers_every_pixel_once(h, w, layout):
    """coverage canaries: all 0 except one pixel of (1, 1, 1) -- every partial sum is then exact, and m = f32(g(1, 1, 1)) / N"""
    from vq_seg_amd import _hip
    n_px = h * w
    per = _hip.PHOTOMETRIC_MEAN_THREADS * _hip.photometric_mean_blocks(n_px)
    at = {0, w - 1, (h - 1) * w, n_px - 1}                                      # first pixel, last column, last row, last pixel
    for seam in (64, 256, per, 2 * per, per * (_hip.photometric_mean_run(n_px) - 1)):      # wave, workgroup, stride seams; the last trip
        at |= {p for p in (seam - 1, seam, seam + 1) if 0 <= p < n_px}
    at = sorted(at)
    assert len(at) <= _hip.PHOTOMETRIC_ARG_SAMPLES
    x = np.zeros((len(at), 3, n_px), dtype=np.float32)
    for s_, p in enumerate(at):
        x[s_, :, p] = 1.0
    _out, means = _hip.photometric(_dev(x.reshape(len(at), 3, h, w), layout), [PC._row(c=0.5)] * len(at), return_means=True)
    g1 = (np.float32(0.299) + np.float32(0.587)) + np.float32(0.114)
    want = g1 / np.float32(n_px)
    assert (np.abs(means.cpu().numpy() - want) <= 2 * np.spacing(want)).all(), (at, means.cpu().numpy(), want)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_identity_rows_are_bit_copies(layout):
    from vq_seg_amd import _hip
    x = PC.images(3, 17, 70, seed=9).copy()
    x[0, 0, 0, 0], x[0, 1, 5, 65], x[0, 2, 16, 69], x[2, 0, 3, 3] = 1.5, -0.25, -0.0, np.inf
    t = _dev(x, layout)
    calls = _hip.PHOTOMETRIC_CALLS
    got = _hip.photometric(t, [PC.IDENTITY, PC._row(b=0.5), PC.IDENTITY])
    assert _hip.PHOTOMETRIC_CALLS == calls + 1
    for s_ in (0, 2):
        assert torch.equal(got[s_].view(torch.int32), t[s_].view(torch.int32))
    assert not torch.equal(got[1], t[1])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_gray_rows_have_three_equal_planes(layout):
    from vq_seg_amd import _hip
    t = _dev(PC.images(2, 33, 130, seed=8), layout)
    got = _hip.photometric(t, [PC._row(gray=1.0), PC._row(b=1.2, sat=0.6, hue=0.3, gray=1.0, sigma=1.0)])
    assert torch.equal(got[:, 0], got[:, 1]) and torch.equal(got[:, 0], got[:, 2]) and not torch.equal(got[0, 0], t[0, 0])


@pytest.mark.parametrize("sigma", [0.1, 0.7, 2.0])
def test_blur_keeps_a_constant_within_one_ulp(sigma):
    """constants: 0 and 1 (the ends of the range), 0.5 (every product with a tap is exact: isolates the order the taps are added in),
    0.3 and 0.7 (generic, in the lower and the upper half of their binade)"""
    from vq_seg_amd import _hip
    consts = np.asarray([0.0, 1.0, 0.5, 0.3, 0.7], dtype=np.float32)
    x = np.broadcast_to(consts[:, None, None, None], (5, 3, 17, 70))
    got = _hip.photometric(_dev(x), [PC._row(sigma=sigma)] * 5).cpu().numpy()
    ulps = np.abs(got - consts[:, None, None, None]).max(axis=(1, 2, 3)) / np.spacing(np.maximum(consts, np.float32(2.0 ** -126)))
    print(f"photometric blur of constants, sigma {sigma}: {dict(zip(consts.tolist(), ulps.tolist()))} ulp")
    assert (ulps <= 1.0).all()


@pytest.mark.parametrize("sigma", [0.7, 2.0])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_blur_of_a_one_hot_image_is_the_outer_product_of_the_taps(sigma, layout):
    """one-hot at a centre pixel (across the tile seams at x = 64 and y = 16) and at every corner, where reflect-101 folds nothing onto
    the corner itself: out[y, x] = w[|y - y0|] w[|x - x0|] plus, next to a border, the taps reflection sends back -- expected from the
    float32 taps in float64, compared within 1 ulp of the expected value"""
    from vq_seg_amd import _hip
    h, w = 33, 130
    r, taps = PC.taps_of(sigma)
    spots = [(16, 64), (0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    x = np.zeros((len(spots), 3, h, w), dtype=np.float32)
    want = np.zeros((len(spots), h, w), dtype=np.float64)

    def line(n, at):                                                           # the 1-D response of a unit pulse at `at`, reflect-101
        pulse = np.zeros(n)
        pulse[at] = 1.0
        p = np.pad(pulse, r, mode="reflect")
        return np.asarray([(taps.astype(np.float64) * p[i:i + 2 * r + 1]).sum() for i in range(n)])

    for s_, (y0, x0) in enumerate(spots):
        x[s_, :, y0, x0] = 1.0
        want[s_] = np.outer(line(h, y0), line(w, x0))
    got = _hip.photometric(_dev(x, layout), [PC._row(sigma=sigma)] * len(spots)).cpu().numpy()
    for p in range(3):
        diff = np.abs(got[:, p].astype(np.float64) - want)
        assert (diff <= np.spacing(want.astype(np.float32))).all(), (p, float(diff.max()))
    assert (got[0, 0, 16 - r:17 + r, 64 - r:65 + r] > 0).all() and got[0].sum() > 0.99 * 3


def test_bit_identity_between_calls_batches_and_layouts():
    from vq_seg_amd import _hip
    x = PC.images(4, 96, 160, seed=12)                                         # 4 mean workgroups per sample
    rows = [PC.ALL_A, PC.ALL_B, PC._row(c=1.5, sigma=2.0), PC._row(c=0.5)]
    t = _dev(x)
    a, ma = _hip.photometric(t, rows, return_means=True)
    b, mb = _hip.photometric(t, rows, return_means=True)
    assert torch.equal(a, b) and torch.equal(ma, mb)                            # two calls
    for s_ in range(4):                                                         # a sample alone, or at another place of another batch
        alone, m1 = _hip.photometric(t[s_:s_ + 1].contiguous(), rows[s_:s_ + 1], return_means=True)
        assert torch.equal(alone[0], a[s_]) and torch.equal(m1[0], ma[s_])
    rev = _hip.photometric(t.flip(0).contiguous(), rows[::-1])
    assert torch.equal(rev.flip(0), a)
    cl, mc = _hip.photometric(t.contiguous(memory_format=torch.channels_last), rows, return_means=True)
    assert cl.is_contiguous(memory_format=torch.channels_last) and torch.equal(cl, a) and torch.equal(mc, ma)      # the two layouts
    big = torch.cat([t[:1]] * 33)                                               # the same sample on both sides of a parameter-chunk seam
    out = _hip.photometric(big, [rows[0]] * 33)
    assert torch.equal(out[0], a[0]) and torch.equal(out[31], a[0]) and torch.equal(out[32], a[0])


def test_wrapper_checks_and_counter():
    from vq_seg_amd import _hip
    from vq_seg_amd.data import photometric
    t = _dev(PC.images(2, 7, 9, seed=1))
    calls = _hip.PHOTOMETRIC_CALLS
    out = photometric(t, [PC.IDENTITY, PC._row(sigma=2.0)])
    assert _hip.PHOTOMETRIC_CALLS == calls + 1 and out.is_cuda
    photometric(t[:, :, :, ::2], [PC.IDENTITY] * 2)                            # any other layout is copied once
    assert _hip.PHOTOMETRIC_CALLS == calls + 2
    with pytest.raises(_hip.HipLibraryError, match="out of place"):
        _hip.photometric(t, [PC.IDENTITY] * 2, out=t)
    with pytest.raises(ValueError, match="min"):
        photometric(t[:, :, :6].contiguous(), [PC._row(sigma=2.0)] * 2)
    assert _hip.PHOTOMETRIC_CALLS == calls + 2
