"""similarity_transform / inverse_similarity_transform / warp_batch on device tensors: they take the affine-warp kernel (seen
through its call counter) and agree with the CPU path on the same input -- exactly where the transform is a permutation of the
pixels, within twice the tolerance of tests/warp_cases.py (both paths round) elsewhere; integer labels take the nearest pixel
with the requested fill."""
import numpy as np
import pytest
import torch

from tests import synth, warp_cases as W

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_exact_codes_equal_the_cpu_path_bit_for_bit(layout):
    from vq_seg_amd import _hip
    from vq_seg_amd.data import inverse_similarity_transform, similarity_transform
    host = synth.uniform(70, (2, 3, 16, 16), -1.0, 1.0)
    host[0, 0, 1, 2], host[1, 1, 3, 0] = float("nan"), -0.0
    if layout == "channels_last":
        host = host.contiguous(memory_format=torch.channels_last)
    dev = host.to(DEV)
    for code in (0, 1, 2, 9):
        calls = _hip.AFFINE_WARP_CALLS
        out, aug, angle = similarity_transform(dev, code)
        back = inverse_similarity_transform(out, aug, angle)
        assert _hip.AFFINE_WARP_CALLS == calls + 2 and out.is_cuda and out.stride() == dev.stride()
        want, _a, _b = similarity_transform(host, code)
        assert (aug, angle) == (code, 0.0)
        assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32)) and torch.equal(back.cpu().view(torch.int32), host.view(torch.int32))
    for code, angle in ((3, 90.0), (4, -90.0), (5, 180.0), (7, 270.0)):         # quarter turns through the inverse (a square image)
        calls = _hip.AFFINE_WARP_CALLS
        out = inverse_similarity_transform(dev, code, angle)
        assert _hip.AFFINE_WARP_CALLS == calls + 1
        assert torch.equal(out.cpu().view(torch.int32), inverse_similarity_transform(host, code, angle).view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_generic_angles_agree_with_the_cpu_path(dtype):
    from vq_seg_amd import _hip
    from vq_seg_amd.data import inverse_similarity_transform, similarity_transform
    h, w = 33, 20
    host = synth.uniform(71, (3, 3, h, w), -1.0, 1.0).to(dtype)
    dev = host.to(DEV)
    ref = host.float().numpy()
    for code in (3, 4, 5, 6, 7, 8):
        torch.manual_seed(code)
        calls = _hip.AFFINE_WARP_CALLS
        out, aug, angle = similarity_transform(dev, code)
        back = inverse_similarity_transform(dev, aug, angle)
        assert _hip.AFFINE_WARP_CALLS == calls + 2
        torch.manual_seed(code)
        want, aug_c, angle_c = similarity_transform(host, code)
        assert (aug, angle) == (aug_c, angle_c) and 0.0 < abs(angle) < 90.0 and (angle > 0) == (code in (3, 5, 7))
        want_back = inverse_similarity_transform(host, aug, angle)
        for got, exp in ((out, want), (back, want_back)):
            exp = exp.float().double().numpy()
            tol = 2 * (W.tol_f32(ref, h, w) if dtype == torch.float32 else W.tol_bf16(ref, h, w, exp))
            err = np.abs(got.float().cpu().double().numpy() - exp)
            print(f"code {code} angle {angle:.3f} {dtype}: max err {err.max():.3e}, worst err / tol {float((err / tol).max()):.3f}")
            assert (err <= tol).all()


def test_integer_labels_take_nearest_with_the_requested_fill():
    from vq_seg_amd import _hip
    from vq_seg_amd.data import inverse_similarity_transform, similarity_matrices, warp_batch
    host = synth.labels(72, (2, 17, 19)) * 2                                # classes {0, 2, 4}
    dev = host.to(DEV)
    for fill in (0, 255):
        calls = _hip.AFFINE_WARP_CALLS
        got = inverse_similarity_transform(dev, 6, -33.7, fill=fill)
        assert _hip.AFFINE_WARP_CALLS == calls + 1 and got.dtype == torch.int64 and got.is_cuda
        assert set(got.unique().tolist()) <= {0, 2, 4, fill}                # no interpolated class
        mats = similarity_matrices([6, 6], [-33.7, -33.7], inverse=True)
        want, decided = W.nearest(host.numpy()[:, None], mats, fill)
        assert decided.mean() >= 0.99 and np.array_equal(got.cpu().numpy()[:, None][decided], want[decided])
        cpu = inverse_similarity_transform(host, 6, -33.7, fill=fill).numpy()[:, None]
        assert np.array_equal(cpu[decided], want[decided])
        if fill:
            assert bool((got == fill).any()) and int(got[0, 0, 0]) == fill
    u8 = warp_batch(dev.to(torch.uint8), similarity_matrices([1, 2], [0.0, 0.0]), mode="nearest")
    assert torch.equal(u8.cpu(), torch.stack([host[0].flip(-1), host[1].flip(-2)]).to(torch.uint8))
