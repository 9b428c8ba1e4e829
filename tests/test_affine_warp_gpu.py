"""The affine-warp kernel (vqseg_affine_warp_f) on the GPU.  Exact cases -- identity, flips, quarter and half turns -- against
flip / rot90 of the same device tensor, bit for bit over random BIT patterns (NaN payloads, infinities, -0.0, denormals);
generic angles against the float64 restatement of tests/warp_cases.py within its tolerance (zero padding included); nearest
on label maps wherever float64 decides the source pixel; per-sample matrices, `out=`, the call counter and the argument checks."""
import numpy as np
import pytest
import torch

from tests import synth, warp_cases as W

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LAYOUTS = ["nchw", "channels_last"]
BITS = {"f32": (torch.float32, torch.int32, "bilinear"), "bf16": (torch.bfloat16, torch.int16, "bilinear"), "u8": (torch.uint8, torch.uint8, "nearest"),
        "i16": (torch.int16, torch.int16, "nearest"), "i32": (torch.int32, torch.int32, "nearest"), "i64": (torch.int64, torch.int64, "nearest")}
IDS = ["x".join(map(str, s)) for s in W.SHAPES]


def lay(t, layout):
    return t.contiguous(memory_format=torch.channels_last) if layout == "channels_last" and t.dim() == 4 else t.contiguous()


def bit_patterns(shape, key, seed):
    """random bit patterns of the element type; for the float types -0.0, a NaN payload, a denormal, +-inf planted in every row"""
    dt, it, _mode = BITS[key]
    g = torch.Generator(device="cpu").manual_seed(seed)
    info = torch.iinfo(it)
    bits = torch.randint(info.min, info.max, shape, dtype=torch.int64, generator=g).to(it) if it != torch.int64 else \
        torch.randint(-(1 << 62), 1 << 62, shape, dtype=torch.int64, generator=g) * 2 + 1
    special = {"f32": torch.tensor([-0x80000000, 0x7fc12345, 0x00000001, 0x7f800000, -0x00800000], dtype=torch.int64).to(torch.int32),
               "bf16": torch.tensor([-0x8000, 0x7fc1, 0x0001, 0x7f80, -0x0080], dtype=torch.int64).to(torch.int16)}.get(key)
    if special is not None and shape[-1] >= 5:
        bits[..., :5] = special
    return bits.to(DEV).view(dt)


def exact_transforms(square):
    """name -> (codes, angle, the same permutation with torch ops)"""
    t = {"identity": (0, 0.0, lambda x: x), "hflip": (1, 0.0, lambda x: x.flip(-1)), "vflip": (2, 0.0, lambda x: x.flip(-2)),
         "turn180": (3, 180.0, lambda x: x.flip(-1, -2)), "hflip_turn180": (5, 180.0, lambda x: x.flip(-2))}
    if square:
        t.update(turn90=(3, 90.0, lambda x: torch.rot90(x, 1, (-2, -1))), turn270=(3, 270.0, lambda x: torch.rot90(x, 3, (-2, -1))),
                 turn_minus90=(4, -90.0, lambda x: torch.rot90(x, -1, (-2, -1))), hflip_turn90=(5, 90.0, lambda x: torch.rot90(x.flip(-1), 1, (-2, -1))),
                 vflip_turn270=(7, 270.0, lambda x: torch.rot90(x.flip(-2), 3, (-2, -1))))
    return t


@pytest.mark.parametrize("key", list(BITS))
@pytest.mark.parametrize("layout", LAYOUTS + ["labels3d"])
def test_exact_cases_pass_every_bit(key, layout):
    from vq_seg_amd import _hip
    from vq_seg_amd.data.augmentations import similarity_matrices
    dt, it, mode = BITS[key]
    shapes = [W.LABELS_3D, (2, 19, 19)] if layout == "labels3d" else W.SHAPES + W.SQUARE
    for i, shape in enumerate(shapes):
        src = lay(bit_patterns(shape, key, 100 + i), layout)
        for name, (code, angle, perm) in exact_transforms(shape[-1] == shape[-2]).items():
            mats = similarity_matrices([code] * shape[0], [angle] * shape[0])
            out = _hip.affine_warp(src, mats, mode=mode, fill=7)
            assert out.dtype == dt and out.shape == src.shape and out.stride() == src.stride()
            assert torch.equal(out.view(it), perm(src).view(it)), (shape, name)


def generic_inputs(shape, seed, bf16):
    x = synth.uniform(seed, shape, -1.0, 1.0)
    return x.bfloat16().float() if bf16 else x


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("key", ["f32", "bf16"])
@pytest.mark.parametrize("shape", W.SHAPES, ids=IDS)
def test_generic_bilinear_against_the_float64_restatement(shape, key, layout):
    from vq_seg_amd import _hip
    n, _p, h, w = shape
    dt = BITS[key][0]
    host = generic_inputs(shape, 31, key == "bf16")
    src = lay(host.to(DEV).to(dt), layout)
    worst = 0.0
    for flip in (None, "h", "v"):
        for angle in W.ANGLES:
            mats = W.matrices(angle, flip, n)
            got = _hip.affine_warp(src, mats).float().cpu().double().numpy()
            want = W.bilinear(host.numpy(), mats)                           # every pixel: the zero padding is part of what is compared
            tol = W.tol_f32(host.numpy(), h, w) if key == "f32" else W.tol_bf16(host.numpy(), h, w, want)
            err = np.abs(got - want)
            worst = max(worst, float((err / tol).max()))
            print(f"{shape} {key} {layout} flip={flip} angle={angle}: max err {err.max():.3e}, worst err / tol {float((err / tol).max()):.3f}")
            assert (err <= tol).all(), (flip, angle, float(err.max()))
    assert worst > 0.0 or h * w == 1


@pytest.mark.parametrize("layout", LAYOUTS + ["labels3d"])
@pytest.mark.parametrize("fill", [0, 255])
def test_generic_nearest_on_label_maps(layout, fill):
    from vq_seg_amd import _hip
    shapes = [W.LABELS_3D] if layout == "labels3d" else W.SHAPES
    for i, shape in enumerate(shapes):
        host = synth.labels(40 + i, shape, num_classes=250) + 1                 # 1..250: neither fill value is a label
        src = lay(host.to(DEV), layout)
        host4 = host.numpy() if host.dim() == 4 else host.numpy()[:, None]
        for flip in (None, "h", "v"):
            for angle in W.ANGLES:
                mats = W.matrices(angle, flip, shape[0])
                got = _hip.affine_warp(src, mats, mode="nearest", fill=fill).cpu().numpy().reshape(host4.shape)
                want, decided = W.nearest(host4, mats, fill)
                if angle == 89.99 and (shape[-2] + shape[-1]) % 2 == 1:
                    # one odd and one even side: the exact quarter turn maps pixel centres onto HALF-integer source coordinates (an integer
                    # offset from one centre plus the other, half-integer, centre), and 89.99 degrees moves them by sin(0.01 deg) = 1.7e-4 per
                    # pixel of distance from the centre line -- inside the 1e-3 band for every pixel closer than 5.7 to it.  The 1 % bound
                    # cannot hold for this one geometry whatever the kernel does; the decided pixels (those farther out) are still compared
                    assert 0.2 <= decided.mean() < 0.99, (shape, flip, angle)
                else:
                    assert 1.0 - decided.mean() <= 0.01, (shape, flip, angle, 1.0 - decided.mean())
                decided = np.broadcast_to(decided, host4.shape)
                assert np.array_equal(got[decided], want[decided]), (shape, flip, angle)
                if angle != 0.001 and min(shape[-2:]) >= 17:
                    assert (want == fill).any()                                 # some pixel does come from outside the image


def test_per_sample_matrices_equal_single_sample_calls():
    from vq_seg_amd import _hip
    from vq_seg_amd.data.augmentations import similarity_matrices
    src = synth.uniform(50, (3, 3, 17, 19), -1.0, 1.0).to(DEV)
    lab = synth.labels(51, (3, 17, 19)).to(DEV)
    mats = similarity_matrices([1, 3, 8], [0.0, 17.3, -33.7])
    for t, mode in ((src, "bilinear"), (lay(src, "channels_last"), "bilinear"), (src.bfloat16(), "bilinear"), (lab, "nearest"), (lab.to(torch.uint8), "nearest")):
        whole = _hip.affine_warp(t, mats, mode=mode)
        for s in range(3):
            one = _hip.affine_warp(t[s:s + 1], mats[s:s + 1], mode=mode)              # a slice of samples is dense in either layout
            assert torch.equal(whole[s:s + 1], one), (mode, s)
        assert not torch.equal(whole[1], whole[2])


@pytest.mark.parametrize("layout", LAYOUTS + ["labels3d"])
def test_out_is_written_in_place_and_may_have_a_larger_sample_stride(layout):
    from vq_seg_amd import _hip
    shape = W.LABELS_3D if layout == "labels3d" else (2, 3, 17, 19)
    src = lay(synth.uniform(60, shape, -1.0, 1.0).to(DEV), layout)
    mats = W.matrices(17.3, "h", 2)
    want = _hip.affine_warp(src, mats)
    calls = _hip.AFFINE_WARP_CALLS
    out = torch.empty_like(src)
    assert _hip.affine_warp(src, mats, out=out) is out and torch.equal(out, want)
    big = lay(torch.full((4,) + tuple(shape[1:]), -5.0, device=DEV), layout)
    view = big[::2]                                                         # samples two samples apart
    assert view.stride(0) == 2 * src.stride(0)
    assert _hip.affine_warp(src, mats, out=view) is view
    assert torch.equal(big[0], want[0]) and torch.equal(big[2], want[1])
    assert bool((big[1] == -5.0).all()) and bool((big[3] == -5.0).all())     # nothing written between the samples
    assert _hip.AFFINE_WARP_CALLS == calls + 2


def test_bad_arguments_on_device_tensors_raise_without_a_launch():
    from vq_seg_amd import _hip
    x = torch.zeros(2, 3, 4, 6, device=DEV)
    ok = W.matrices(17.3, None, 2)
    calls = _hip.AFFINE_WARP_CALLS
    nan = ok.copy()
    nan[0, 1] = float("nan")
    shifted = ok.copy()
    shifted[1, 2] = 1.0
    cases = [(dict(src=x.double()), "float64"), (dict(src=x.long(), mode="bilinear"), "int64"), (dict(out=x), "out of place"),
             (dict(out=torch.zeros(2, 3, 4, 5, device=DEV)), "shape and layout"), (dict(out=lay(torch.zeros(2, 3, 4, 6, device=DEV), "channels_last")), "shape and layout"),
             (dict(out=torch.zeros(2, 3, 4, 6)), "no CPU fallback"), (dict(out=torch.zeros(2, 3, 4, 6, device=DEV, dtype=torch.bfloat16)), "bfloat16|float32"),
             (dict(src=torch.zeros(2, 3, 4, 12, device=DEV)[..., ::2]), "dense"), (dict(matrices=ok[:1]), "per sample"), (dict(matrices=nan), "finite"),
             (dict(matrices=shifted), "reserved"), (dict(mode="bicubic"), "mode"), (dict(src=torch.zeros(0, 3, 4, 6, device=DEV), matrices=ok[:0]), "empty")]
    for kw, match in cases:
        args = dict(src=x, matrices=ok, mode="bilinear")
        args.update(kw)
        with pytest.raises(_hip.HipLibraryError, match=match):
            _hip.affine_warp(args.pop("src"), args.pop("matrices"), **args)
    assert _hip.AFFINE_WARP_CALLS == calls
