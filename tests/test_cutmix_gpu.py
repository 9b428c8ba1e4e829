"""The box-mix kernel (vqseg_box_mix_f) on the GPU against a torch.where restatement on the same device tensors: exactly equal, bit
for bit (compared as integer views, over random BIT patterns: -0.0, denormals, NaN payloads and all), for every element width,
layout, both modes and boxes on every edge; then CutMix / CutOut / augmentation() on GPU tensors against their CPU copies."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = {"f32": (torch.float32, torch.int32), "bf16": (torch.bfloat16, torch.int16), "i64": (torch.int64, torch.int64), "u8": (torch.uint8, torch.uint8)}
# (n, H, W): partner wrap-around with nothing 16-byte alignable; whole 1 KiB tiles; box edges inside 16-byte units of 12-byte pixels;
# the 64-sample block boundary of the kernel-argument boxes (partners 63 -> 64 and 64 -> 0); a sample that is its own partner;
# and the block boundary once more with samples large enough for the 16-byte body
SHAPES = [(3, 5, 7), (2, 16, 24), (2, 33, 65), (65, 4, 8), (1, 8, 8), (66, 16, 16)]
LAYOUTS = ["nchw", "channels_last", "labels3d"]
PLANES = 3


def make_src(n, h, w, dtype_key, layout, seed):
    """random bit patterns of the element type, with -0.0, a NaN payload and denormals planted in the first pixels of every row"""
    dt, it = DTYPES[dtype_key]
    dev = torch.device("cuda:0")
    shape = (n, h, w) if layout == "labels3d" else (n, PLANES, h, w)
    g = torch.Generator(device="cpu").manual_seed(seed)
    info = torch.iinfo(it)
    bits = torch.randint(info.min, info.max, shape, dtype=torch.int64, generator=g).to(it) if it != torch.int64 else \
        torch.randint(-(1 << 62), 1 << 62, shape, dtype=torch.int64, generator=g) * 2 + 1
    if dtype_key == "f32":
        special = torch.tensor([-0x80000000, 0x7fc12345, 0x00000001, -0x7fffffff, 0x7f800001], dtype=torch.int64).to(torch.int32)
    elif dtype_key == "bf16":
        special = torch.tensor([-0x8000, 0x7fc1, 0x0001, -0x7fff, 0x0001], dtype=torch.int64).to(torch.int16)     # ... 0x0001 0x0001: a denormal-looking pair
    else:
        special = None
    if special is not None and w >= 5:
        bits[..., :5] = special
    src = bits.to(dev).view(dt)
    if layout == "channels_last":
        src = src.contiguous(memory_format=torch.channels_last)
    return src


def box_sets(n, h, w):
    named = {"one_pixel": (h // 2, w // 2, 1, 1), "full_width": (h // 2, 0, 1, w), "full_height": (0, w // 2, h, 1),
             "top_left": (0, 0, 2, 3), "top_right": (0, w - 3, 2, 3), "bottom_left": (h - 2, 0, 2, 3), "bottom_right": (h - 2, w - 3, 2, 3),
             "whole": (0, 0, h, w), "empty_h": (1, 1, 0, 3), "empty_w": (1, 1, 2, 0), "odd": (1, 1, h - 2, w - 3)}
    sets = {k: [b] * n for k, b in named.items()}
    order = list(named.values())
    sets["per_sample"] = [order[(s * 5 + 3) % len(order)] for s in range(n)]
    return sets


def restate(bits, boxes, mode, fill_bits):
    """the semantics, on integer views: out = inside(box[s]) ? (mix: src[(s + 1) % n] | fill) : src"""
    n, (h, w) = bits.shape[0], bits.shape[-2:]
    inside = torch.zeros((n, h, w), dtype=torch.bool, device=bits.device)
    for s, (y1, x1, ch, cw) in enumerate(boxes):
        inside[s, y1:y1 + ch, x1:x1 + cw] = True
    if bits.dim() == 4:
        inside = inside[:, None]
    other = torch.roll(bits, -1, 0) if mode == "mix" else torch.full_like(bits, fill_bits)
    return torch.where(inside, other, bits)


def fill_bits_of(fill, dt, it):
    return int(torch.tensor([fill], dtype=dt).view(it).item())


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype_key", sorted(DTYPES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_the_restatement(shape, dtype_key, layout):
    from vq_seg_amd import _hip
    n, h, w = shape
    dt, it = DTYPES[dtype_key]
    src = make_src(n, h, w, dtype_key, layout, seed=n * 1000 + h * 10 + w)
    keep = src.view(it).clone()
    calls = _hip.BOX_MIX_CALLS
    fill = 255 if dt in (torch.int64, torch.uint8) else -1.5
    done = 0
    for name, boxes in box_sets(n, h, w).items():
        for mode in ("mix", "fill"):
            out = _hip.box_mix(src, boxes, mode=mode, fill=fill)
            assert out.dtype == dt and out.shape == src.shape and out.stride() == src.stride() and out.data_ptr() != src.data_ptr()
            want = restate(src.view(it), boxes, mode, fill_bits_of(fill, dt, it))
            assert torch.equal(out.view(it), want), (name, mode)
            done += 1
    assert torch.equal(src.view(it), keep)                   # src bit-unchanged
    assert _hip.BOX_MIX_CALLS == calls + done
    if n == 1:                                               # its own partner: mixing changes nothing, whatever the box
        assert torch.equal(_hip.box_mix(src, [(0, 0, h, w)]).view(it), keep)


def test_grid_stride_loop_and_preallocated_out():
    """nn_grid_cap at its minimum of 256 workgroups (1024 tiles a turn) and 3 x 3 x 300 x 301 f32 = 3175 tiles: the grid-stride loop
    takes four turns"""
    from vq_seg_amd import _hip
    src = make_src(3, 300, 301, "f32", "channels_last", seed=9)
    boxes = box_sets(3, 300, 301)["per_sample"]
    want = restate(src.view(torch.int32), boxes, "mix", 0)
    out = torch.empty_like(src)
    prev = _hip.set_option("nn_grid_cap", 256)
    try:
        got = _hip.box_mix(src, boxes, out=out)
    finally:
        _hip.set_option("nn_grid_cap", prev)
    assert got is out and torch.equal(out.view(torch.int32), want)


def test_wrong_arguments_raise_on_the_device_too():
    from vq_seg_amd import _hip
    x = torch.zeros(2, 3, 4, 6, device="cuda:0")
    with pytest.raises(_hip.HipLibraryError, match="outside"):
        _hip.box_mix(x, [(0, 0, 1, 1), (0, 0, 5, 1)])
    with pytest.raises(_hip.HipLibraryError, match="per sample"):
        _hip.box_mix(x, [(0, 0, 1, 1)])
    with pytest.raises(_hip.HipLibraryError, match="dense"):
        _hip.box_mix(x[:, :, :, ::2], [(0, 0, 1, 1)] * 2)
    with pytest.raises(_hip.HipLibraryError, match="float16"):
        _hip.box_mix(x.half(), [(0, 0, 1, 1)] * 2)


def _seed(seed):
    np.random.seed(seed)
    random.seed(seed)


def _inputs(n, h, w):
    from tests import synth
    x = synth.uniform(41, (n, 3, h, w), -1.0, 1.0)
    lab = synth.uniform(42, (n, h, w), 0.0, 3.0).long()
    logits = synth.uniform(43, (n, 3, h, w), -4.0, 4.0)
    return x, lab, logits


@pytest.mark.parametrize("cls_name", ["CutMix", "CutOut"])
def test_cutmix_object_on_the_gpu_equals_its_cpu_copy(cls_name):
    from vq_seg_amd import _hip
    from vq_seg_amd import data
    cls = getattr(data, cls_name)
    dev = torch.device("cuda:0")
    x, lab, _ = _inputs(3, 16, 24)
    for seed in (3, 4, 6):
        _seed(seed)
        cpu = cls(0.25)
        want, mask_c = cpu(x)
        want_l, _ = cpu(lab, mask_c)
        _seed(seed)
        aug = cls(0.25)
        calls = _hip.BOX_MIX_CALLS
        xg = x.to(dev).contiguous(memory_format=torch.channels_last)
        got, mask = aug(xg)
        assert _hip.BOX_MIX_CALLS == calls + 1               # the kernel, not tensor ops
        assert mask.is_cuda and mask.dtype == torch.int64 and torch.equal(mask.cpu(), mask_c)
        assert got.is_contiguous(memory_format=torch.channels_last) and torch.equal(got.cpu(), want)
        got_l, mask_2 = aug(lab.to(dev), mask)               # the returned mask handed back in: int64 labels take the kernel too
        assert _hip.BOX_MIX_CALLS == calls + 2 and mask_2 is mask
        assert got_l.dtype == torch.int64 and torch.equal(got_l.cpu(), want_l)
        foreign = mask.clone()                               # a mask this object did not make: tensor ops, the same values
        got_f, _ = aug(xg, foreign)
        got_fl, _ = aug(lab.to(dev), foreign)
        assert _hip.BOX_MIX_CALLS == calls + 2
        assert torch.equal(got_f.cpu(), want) and torch.equal(got_fl.cpu(), want_l)
        mask.zero_()                                         # a remembered mask that was written since: no longer trusted
        aug(xg, mask)
        assert _hip.BOX_MIX_CALLS == calls + 2


@pytest.mark.parametrize("name", ["cutmix", "cutout"])
def test_augmentation_on_the_gpu_equals_its_cpu_copy(name):
    from vq_seg_amd import _hip
    from vq_seg_amd.data import augmentation
    dev = torch.device("cuda:0")
    x, lab, logits = _inputs(4, 16, 24)
    _seed(11)
    want = augmentation(x, lab, logits, {"name": name, "ratio": 0.25})
    _seed(11)
    calls = _hip.BOX_MIX_CALLS
    lab_g = lab.to(dev)
    got = augmentation(x.to(dev), lab_g, logits.to(dev).contiguous(memory_format=torch.channels_last), {"name": name, "ratio": 0.25})
    assert _hip.BOX_MIX_CALLS == calls + 3                   # one kernel call per tensor
    assert torch.equal(lab_g.cpu(), lab)
    for g, w_ in zip(got, want):
        assert g.dtype == w_.dtype and torch.equal(g.cpu(), w_)
