"""The layer census without a GPU: tests/layer_cases.py's table equals the convolutions the benchmark's model has, the two fp64
weight-gradient references agree on its rows, and the weight-gradient bar (max |gw - ref| < 2e-5 max |ref|, test_wgrad3x3_fused_taps')
passes the kernels' arithmetic emulated on the CPU and fails a reduce that stops at its grid cap, a 1-D grid decode that masks with
t_all - 1 instead of taking the modulus, and a concat source switched one ci tile late."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests import layer_cases as lc
from tests.test_nn_gpu import _wgrad_ref_by_taps, rel

BAR = 2e-5


def _model_geometries():
    """{(c1, c2, cout, k, stride, pad, reflect, (n, h, w), dgrad path)} of every convolution of bench.py's model that runs on the conv
    kernels, and the modules left out"""
    import bench
    from vq_seg_amd.models.encoders.resnet import Bottleneck
    from vq_seg_amd.models.networks import make_model
    wl = bench.WORKLOADS["cfg3"]
    model = make_model(bench.model_cfg("cfg3"))
    batch, size = wl["batch"], wl["size"]
    seen, left_out = set(), []

    def add(conv, c1, c2, h, role):
        k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        assert conv.bias is None and conv.in_channels == c1 + c2 and conv.kernel_size == (k, k)
        reflect = conv.padding_mode == "reflect" and p > 0
        if role == "conv1":
            path = "shortcut"
        elif k == 3 and s == 1 and reflect:
            path = "ring"
        elif k == 3 and s == 2:
            path = "folded"
        elif k == 1 and s == 2:
            path = "classes"
        else:
            path = "generic"
        seen.add((c1, c2, conv.out_channels, k, s, p, reflect, (batch, h, h), path))

    enc = model.encoder
    left_out.append(enc.conv1)                              # the 7 x 7 stem: nn_stem.hip
    h = size // 4                                           # stem / 2, max pool / 2
    for layer in (enc.layer1, enc.layer2, enc.layer3, enc.layer4):
        for blk in layer:
            assert isinstance(blk, Bottleneck)
            ho = h // blk.stride
            add(blk.conv1, blk.conv1.in_channels, 0, h, "conv1")
            add(blk.conv2, blk.conv2.in_channels, 0, h, "conv2")
            add(blk.conv3, blk.conv3.in_channels, 0, ho, "conv3")
            if blk.downsample is not None:
                add(blk.downsample[0], blk.downsample[0].in_channels, 0, h, "down")
            h = ho
    skips = list(enc.out_channels()[1:])[::-1]              # deep -> shallow; the decoder concatenates (upsampled, skip)
    prev, h = 0, size // 32
    for i, block in enumerate(model.decoder.blocks):
        first, second = block[0][0], block[1][0]
        add(first, prev if prev else skips[i], skips[i] if prev else 0, h, "decoder")
        add(second, second.in_channels, 0, h, "decoder")
        prev, h = second.out_channels, h * 2
    left_out.append(model.segmentation_head)                # the 1 x 1 head: nn_head.hip
    convs = [m for m in model.modules() if isinstance(m, nn.Conv2d)]
    return seen, left_out, convs


def test_the_table_equals_the_models_convolutions():
    """Every nn.Conv2d of make_model(bench.model_cfg("cfg3")) is walked (encoder Bottlenecks by role, the decoder's concat order for
    c1 / c2) or named as left out (stem, head); the set of geometries with their benchmark sizes and data-gradient paths equals the
    table's, which names every geometry once.  A new layer fails here until someone adds a row."""
    seen, left_out, convs = _model_geometries()
    assert len(convs) == 53 + 10 + 1 and len(left_out) == 2         # ResNet-50's 53 convolutions, five double blocks, the head
    assert type(left_out[1]).__name__ == "_Head1x1" and left_out[0].kernel_size == (7, 7)
    table = [tuple(r[1:]) for r in lc.ROWS]
    assert len(set(table)) == len(table) == len(lc.ROWS)
    assert set(table) == seen, (set(table) - seen, seen - set(table))
    assert set(lc.SIZES) == set(lc.IDS) == set(lc.BY_NAME) and set(lc.EXCEPTIONS) <= set(lc.BY_NAME)
    assert not any(tuple(r[1:8]) in {t[:7] for t in table} for r in lc.EXTRA_WGRAD_ROWS)


def test_the_tile_counts_the_one_dimensional_grid_decodes():
    """The rows that take the XCD-aware 1-D grid at their eight-slab size and their (ci, co) tile counts: the model's own are powers
    of two and 3 (d4.0), among them 32 (512 -> 512 at stride 1 and 2, (512 + 512) -> 256, 512 -> 2048, 2048 -> 512); the two extra rows
    add 6 and 12.  Rows without an eight-slab size have one tile or a plan below 8 slabs (one resident round / tiles)."""
    counts = {r.name: lc.wgrad_tiles(r)[2] for r in lc.ROWS + lc.EXTRA_WGRAD_ROWS}
    xcd = {name: t for name, t in counts.items() if lc.SIZES[name].wgrad8 is not None}
    assert all(t > 1 for t in xcd.values())
    assert {3, 6, 12, 32} <= set(xcd.values())
    assert (xcd["d4.0"], xcd["x6"], xcd["x12"], xcd["d1.1"], xcd["l4.conv2"], xcd["l4.0.conv2"], xcd["d2.0"]) == (3, 6, 12, 32, 32, 32, 32)
    assert {t for name, t in xcd.items() if lc.BY_NAME[name].k == 1} == {2, 4, 8, 16, 32}       # the model's 1x1 counts: all powers of two
    for name, t in counts.items():
        if lc.SIZES[name].wgrad8 is None:
            assert t == 1 or t >= 64, name
    for name in ("d1.1", "l4.conv2", "l4.0.conv2", "d2.0", "d1.0", "d0.0", "d0.1"):
        r = lc.BY_NAME[name]
        assert r.cout * 9 * (r.c1 + r.c2) > lc.REDUCE_CAP


def _conv2d_weight(row, size):
    x, gy = lc.wgrad_operands(row, size)
    xp = x.double().permute(0, 3, 1, 2)
    if row.pad:
        xp = F.pad(xp, (row.pad,) * 4, mode="reflect" if row.reflect else "constant")
    return torch.nn.grad.conv2d_weight(xp, (row.cout, row.c1 + row.c2, row.k, row.k), gy.double().permute(0, 3, 1, 2), stride=row.stride)


@pytest.mark.parametrize("name", ["l2.conv2", "l2.0.conv2", "d4.0"])
def test_the_reference_by_taps_equals_conv2d_weight(name):
    """a stride-1 reflect row, a stride-2 row and a concat row at their one-block sizes: both fp64, equal to 1e-13 of scale"""
    row, size = lc.BY_NAME[name], lc.SIZES[name].wgrad
    x, gy = lc.wgrad_operands(row, size)
    by_taps = _wgrad_ref_by_taps(x, gy, row.k, row.stride, row.reflect)
    assert rel(by_taps, _conv2d_weight(row, size)) < 1e-13


TEETH = [
    # row, size, slabs of the emulation, mutation
    ("d1.1", "wgrad", 1, "reduce_cap"),                     # 3x3 512 -> 512: 2 359 296 slab elements
    ("x6", "wgrad8", 8, "mask_decode"),                     # 6 tiles: the mask 5 never names tiles 2 and 3
    ("d4.0", "wgrad8", 16, "mask_decode"),                  # 3 tiles, the model's own odd count: the mask 2 never names tile 1
    ("d4.0", "wgrad", 1, "late_switch"),                    # C1 = 128, 64-channel ci tiles: the skip's only tile
    ("x12", "wgrad", 1, "late_switch"),                     # C1 = 256, twelve ci tiles
]


@pytest.mark.parametrize("name,which,slabs,mutation", TEETH, ids=[f"{t[0]}-{t[3]}" for t in TEETH])
def test_the_weight_gradient_bar_has_teeth_at_these_shapes(name, which, slabs, mutation):
    row, size = lc.BY_NAME[name], getattr(lc.SIZES[name], which)
    x, gy = lc.wgrad_operands(row, size)
    ref = _wgrad_ref_by_taps(x, gy, row.k, row.stride, row.reflect)
    good = rel(lc.emulate_wgrad(row, size, slabs), ref)
    bad = rel(lc.emulate_wgrad(row, size, slabs, mutation), ref)
    print(f"{name} {size} {slabs} slab(s): emulation {good / BAR:.3g} of the bar, {mutation} {bad / BAR:.3g}")
    assert good < BAR
    assert not bad < BAR
