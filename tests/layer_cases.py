"""The census of the convolution geometries the benchmark's model runs on the conv kernels (bench.py: model_cfg("cfg3"), vqreptunet1x1
on a ResNet-50 encoder, 32 images of 512 x 512 per forward), with the test size of each row's forward, data-gradient and
weight-gradient launch.  tests/test_layer_census_gpu.py runs the kernels at these sizes against fp64 and, with zero-filled buffers, at
the benchmark's own sizes to see that both take the same instantiation; tests/test_layer_census_cpu.py holds the table against the
model, the weight-gradient references against each other, and shows without a GPU that the weight-gradient bar sees a reduce that
stops at its grid cap, a (tile, slab) decode that masks instead of taking the modulus, and a concat source switched one tile late.

What is NOT in the table, because it does not run on the conv kernels: the 7 x 7 stem (nn_stem.hip, tests/test_stem_kernels_gpu.py)
and the 1 x 1 head (nn_head.hip, tests/test_nn_kernels_gpu.py).  The model has no 1 x 1 VQ projections.

Operands are bf16-exact (tests/synth.py through fast_cases / precise_cases), references fp64 (fast_cases.reference,
precise_cases.reference, test_nn_gpu._wgrad_ref_by_taps): nothing here restates their arithmetic."""
from collections import namedtuple

from tests import fast_cases as fc

# c1 + c2 input channels (c2: the decoder's skip, concatenated behind the upsampled c1), bench: (n, h, w) of the layer's INPUT in one
# forward of the benchmark; dgrad: the path nnf._dgrad takes for the layer in the bf16 step
#   ring      3x3 stride 1 reflect (Bottleneck conv2): the zero-padded gradient on the patch kernel + vqseg_reflect_ring_f
#   shortcut  Bottleneck conv1: the block input's shortcut gradient is added in the convolution's epilogue (vqseg_conv2d_affine_f)
#   folded    3x3 stride 2 reflect: vqseg_conv2d_dgrad_s2_fold_f
#   classes   1x1 stride 2 projection: vqseg_conv2d_dgrad_s2_f, accumulating onto the other consumer's gradient
#   generic   vqseg_conv2d_f over gy with the transposed, tap-flipped image, one launch per concat source
Row = namedtuple("Row", "name c1 c2 cout k stride pad reflect bench dgrad")

B = 32                                                      # images per forward (bench.py WORKLOADS["cfg3"]["batch"])
ROWS = [
    # encoder: ResNet-50 Bottlenecks, reflect padding on their 3x3 convs; stage inputs 128^2, 128^2, 64^2, 32^2
    Row("l1.0.conv1", 64, 0, 64, 1, 1, 0, False, (B, 128, 128), "shortcut"),
    Row("l1.conv2", 64, 0, 64, 3, 1, 1, True, (B, 128, 128), "ring"),
    Row("l1.conv3", 64, 0, 256, 1, 1, 0, False, (B, 128, 128), "generic"),          # and layer1's projection shortcut
    Row("l1.conv1", 256, 0, 64, 1, 1, 0, False, (B, 128, 128), "shortcut"),
    Row("l2.0.conv1", 256, 0, 128, 1, 1, 0, False, (B, 128, 128), "shortcut"),
    Row("l2.0.conv2", 128, 0, 128, 3, 2, 1, True, (B, 128, 128), "folded"),
    Row("l2.conv3", 128, 0, 512, 1, 1, 0, False, (B, 64, 64), "generic"),
    Row("l2.0.down", 256, 0, 512, 1, 2, 0, False, (B, 128, 128), "classes"),
    Row("l2.conv1", 512, 0, 128, 1, 1, 0, False, (B, 64, 64), "shortcut"),
    Row("l2.conv2", 128, 0, 128, 3, 1, 1, True, (B, 64, 64), "ring"),
    Row("l3.0.conv1", 512, 0, 256, 1, 1, 0, False, (B, 64, 64), "shortcut"),
    Row("l3.0.conv2", 256, 0, 256, 3, 2, 1, True, (B, 64, 64), "folded"),
    Row("l3.conv3", 256, 0, 1024, 1, 1, 0, False, (B, 32, 32), "generic"),
    Row("l3.0.down", 512, 0, 1024, 1, 2, 0, False, (B, 64, 64), "classes"),
    Row("l3.conv1", 1024, 0, 256, 1, 1, 0, False, (B, 32, 32), "shortcut"),
    Row("l3.conv2", 256, 0, 256, 3, 1, 1, True, (B, 32, 32), "ring"),
    Row("l4.0.conv1", 1024, 0, 512, 1, 1, 0, False, (B, 32, 32), "shortcut"),
    Row("l4.0.conv2", 512, 0, 512, 3, 2, 1, True, (B, 32, 32), "folded"),
    Row("l4.conv3", 512, 0, 2048, 1, 1, 0, False, (B, 16, 16), "generic"),
    Row("l4.0.down", 1024, 0, 2048, 1, 2, 0, False, (B, 32, 32), "classes"),
    Row("l4.conv1", 2048, 0, 512, 1, 1, 0, False, (B, 16, 16), "shortcut"),
    Row("l4.conv2", 512, 0, 512, 3, 1, 1, True, (B, 16, 16), "ring"),
    # decoder: zero padding, (upsampled + skip) -> out, out -> out at the skip's size
    Row("d0.0", 2048, 0, 1024, 3, 1, 1, False, (B, 16, 16), "generic"),
    Row("d0.1", 1024, 0, 1024, 3, 1, 1, False, (B, 16, 16), "generic"),
    Row("d1.0", 1024, 1024, 512, 3, 1, 1, False, (B, 32, 32), "generic"),
    Row("d1.1", 512, 0, 512, 3, 1, 1, False, (B, 32, 32), "generic"),
    Row("d2.0", 512, 512, 256, 3, 1, 1, False, (B, 64, 64), "generic"),
    Row("d2.1", 256, 0, 256, 3, 1, 1, False, (B, 64, 64), "generic"),
    Row("d3.0", 256, 256, 128, 3, 1, 1, False, (B, 128, 128), "generic"),
    Row("d3.1", 128, 0, 128, 3, 1, 1, False, (B, 128, 128), "generic"),
    Row("d4.0", 128, 64, 32, 3, 1, 1, False, (B, 256, 256), "generic"),
    Row("d4.1", 32, 0, 32, 3, 1, 1, False, (B, 256, 256), "generic"),
]
# Not in the model: two weight-gradient-only geometries whose nine-tap plans have 6 and 12 (ci, co) tiles.  The model's own plans have
# 1, 2, 3, 4, 8, 16, 32, 64, 128 or 256 tiles -- `q % t_all` meets one count that is no power of two (3, d4.0) -- so these two keep the
# decode honest at the other small counts a decoder with other widths would give.
EXTRA_WGRAD_ROWS = [
    Row("x6", 128, 256, 64, 3, 1, 1, False, None, None),
    Row("x12", 256, 512, 128, 3, 1, 1, False, None, None),
]
BY_NAME = {r.name: r for r in ROWS + EXTRA_WGRAD_ROWS}


def geometry(row):
    """what identifies a layer: (c1, c2, cout, k, stride, pad, reflect) and the benchmark's input size"""
    return row[1:9]


def out_size(row, size):
    n, h, w = size
    return (h + 2 * row.pad - row.k) // row.stride + 1, (w + 2 * row.pad - row.k) // row.stride + 1


# ---------------------------------------------------------------------------------------------------------------------------
# Test sizes.  fwd / dgrad / wgrad: the smallest (n, h, w) of the layer's INPUT at which the launch reads back the benchmark-size
# `conv_last_variant` id (bit 0, the grid mapping, ignored); weight gradients take two images so that the same size also runs as two
# uses (vqseg_conv2d_wgrad2_f).  wgrad8: the "eight slabs" size where the plan can give 8 or more slabs of several tiles (the XCD-aware
# 1-D grid, id bit 0); None: the plan stays below 8 slabs (or has one tile) at every size -- 3-D grid only.
# ---------------------------------------------------------------------------------------------------------------------------
Sizes = namedtuple("Sizes", "fwd dgrad wgrad wgrad8")
PATCH = {"conv3x3_patch_min_workgroups": 1, "conv3x3_patch_tile512_min_workgroups": 1}     # the patch kernel's grid bars lowered (fast_cases.TALL)
NARROW = {**PATCH, "conv3x3_patch_wide_tile": 0}            # ... and the 256-channel tile off: at 16^2 the benchmark's 64 wide workgroups do not fill the chip

G = (2, 9, 11)                                              # 198 pixels: a full 128-row tile and a ragged one (fast_cases C1)
G2 = (2, 17, 15)                                            # stride 2 on odd sizes -> 9 x 8 (fast_cases C2 / C3 / S1)
F2 = (2, 8, 12)                                             # the one-launch stride-2 gradient needs even sizes (fast_cases R1)
P8 = (1, 16, 64)                                            # patch kernel, W % 32 == 0: 2 x 2 tiles of 8 x 32 pixels
P16 = (1, 32, 48)                                           # ... else 16 x 16 tiles, 2 x 3 an image
P16S = (2, 16, 16)                                          # ... the rows with 9 M and more weights: one tile an image, the reference stays quick
T512 = (1, 32, 64)                                          # 512-pixel tiles of 16 x 32, 2 x 2
W3, W3S2, W1 = (2, 4, 16), (2, 4, 32), (2, 8, 8)            # one block of the nine-tap plans (stride 1, stride 2) / two 64-pixel stages
E3, E3S2, E1, E1S2 = (2, 32, 64), (2, 64, 128), (2, 32, 32), (2, 64, 64)     # 4096 / 4096 / 2048 / 2048 output pixels

SIZES = {
    "l1.0.conv1": Sizes(G, G, W1, None), "l1.conv2": Sizes(T512, T512, W3, None), "l1.conv3": Sizes(G, G, W1, None),
    "l1.conv1": Sizes(G, G, W1, E1), "l2.0.conv1": Sizes(G, G, W1, E1), "l2.0.conv2": Sizes(G2, F2, W3S2, E3S2),
    "l2.conv3": Sizes(G, G, W1, E1), "l2.0.down": Sizes(G2, G2, W1, E1S2), "l2.conv1": Sizes(G, G, W1, E1),
    "l2.conv2": Sizes(P8, P8, W3, E3), "l3.0.conv1": Sizes(G, G, W1, E1), "l3.0.conv2": Sizes(G2, F2, W3S2, E3S2),
    "l3.conv3": Sizes(G, G, W1, E1), "l3.0.down": Sizes(G2, G2, W1, E1S2), "l3.conv1": Sizes(G, G, W1, E1),
    "l3.conv2": Sizes(P8, P8, W3, E3), "l4.0.conv1": Sizes(G, G, W1, E1), "l4.0.conv2": Sizes(G2, F2, W3S2, E3S2),
    "l4.conv3": Sizes(G, G, W1, E1), "l4.0.down": Sizes(G2, G2, W1, None), "l4.conv1": Sizes(G, G, W1, E1),
    "l4.conv2": Sizes(P16, P16, W3, E3),
    "d0.0": Sizes(P16S, P16S, W3, None), "d0.1": Sizes(P16S, P16S, W3, None), "d1.0": Sizes(P16S, P16S, W3, None),
    "d1.1": Sizes(P8, P8, W3, E3), "d2.0": Sizes(P8, P8, W3, E3), "d2.1": Sizes(P8, P8, W3, E3), "d3.0": Sizes(P8, P8, W3, E3),
    "d3.1": Sizes(P8, P8, W3, E3), "d4.0": Sizes(T512, P8, W3, E3), "d4.1": Sizes(T512, T512, W3, None),
    "x6": Sizes(None, None, W3, E3), "x12": Sizes(None, None, W3, E3),
}
# options under which the test size reaches the benchmark's instantiation (default options where a row is not named)
OPTIONS = {name: PATCH for name in ("l1.conv2", "l2.conv2", "l3.conv2", "d0.0", "d0.1", "d1.0", "d1.1", "d2.0", "d2.1", "d3.0", "d3.1", "d4.0", "d4.1")}
OPTIONS["l4.conv2"] = NARROW


# ---------------------------------------------------------------------------------------------------------------------------
# `conv_last_variant` at the test size, under OPTIONS (conv_internal.h spells the digits): the forward launch, the data-gradient launches
# in order (ring: the zero-padded gradient, then the ring convolution; generic: one per concat source; classes: the 1 x 1 class), the
# weight gradient at the one-block size (the eight-slab size reads back the same id with bit 0 set).  test_layer_census_gpu asserts
# every one, and that the benchmark's size reads back the same id modulo bit 0 -- apart from EXCEPTIONS.
# ---------------------------------------------------------------------------------------------------------------------------
Ids = namedtuple("Ids", "fwd dgrad wgrad")
IDS = {
    "l1.0.conv1": Ids(0x1124314, (0x1124314,), 0x5022000),
    "l1.conv2": Ids(0x3220110, (0x3220110, 0x1124310), 0x4022100),
    "l1.conv3": Ids(0x1144245, (0x1124314,), 0x5082000),
    "l1.conv1": Ids(0x1124314, (0x1144245,), 0x5024000),
    "l2.0.conv1": Ids(0x1144144, (0x1144145,), 0x5044000),
    "l2.0.conv2": Ids(0x1144210, (0x1144142,), 0x4042200),
    "l2.conv3": Ids(0x1144145, (0x1144144,), 0x5084000),
    "l2.0.down": Ids(0x1144141, (0x1144141,), 0x5084000),
    "l2.conv1": Ids(0x1144144, (0x1144145,), 0x5044000),
    "l2.conv2": Ids(0x3143210, (0x3143210, 0x1144210), 0x4042100),
    "l3.0.conv1": Ids(0x1144145, (0x1144145,), 0x5084000),
    "l3.0.conv2": Ids(0x1144211, (0x1144212,), 0x4042200),
    "l3.conv3": Ids(0x1144145, (0x1144215,), 0x5084000),
    "l3.0.down": Ids(0x1144141, (0x1144211,), 0x5084000),
    "l3.conv1": Ids(0x1144215, (0x1144145,), 0x5084000),
    "l3.conv2": Ids(0x3182200, (0x3182200, 0x1144211), 0x4042100),
    "l4.0.conv1": Ids(0x1144215, (0x1144145,), 0x5084000),
    "l4.0.conv2": Ids(0x1144211, (0x1144212,), 0x4042200),
    "l4.conv3": Ids(0x1144144, (0x1144215,), 0x5084000),
    "l4.0.down": Ids(0x1144210, (0x1144211,), 0x5084000),
    "l4.conv1": Ids(0x1144215, (0x1144144,), 0x5084000),
    "l4.conv2": Ids(0x3143210, (0x3143210, 0x1144211), 0x4042100),
    "d0.0": Ids(0x3182200, (0x3182200,), 0x4042100),
    "d0.1": Ids(0x3182200, (0x3182200,), 0x4042100),
    "d1.0": Ids(0x3182200, (0x3182200, 0x3182200), 0x4042100),
    "d1.1": Ids(0x3182200, (0x3182200,), 0x4042100),
    "d2.0": Ids(0x3182200, (0x3182200, 0x3182200), 0x4042100),
    "d2.1": Ids(0x3182200, (0x3182200,), 0x4042100),
    "d3.0": Ids(0x3143210, (0x3182200, 0x3182200), 0x4042100),
    "d3.1": Ids(0x3143210, (0x3143210,), 0x4042100),
    "d4.0": Ids(0x3210110, (0x3140110, 0x3120110), 0x4012100),
    "d4.1": Ids(0x3210110, (0x3210110,), 0x4011100),
    "x6": Ids(None, None, 0x4022100),
    "x12": Ids(None, None, 0x4042100),
}

# row -> (launch, id at the benchmark's size, why no small size reaches it).  That launch of these rows runs at the nearest
# instantiation, the 128-row tile with the same BN and prologue.
EXCEPTIONS = {
    "l3.0.down": ("dgrad", 0x1248311, "the eight-wave 256 x 128 tile needs 512 workgroups: the 1x1 class's 32768 gradient pixels at four chunks -- the benchmark's own size"),
    "l2.0.conv2": ("fwd", 0x1248310, "the eight-wave 256 x 128 tile needs 512 workgroups: 131072 output pixels at one Cout chunk -- the benchmark's own size"),
    "l4.0.conv1": ("fwd", 0x1248315, "the eight-wave 256 x 128 tile needs 512 workgroups: 32768 pixels at four Cout chunks -- the benchmark's own size"),
    "l4.0.down": ("fwd", 0x1248310, "the eight-wave 256 x 128 tile needs 512 workgroups: 8192 output pixels at 16 Cout chunks -- the benchmark's own size"),
}
# (that tile is held to fp64 at 576 -> 2048 / 1024 1x1, 1x1 stride 2 and 64 -> 1024 3x3 stride 2 reflect: dispatch_cases E1 .. E4)

PRECISE_ROWS = ["d1.1", "d2.0"]                             # fp32 forward, data and weight gradient: a 3x3 at 512 channels, a wide concat row
PRECISE_IDS = Ids(0x2040110, (0x2040110, 0x2040110), 0x6044010)     # conv_igemm_kernel<128, true, 32>, conv_wgrad_kernel<4, 4, true>
PRECISE_SIZE = (2, 7, 10)                                   # two of precise_cases W1's images: 140 pixels, a ragged last 32-pixel stage

REDUCE_CAP = 8192 * 256                                     # launch_wgrad_reduce: the elements one trip of wgrad_reduce_kernel's grid covers


def wgrad_tiles(row):
    """(cot, cit, (ci, co) tiles) of the LDS-DMA weight-gradient plan the bf16 launch takes (wgrad3x3_plan / wgrad1x1_plan, conv_wgrad.hip):
    what `t_all` is in the kernels' 1-D grid decode"""
    cin = row.c1 + row.c2
    if row.k == 3:
        cit = 2 if cin % 64 == 0 and (not row.c2 or row.c1 % 64 == 0) else 1
        cot = 4 if row.cout % 128 == 0 else 2 if row.cout % 64 == 0 else 1
    else:
        cot, cit = next((o, i) for o, i in ((8, 4), (8, 2), (4, 4), (4, 2), (2, 4), (2, 2)) if row.cout % (32 * o) == 0 and cin % (32 * i) == 0)
    return cot, cit, (cin // (32 * cit)) * (row.cout // (32 * cot))


def fast_case(row, kind, size):
    """the row as a fast_cases geometry tuple: kind "fwd", "dgrad" or "fold" at input size (n, h, w)"""
    return (kind,) + tuple(size) + (row.c1, row.c2, row.cout, row.k, row.stride, row.pad, row.reflect)


def precise_case(row, kind, size, accumulate=0):
    """the row as a precise_cases row"""
    return fast_case(row, kind, size) + (accumulate,)


def wgrad_operands(row, size):
    """(x [n, h, w, cin], gy [n, ho, wo, cout]) bf16-exact in fp32: fast_cases' generators (the forward case's x, the gradient case's gy)"""
    return fc.operands(fast_case(row, "fwd", size))[0], fc.operands(fast_case(row, "dgrad", size))[0]


# ---------------------------------------------------------------------------------------------------------------------------
# the weight-gradient kernels' arithmetic on the CPU, and three ways their host plan and grid decode go wrong
# ---------------------------------------------------------------------------------------------------------------------------
def emulate_wgrad(row, size, slabs=1, mutation=None):
    """[cout, cin, k, k] fp32.  Products of bf16 values are exact in fp32; a workgroup sums its slab's pixels in fp32 (one fp32 matmul
    per tap and slab, the pixels cut into `slabs` runs), the reduce sums the slabs in fp64 and rounds once.  Mutations (values only):
      reduce_cap   the reduce stops after REDUCE_CAP elements of the slab layout [cout][kh][kw][cin]: the rest of gw is never written (0)
      mask_decode  the 1-D grid's workgroup q takes tile `q & (t_all - 1)` instead of `q % t_all`: tiles nobody takes stay unwritten (0)
      late_switch  the concat source switches one ci tile late: the first tile of the second source reads the first source's last tile"""
    import torch
    import torch.nn.functional as F
    x, gy = wgrad_operands(row, size)
    n, ho, wo, cout = gy.shape
    cin, k = row.c1 + row.c2, row.k
    cot, cit, tiles = wgrad_tiles(row)
    if mutation == "late_switch":
        assert row.c2 and row.c1 >= 32 * cit
        x = x.clone()
        x[..., row.c1:row.c1 + 32 * cit] = x[..., row.c1 - 32 * cit:row.c1]
    xp = F.pad(x.permute(0, 3, 1, 2), (row.pad,) * 4, mode="reflect" if row.reflect else "constant").permute(0, 2, 3, 1) if row.pad else x
    g = gy.reshape(-1, cout)
    m = g.shape[0]
    cuts = [m * z // slabs for z in range(slabs + 1)]
    part = torch.zeros(slabs, cout, k, k, cin)
    for kh in range(k):
        for kw in range(k):
            win = xp[:, kh:kh + (ho - 1) * row.stride + 1:row.stride, kw:kw + (wo - 1) * row.stride + 1:row.stride, :].reshape(m, cin)
            for z in range(slabs):
                part[z, :, kh, kw] = g[cuts[z]:cuts[z + 1]].t() @ win[cuts[z]:cuts[z + 1]]
    if mutation == "mask_decode":
        assert tiles > 1 and slabs >= 8
        taken = {q & (tiles - 1) for q in range(tiles * ((slabs + 7) // 8))}
        ci_tiles = cin // (32 * cit)
        for t in set(range(tiles)) - taken:
            bx, by = t % ci_tiles, t // ci_tiles
            part[:, by * 32 * cot:(by + 1) * 32 * cot, :, :, bx * 32 * cit:(bx + 1) * 32 * cit] = 0
    gw = part.double().sum(0).float()
    if mutation == "reduce_cap":
        assert gw.numel() > REDUCE_CAP
        gw.reshape(-1)[REDUCE_CAP:] = 0
    return gw.permute(0, 3, 1, 2).contiguous()
