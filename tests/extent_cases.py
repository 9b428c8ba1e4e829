"""The case table of the extent suite (tests/test_extent_gpu.py): for every training-step entry point of include/vqseg.h a ragged
shape -- every tiled or vectorised dimension one unit past a multiple of the kernel's own granule, named next to the shape --
and the smallest shape the entry point accepts, with every pointer argument tagged through tests/extent.py:

    In      input                         Out    output, with its documented extent
    InOut   read and written              Ws     workspace: exactly what the size function returns

A case is (entry point, name, granule note, build).  build(L) runs on the GPU machine (it asks the library's size functions and
packs weight images with the library's own pack kernels) and returns (spec, call, options, short): the dict of tagged arguments,
call(t) -> return code from the dict of materialised tensors, the dispatch options the case runs under, and -- where the entry
point takes a size argument -- short(t), the same call with the size one unit under what the size function returns.

Pointer alignment (include/vqseg.h, "alignment"): 16 bytes where the header asks for it and the entry point checks it -- the
convolutions' tensors and images, the VQ rows, and the row kernels' activations when the channel count lets a thread move a 16-byte
vector (act_align).  These get their element's alignment and no more: per-channel fp32 vectors, scalars, counters, uint8 index /
bit tensors, the head's fp32 operands, weight gradients, the buffers of vqseg_cast_f, im2col's image, and the activations of a
one-channel-per-thread launch, the BatchNorm statistics slots, fp32 weights to be packed, and the VQ side's idx / dmin / sums /
counts / bins / EMA state (and the `means` of vqseg_kmeans_finalize_f32, which no kernel reads in vectors).
UNALIGNED lists, per entry point, pointers that must be REFUSED when they are only 8-byte aligned."""
import collections
import ctypes

import torch

from tests import dispatch_cases as dc
from tests import synth
from tests.extent import In, InOut, Out, Ws
from tests.test_nn_kernels_gpu import BF16, F32, dev, ok, ptr, stream

I16, I32, I64, U8 = torch.int16, torch.int32, torch.int64, torch.uint8
Case = collections.namedtuple("Case", "entry name granule build")
CASES = []

# every entry point the issue lists (section 3); test_extent_gpu.test_table_is_complete compares the table against this list
ENTRY_POINTS = """
vqseg_conv_pack_weights_f32 vqseg_conv_pack_weights_s3_f32 vqseg_conv_pack_weights_s2_f32 vqseg_conv_pack_all_f32
vqseg_conv2d_f vqseg_conv2d_affine_f vqseg_conv2d_affine_bits_f vqseg_conv2d_wgrad_f vqseg_conv2d_wgrad2_f
vqseg_conv2d_dgrad_s2_f vqseg_conv2d_dgrad_s2_fold_f
vqseg_bn_finalize_f vqseg_bn_apply_f vqseg_bn_apply_bits_f vqseg_bn_backward_f vqseg_bn_backward_bits_f
vqseg_maxpool3x3s2_f vqseg_maxpool3x3s2_backward_add_f vqseg_bilinear_f vqseg_s3_maxpool3x3s2_f vqseg_s3_bilinear_f
vqseg_s3_split_f vqseg_s3_merge_f vqseg_cast_f vqseg_head1x1_forward_f vqseg_head1x1_backward_f vqseg_head1x1_backward_add_f
vqseg_im2col_f vqseg_reflect_fold_f vqseg_stem7_conv_f vqseg_reflect_ring_f
vqseg_vq_prepare_f32 vqseg_vq_assign_f32 vqseg_vq_assign_bf16 vqseg_vq_assign_s3 vqseg_vq_forward_f32 vqseg_vq_forward_bf16
vqseg_vq_forward_group vqseg_vq_backward_f32 vqseg_vq_backward_bf16 vqseg_vq_code_sums vqseg_kmeans_f32
vqseg_kmeans_accumulate_f32 vqseg_kmeans_finalize_f32 vqseg_vq_ema_update_f32 vqseg_vq_revive_candidates
vqseg_vq_ema_update_revive_f32
""".split()

FAMILY = {"conv": ("vqseg_conv",), "bn": ("vqseg_bn",),
          "spatial": ("vqseg_maxpool", "vqseg_bilinear", "vqseg_s3_", "vqseg_cast", "vqseg_head1x1", "vqseg_im2col", "vqseg_reflect", "vqseg_stem7"),
          "vq": ("vqseg_vq_", "vqseg_kmeans")}


def family(entry):
    return next(f for f, prefixes in FAMILY.items() if entry.startswith(prefixes))


def add(entry, name, granule, build):
    assert entry in ENTRY_POINTS, entry
    CASES.append(Case(entry, name, granule, build))


_SEEDS = [0]


def U(shape, lo=-1.0, hi=1.0, dtype=F32):
    """deterministic values: the next seed of the table, in table order"""
    _SEEDS[0] += 1
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return synth.uniform(77000 + _SEEDS[0], shape, lo, hi).to(dtype)


def split3(v):
    """fp32 rows [.., C] -> split-3 rows [.., 2C] bf16 = [hi | lo] (include/vqseg.h, "Split-3")"""
    hi = v.bfloat16()
    return torch.cat([hi, (v - hi.float()).bfloat16()], -1)


def act_align(bf16, c):
    """the row kernels move 8 bf16 / 4 fp32 channels a thread when C allows (16-byte aligned, checked); else one channel"""
    return 16 if (c % 8 == 0 if bf16 else c % 4 == 0) else (2 if bf16 else 4)


POST = {}          # (entry, name) -> check(L, t) on the materialised tensors after each of the three calls
UNALIGNED = []     # (entry, case name, pointer): the pointer at 8 mod 16 must be refused with VQSEG_EINVAL and nothing written


def out_hw(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


# ------------------------------------------------------------------------------------------------------------------------------
# weight images for the convolution cases: packed once by the library itself, handed to the cases as plain int16 inputs
# ------------------------------------------------------------------------------------------------------------------------------
def weight(cout, cin, kh, kw):
    return U((cout, cin, kh, kw)) * (2.0 / (cin * kh * kw)) ** 0.5


def packed(L, wt, flip=0, lo=False):
    cout, cin, kh, kw = wt.shape
    n = L.vqseg_conv_packed_elems(cout, cin, kh, kw, flip)
    wd = wt.to(dev())
    hi = torch.zeros(n, dtype=I16, device=dev())
    lo_t = torch.zeros(n, dtype=I16, device=dev()) if lo else None
    ok(L.vqseg_conv_pack_weights_f32(wd.data_ptr(), cout, cin, kh, kw, flip, hi.data_ptr(), ptr(lo_t), stream()))
    torch.cuda.synchronize()
    return hi.cpu(), (lo_t.cpu() if lo else None)


def packed_s3(L, wt, c1):
    cout, cin, kh, kw = wt.shape
    wd = wt.to(dev())
    img = torch.zeros(cout * kh * kw * 3 * cin, dtype=I16, device=dev())
    ok(L.vqseg_conv_pack_weights_s3_f32(wd.data_ptr(), cout, cin, c1, kh, kw, img.data_ptr(), stream()))
    torch.cuda.synchronize()
    return img.cpu()


def packed_s2(L, wt, lo=False):
    cout, cin, k, _ = wt.shape
    n = L.vqseg_conv_packed_s2_elems(cout, cin, k)
    wd = wt.to(dev())
    hi = torch.zeros(n, dtype=I16, device=dev())
    lo_t = torch.zeros(n, dtype=I16, device=dev()) if lo else None
    ok(L.vqseg_conv_pack_weights_s2_f32(wd.data_ptr(), cout, cin, k, hi.data_ptr(), ptr(lo_t), stream()))
    torch.cuda.synchronize()
    return hi.cpu(), (lo_t.cpu() if lo else None)


# ==============================================================================================================================
# Conv: weight images
# ==============================================================================================================================
def pack_weights(cout, cin, kh, kw, flip, lo):
    def build(L):
        n = L.vqseg_conv_packed_elems(cout, cin, kh, kw, flip)
        spec = {"w": In(weight(cout, cin, kh, kw), 4), "hi": Out(n, I16), "lo": Out(n, I16) if lo else None}
        return spec, lambda t: L.vqseg_conv_pack_weights_f32(ptr(t["w"]), cout, cin, kh, kw, flip, ptr(t["hi"]), ptr(t["lo"]), stream()), {}, None
    return build


for _flip in (0, 1):
    for _lo in (False, True):
        # contracted channels padded to 32 (conv_pack.hip packed_elems): 33 = 32 + 1 in the direction the image contracts over
        add("vqseg_conv_pack_weights_f32", f"ragged-flip{_flip}-lo{int(_lo)}", "Kp = 32: cin = cout = 33, 3x3", pack_weights(33, 33, 3, 3, _flip, _lo))
        add("vqseg_conv_pack_weights_f32", f"smallest-flip{_flip}-lo{int(_lo)}", "one weight", pack_weights(1, 1, 1, 1, _flip, _lo))
add("vqseg_conv_pack_weights_f32", "stem-7x7", "7x7x3: 147 columns", pack_weights(5, 3, 7, 7, 0, True))


def pack_s3(cout, cin, c1, k):
    def build(L):
        spec = {"w": In(weight(cout, cin, k, k), 4), "out": Out(cout * k * k * 3 * cin, I16)}
        return spec, lambda t: L.vqseg_conv_pack_weights_s3_f32(ptr(t["w"]), cout, cin, c1, k, k, ptr(t["out"]), stream()), {}, None
    return build


add("vqseg_conv_pack_weights_s3_f32", "ragged", "cin, c1 % 32 (checked); cout = 5 odd, 3x3, concat 32 + 32", pack_s3(5, 64, 32, 3))
add("vqseg_conv_pack_weights_s3_f32", "smallest", "cout 1, cin 32, 1x1", pack_s3(1, 32, 32, 1))


def pack_s2(cout, cin, k, lo):
    def build(L):
        n = L.vqseg_conv_packed_s2_elems(cout, cin, k)
        spec = {"w": In(weight(cout, cin, k, k), 4), "hi": Out(n, I16), "lo": Out(n, I16) if lo else None}
        return spec, lambda t: L.vqseg_conv_pack_weights_s2_f32(ptr(t["w"]), cout, cin, k, ptr(t["hi"]), ptr(t["lo"]), stream()), {}, None
    return build


add("vqseg_conv_pack_weights_s2_f32", "ragged-k3", "Cp = 32 (cout padded): cout 33, cin 5", pack_s2(33, 5, 3, True))
add("vqseg_conv_pack_weights_s2_f32", "ragged-k1", "Cp = 32: cout 33, cin 5", pack_s2(33, 5, 1, False))
add("vqseg_conv_pack_weights_s2_f32", "smallest", "one weight", pack_s2(1, 1, 1, True))


def pack_all(cout, cin, k, c1, which):
    def build(L):
        sizes = {"fwd": L.vqseg_conv_packed_elems(cout, cin, k, k, 0), "tr": L.vqseg_conv_packed_elems(cout, cin, k, k, 1),
                 "s3": cout * k * k * 3 * cin}
        spec = {"w": In(weight(cout, cin, k, k), 4)}
        for name in ("fwd", "tr", "s3"):
            spec[name] = Out(sizes[name], I16) if name in which else None
        return spec, lambda t: L.vqseg_conv_pack_all_f32(ptr(t["w"]), cout, cin, k, c1, ptr(t["fwd"]), ptr(t["tr"]), ptr(t["s3"]), stream()), {}, None
    return build


for _which in (("fwd",), ("tr",), ("s3",), ("fwd", "tr", "s3")):
    add("vqseg_conv_pack_all_f32", "ragged-" + "+".join(_which), "Kp = 32 for tr: cout 40; cin 64 = 32 + 32 (s3 needs % 32), 3x3", pack_all(40, 64, 3, 32, _which))
    add("vqseg_conv_pack_all_f32", "smallest-" + "+".join(_which), "cout 1, cin 32, 1x1", pack_all(1, 32, 1, 32, _which))
add("vqseg_conv_pack_all_f32", "ragged-no-s3", "Kp = 32: cin = cout = 33 (no split-3 image)", pack_all(33, 33, 3, 33, ("fwd", "tr")))


# ==============================================================================================================================
# Conv: forward / data gradient.  BM = 128 rows per M tile (conv_igemm.hip), TBM = 128 / 256 (LDS-DMA), Cout tiles 32 / 64 / 128
# (launch_conv_impl): M = 129 = 3 x 43 pixels, Cout = 8 / 40 / 72 / 136 (a last chunk of 8 channels).
# ==============================================================================================================================
def stat_spec(L, m, cout):
    """[slots][2][cout] fp32; the slots behind the last row's are part of the extent and stay unwritten"""
    slots = int(L.vqseg_conv_stat_slots(m, cout))
    rps = 64 if cout >= 64 else 32
    return Out((slots, 2, cout), F32, 4, compare=(m + rps - 1) // rps * 2 * cout)


def conv2d(n, h, w, c1, c2, cout, k, stride, pad, reflect, up=1, precise=0, stat=True, opts=None, hw_out=None, operands=None):
    def build(L):
        cin = c1 + c2
        dt = F32 if precise else BF16
        if hw_out is not None:
            ho, wo = hw_out
        else:
            ho, wo = out_hw(h, w, k, stride, pad)
        m = n * ho * wo
        if operands is None:
            x, wt = U((n, h, w, cin), dtype=dt), weight(cout, cin, k, k)
        else:
            x, wt = operands()
        hi, lo = packed(L, wt, 0, bool(precise))
        spec = {"x": In(x[..., :c1].contiguous()), "x2": In(x[..., c1:].contiguous()) if c2 else None, "w_hi": In(hi),
                "w_lo": In(lo) if precise else None, "y": Out((m, cout), dt), "stat": stat_spec(L, m, cout) if stat else None}
        call = lambda t: L.vqseg_conv2d_f(ptr(t["x"]), ptr(t["x2"]), c1, ptr(t["w_hi"]), ptr(t["w_lo"]), ptr(t["y"]), ptr(t["stat"]), n, h, w, cin, cout, k, k,
                                          stride, pad, int(reflect), up, ho, wo, precise, stream())
        return spec, call, opts or {}, None
    return build


E = "vqseg_conv2d_f"
add(E, "generic-bf16-3x3-stat", "BM = 128: M = 129; Cout tile 32: 8", conv2d(1, 3, 43, 8, 0, 8, 3, 1, 1, False))
add(E, "generic-bf16-concat-reflect", "BM = 128: M = 129; Cout 40 = 32 + 8; x2 concat 8 + 16", conv2d(1, 3, 43, 8, 16, 40, 3, 1, 1, True, stat=False))
add(E, "ldsdma-1x1-lin-stat", "TBM = 128: M = 129; Cout 72 = 64 + 8; linear-pixel prologue", conv2d(1, 3, 43, 64, 0, 72, 1, 1, 0, False))
add(E, "ldsdma-3x3-concat-stat", "TBM = 128: M = 129; Cout 136 = 128 + 8; concat 64 + 64; 18 K stages", conv2d(1, 3, 43, 64, 64, 136, 3, 1, 1, False))
add(E, "ldsdma-3x3-reflect-2d-grid", "TBM = 128: M = 129; Cout 40; conv_xcd_pair = 0", conv2d(1, 3, 43, 64, 0, 40, 3, 1, 1, True, opts={"conv_xcd_pair": 0}))
add(E, "ldsdma-short-k-small", "one K stage, Cout 128: <128,128,4,2,4>; M = 129", conv2d(1, 3, 43, 64, 0, 128, 1, 1, 0, False))
add(E, "ldsdma-short-k-single", "two K stages, Cout 136: <128,128,4,1,4>; M = 129", conv2d(1, 3, 43, 128, 0, 136, 1, 1, 0, False))
add(E, "ldsdma-stride2", "stride 2: 5 x 85 -> 3 x 43, M = 129; Cout 40", conv2d(1, 5, 85, 64, 0, 40, 3, 2, 1, False))
add(E, "generic-stride2-reflect", "stride 2: 5 x 85 -> 3 x 43, M = 129; Cout 8", conv2d(1, 5, 85, 8, 0, 8, 3, 2, 1, True))
add(E, "up2-ldsdma", "up = 2: 3 x 43 -> 5 x 85, M = 425 = 3 x 128 + 41; Cout 8", conv2d(1, 3, 43, 64, 0, 8, 3, 1, 1, False, up=2, stat=False, hw_out=(5, 85)))
add(E, "up2-generic", "up = 2: 3 x 43 -> 5 x 85; Cin 8, Cout 40", conv2d(1, 3, 43, 8, 0, 40, 3, 1, 1, False, up=2, stat=False, hw_out=(5, 85)))
add(E, "generic-bf16-cout72-stat", "BM = 128: M = 129; Cin 8; Cout 72 = 64 + 8: conv_igemm_kernel<64, false, 32>", conv2d(1, 3, 43, 8, 0, 72, 3, 1, 1, False))
add(E, "generic-bf16-cout136-stat", "M = 129; Cin 8; Cout 136 = 128 + 8: conv_igemm_kernel<128, false, 32>", conv2d(1, 3, 43, 8, 0, 136, 3, 1, 1, True))
add(E, "precise-cout136-stat", "M = 129; Cin 4; Cout 136 = 128 + 8: conv_igemm_kernel<128, true, 32>", conv2d(1, 3, 43, 4, 0, 136, 3, 1, 1, False, precise=1))
add(E, "precise-3x3-stat", "BM = 128: M = 129; Cin 4 (16-byte chunk of fp32), Cout 8", conv2d(1, 3, 43, 4, 0, 8, 3, 1, 1, False, precise=1))
add(E, "precise-concat-reflect", "M = 129; concat 4 + 8, Cout 40", conv2d(1, 3, 43, 4, 8, 40, 3, 1, 1, True, precise=1, stat=False))
add(E, "precise-1x1-cout72", "M = 129; Cout 72 = 64 + 8", conv2d(1, 3, 43, 8, 0, 72, 1, 1, 0, False, precise=1))
add(E, "smallest-bf16", "one pixel, Cin 8, Cout 1", conv2d(1, 1, 1, 8, 0, 1, 1, 1, 0, False))
add(E, "smallest-precise", "one pixel, Cin 4, Cout 1", conv2d(1, 1, 1, 4, 0, 1, 1, 1, 0, False, precise=1))
add(E, "smallest-ldsdma", "one pixel, Cin 64, Cout 8", conv2d(1, 1, 1, 64, 0, 8, 1, 1, 0, False))
# the 3x3 patch kernels take whole 16 x 16 / 8 x 32 pixel tiles only (conv3x3_patch_ok): their smallest shape IS a whole tile
_PATCH = {"conv3x3_patch_min_workgroups": 1, "conv3x3_patch_tile512_min_workgroups": 1}
add(E, "patch-32ch-chunks", "tile 16 x 16 = 256 px; Cin 32 -> 32", conv2d(1, 16, 16, 32, 0, 32, 3, 1, 1, False, opts=dict(_PATCH, conv3x3_patch_tile512=0)))
add(E, "patch-32ch-ring", "tile 16 x 16; Cin 32 -> 64, tap ring", conv2d(1, 16, 16, 32, 0, 64, 3, 1, 1, False, opts=dict(_PATCH, conv3x3_patch_tile512=0, conv3x3_patch_chunk_stage=0)))
add(E, "patch-64ch-concat", "tile 16 x 16, two tiles; 64 + 64 -> 128", conv2d(2, 16, 16, 64, 64, 128, 3, 1, 1, False, opts=_PATCH))
add(E, "patch-wide-256", "tile 8 x 32; 64 -> 256, 256-channel tile", conv2d(1, 8, 32, 64, 0, 256, 3, 1, 1, False, opts=_PATCH))
add(E, "patch-tile512", "tile 16 x 32 = 512 px; 32 -> 32", conv2d(1, 16, 32, 32, 0, 32, 3, 1, 1, False, opts=_PATCH))
add(E, "patch-tile512-64", "tile 32 x 16 = 512 px; 64 -> 64", conv2d(1, 32, 16, 64, 0, 64, 3, 1, 1, False, opts=_PATCH))
for _c in sorted(dc.CASES):                                  # the variants only large shapes reach, as dispatch_cases.py has them
    _n, _h, _w, _cin, _cout, _k, _s, _pad, _r = dc.CASES[_c]
    add(E, f"ldsdma-large-{_c}", "tests/dispatch_cases.py " + _c, conv2d(_n, _h, _w, _cin, 0, _cout, _k, _s, _pad, _r, operands=(lambda c=_c: dc.operands(c))))


def conv2d_affine(n, h, w, c1, c2, cout, k, stride, pad, reflect, precise, res, relu, opts=None):
    def build(L):
        cin = c1 + c2
        ho, wo = out_hw(h, w, k, stride, pad)
        m = n * ho * wo
        wt = weight(cout, cin, k, k)
        if precise == 2:
            x = U((n, h, w, cin))
            xa, xb = split3(x[..., :c1]), (split3(x[..., c1:]) if c2 else None)
            hi, lo = packed_s3(L, wt, c1), None
            y, r = Out((m, 2 * cout), BF16), (In(split3(U((m, cout)))) if res else None)
        else:
            dt = F32 if precise else BF16
            x = U((n, h, w, cin), dtype=dt)
            xa, xb = x[..., :c1].contiguous(), (x[..., c1:].contiguous() if c2 else None)
            hi, lo = packed(L, wt, 0, bool(precise))
            y, r = Out((m, cout), dt), (In(U((m, cout), dtype=dt)) if res else None)
        spec = {"x": In(xa), "x2": In(xb) if c2 else None, "w_hi": In(hi), "w_lo": In(lo) if precise == 1 else None,
                "scale": In(U(cout, 0.5, 1.5), 4), "shift": In(U(cout, -0.5, 0.5), 4), "res": r, "y": y}
        call = lambda t: L.vqseg_conv2d_affine_f(ptr(t["x"]), ptr(t["x2"]), c1, ptr(t["w_hi"]), ptr(t["w_lo"]), ptr(t["scale"]), ptr(t["shift"]), ptr(t["res"]), relu,
                                                 ptr(t["y"]), n, h, w, cin, cout, k, k, stride, pad, int(reflect), ho, wo, precise, stream())
        return spec, call, opts or {}, None
    return build


E = "vqseg_conv2d_affine_f"
add(E, "bf16-generic-res-relu", "BM = 128: M = 129; Cout 40", conv2d_affine(1, 3, 43, 8, 0, 40, 3, 1, 1, False, 0, True, 1))
add(E, "bf16-generic-cout72-res", "M = 129; Cin 8; Cout 72: conv_igemm_kernel<64, false, 32>", conv2d_affine(1, 3, 43, 8, 0, 72, 3, 1, 1, True, 0, True, 1))
add(E, "bf16-generic-cout136-res", "M = 129; Cin 8; Cout 136: conv_igemm_kernel<128, false, 32>", conv2d_affine(1, 3, 43, 8, 0, 136, 3, 1, 1, False, 0, True, 0))
add(E, "precise-cout136-res", "M = 129; Cin 4; Cout 136: conv_igemm_kernel<128, true, 32>", conv2d_affine(1, 3, 43, 4, 0, 136, 1, 1, 0, False, 1, True, 1))
add(E, "bf16-ldsdma-nores", "TBM = 128: M = 129; Cout 72", conv2d_affine(1, 3, 43, 64, 0, 72, 1, 1, 0, False, 0, False, 0))
add(E, "bf16-ldsdma-res-relu-concat", "M = 129; Cout 136; concat 64 + 64; reflect", conv2d_affine(1, 3, 43, 64, 64, 136, 3, 1, 1, True, 0, True, 1))
add(E, "bf16-patch-res", "tile 16 x 16; 64 -> 64", conv2d_affine(1, 16, 16, 64, 0, 64, 3, 1, 1, False, 0, True, 1, opts=_PATCH))
add(E, "precise-res-relu", "M = 129; Cin 4, Cout 40", conv2d_affine(1, 3, 43, 4, 0, 40, 3, 1, 1, False, 1, True, 1))
add(E, "precise-nores", "M = 129; Cin 8, Cout 8, stride 2", conv2d_affine(1, 5, 85, 8, 0, 8, 3, 2, 1, True, 1, False, 0))
add(E, "split3-generic-res", "M = 129; logical Cin 32 (96 contracted: not % 64), Cout 8", conv2d_affine(1, 3, 43, 32, 0, 8, 3, 1, 1, False, 2, True, 1))
add(E, "split3-generic-concat", "M = 129; logical 32 + 32 (96 + 96 contracted: the parts are no whole 64-channel stages), Cout 72", conv2d_affine(1, 3, 43, 32, 32, 72, 1, 1, 0, False, 2, False, 1))
add(E, "split3-ldsdma-concat", "M = 129; logical 64 + 64 (192 + 192 contracted), Cout 72", conv2d_affine(1, 3, 43, 64, 64, 72, 1, 1, 0, False, 2, True, 1))
add(E, "split3-patch", "tile 16 x 16; logical 64 -> 64", conv2d_affine(1, 16, 16, 64, 0, 64, 3, 1, 1, False, 2, True, 1, opts=_PATCH))
add(E, "smallest-bf16", "one pixel, Cin 8, Cout 1", conv2d_affine(1, 1, 1, 8, 0, 1, 1, 1, 0, False, 0, True, 1))
add(E, "smallest-precise", "one pixel, Cin 4, Cout 1", conv2d_affine(1, 1, 1, 4, 0, 1, 1, 1, 0, False, 1, False, 0))
add(E, "smallest-split3", "one pixel, logical Cin 32, Cout 8", conv2d_affine(1, 1, 1, 32, 0, 8, 1, 1, 0, False, 2, True, 0))


def conv2d_bits(n, h, w, cin, cout, k, pad, opts=None):
    def build(L):
        ho, wo = out_hw(h, w, k, 1, pad)
        m = n * ho * wo
        hi, _ = packed(L, weight(cout, cin, k, k))
        bits = (U(m * cout // 8, 0, 256)).to(U8)
        spec = {"x": In(U((n, h, w, cin), dtype=BF16)), "w_hi": In(hi), "scale": In(U(cout, 0.5, 1.5), 4), "shift": In(U(cout, -0.5, 0.5), 4),
                "res": In(U((m, cout), dtype=BF16)), "bits": In(bits, 1), "y": Out((m, cout), BF16)}
        call = lambda t: L.vqseg_conv2d_affine_bits_f(ptr(t["x"]), ptr(t["w_hi"]), ptr(t["scale"]), ptr(t["shift"]), ptr(t["res"]), ptr(t["bits"]), ptr(t["y"]),
                                                      n, h, w, cin, cout, k, k, pad, ho, wo, stream())
        return spec, call, opts or {}, None
    return build


E = "vqseg_conv2d_affine_bits_f"
add(E, "generic", "BM = 128: M = 129; Cout 40 = 32 + 8 (bits: 8 channels a byte)", conv2d_bits(1, 3, 43, 8, 40, 3, 1))
add(E, "ldsdma", "TBM = 128: M = 129; Cout 72", conv2d_bits(1, 3, 43, 64, 72, 1, 0))
add(E, "generic-cout72", "M = 129; Cin 8; Cout 72: conv_igemm_kernel<64, false, 32>", conv2d_bits(1, 3, 43, 8, 72, 3, 1))
add(E, "generic-cout136", "M = 129; Cin 8; Cout 136: conv_igemm_kernel<128, false, 32>", conv2d_bits(1, 3, 43, 8, 136, 3, 1))
add(E, "ldsdma-136", "M = 129; Cout 136, 3x3", conv2d_bits(1, 3, 43, 64, 136, 3, 1))
add(E, "patch", "tile 16 x 16; 64 -> 128", conv2d_bits(1, 16, 16, 64, 128, 3, 1, opts=_PATCH))
add(E, "smallest", "one pixel, Cin 8, Cout 8 (one byte of bits)", conv2d_bits(1, 1, 1, 8, 8, 1, 0))


# ==============================================================================================================================
# Conv: weight gradient.  Per-tap kernel: 256 pixels a slab, tiles of 32 x 32 channels; nine-tap LDS-DMA kernel: Wo % 16, Ho % 4,
# channels % 32; 1x1 LDS-DMA kernel: 64-pixel stages, channels % 64.
# ==============================================================================================================================
def wgrad(n, n_b, h, w, c1, c2, cout, k, stride, pad, reflect, precise, accumulate, im2col=0, cin_out=None, opts=None, two=False):
    def build(L):
        cin = c1 + c2
        dt = F32 if precise else BF16
        ho, wo = (h, w) if im2col else out_hw(h, w, k, stride, pad)
        wk = 1 if im2col else k
        nbytes = L.vqseg_conv2d_wgrad_workspace_bytes(n + n_b, h, w, cin, ho, wo, cout, wk, wk)
        co = cin if cin_out is None else cin_out
        gw0 = U((cout, co, k, k))
        spec = {"ws": Ws(nbytes), "gw": InOut(gw0, 4) if accumulate else Out((cout, co, k, k), F32, 4)}
        for tag, nn in (("", n), ("_b", n_b)):
            x = U((max(nn, 1), h, w, cin), dtype=dt)
            spec["gy" + tag] = In(U((nn, ho, wo, cout), dtype=dt)) if nn else None
            spec["x" + tag] = In(x[..., :c1].contiguous()) if nn else None
            spec["x2" + tag] = In(x[..., c1:].contiguous()) if nn and c2 else None

        def call(t, short=0):
            tail = (c1, h, w, cin, ho, wo, cout, k, k, 1 if im2col else stride, 0 if im2col else pad, int(reflect), precise, co, im2col, accumulate,
                    ptr(t["ws"]), nbytes - short, ptr(t["gw"]), stream())
            if two:
                return L.vqseg_conv2d_wgrad2_f(ptr(t["gy"]), ptr(t["x"]), ptr(t["x2"]), n, ptr(t["gy_b"]), ptr(t["x_b"]), ptr(t["x2_b"]), n_b, *tail)
            return L.vqseg_conv2d_wgrad_f(ptr(t["gy"]), ptr(t["x"]), ptr(t["x2"]), c1, n, *tail[1:])
        return spec, call, opts or {}, lambda t: call(t, 1)
    return build


for E, _two, _nb in (("vqseg_conv2d_wgrad_f", False, 0), ("vqseg_conv2d_wgrad2_f", True, 1), ("vqseg_conv2d_wgrad2_f", True, 0)):
    _t = f"-nb{_nb}" if _two else ""
    add(E, "pertap-bf16" + _t, "256 px a slab: M = 129 an image; Cin 8, Cout 40 = 32 + 8", wgrad(1, _nb, 3, 43, 8, 0, 40, 3, 1, 1, False, 0, 0, two=_two))
    add(E, "pertap-bf16-acc-concat" + _t, "M = 129; concat 8 + 16; reflect; accumulate", wgrad(1, _nb, 3, 43, 8, 16, 8, 3, 1, 1, True, 0, 1, two=_two))
    add(E, "pertap-precise-acc" + _t, "M = 129; Cin 4, Cout 4; accumulate", wgrad(1, _nb, 3, 43, 4, 0, 4, 3, 1, 1, False, 1, 1, two=_two))
    add(E, "pertap-precise-stride2" + _t, "5 x 85 -> 3 x 43; Cin 12 = 4 + 8, Cout 8", wgrad(1, _nb, 5, 85, 4, 8, 8, 3, 2, 1, True, 1, 0, two=_two))
    add(E, "ninetap" + _t, "block 4 x 16 px: 4 x 16 image; 32 -> 32", wgrad(1, _nb, 4, 16, 32, 0, 32, 3, 1, 1, False, 0, 0, two=_two))
    add(E, "ninetap-concat-acc" + _t, "8 x 16 image; 32 + 32 -> 64; accumulate", wgrad(1, _nb, 8, 16, 32, 32, 64, 3, 1, 1, False, 0, 1, two=_two))
    add(E, "ninetap-stride2" + _t, "8 x 32 -> 4 x 16; 64 -> 128", wgrad(1, _nb, 8, 32, 64, 0, 128, 3, 2, 1, False, 0, 0, two=_two))
    add(E, "1x1-ldsdma" + _t, "64-px stages: M = 129; 64 -> 64", wgrad(1, _nb, 3, 43, 64, 0, 64, 1, 1, 0, False, 0, 0, two=_two))
    add(E, "1x1-ldsdma-stride2-acc" + _t, "5 x 85 -> 3 x 43; 128 -> 64; accumulate", wgrad(1, _nb, 5, 85, 128, 0, 64, 1, 2, 0, False, 0, 1, two=_two))
    add(E, "im2col-ldsdma" + _t, "patch matrix [129][160] of a 7x7x3 stem -> gw [64][3][7][7]", wgrad(1, _nb, 3, 43, 160, 0, 64, 7, 1, 0, False, 0, 0, 1, 3, two=_two))
    add(E, "im2col-pertap-acc" + _t, "the same on the per-tap kernel (conv_wgrad1x1_narrow = 0); accumulate",
        wgrad(1, _nb, 3, 43, 160, 0, 64, 7, 1, 0, False, 0, 1, 1, 3, opts={"conv_wgrad1x1_narrow": 0}, two=_two))
    add(E, "smallest-bf16" + _t, "one pixel, 8 -> 8, 1x1", wgrad(1, _nb, 1, 1, 8, 0, 8, 1, 1, 0, False, 0, 0, two=_two))
    add(E, "smallest-precise" + _t, "one pixel, 4 -> 4, 1x1", wgrad(1, _nb, 1, 1, 4, 0, 4, 1, 1, 0, False, 1, 0, two=_two))


# ==============================================================================================================================
# Conv: stride-2 data gradients
# ==============================================================================================================================
def dgrad_s2(n, ho, wo, cout, cin, k, oh, ow, precise, accumulate):
    def build(L):
        dt = F32 if precise else BF16
        hi, lo = packed_s2(L, weight(cout, cin, k, k), bool(precise))
        spec = {"gy": In(U((n, ho, wo, cout), dtype=dt)), "w_hi": In(hi), "w_lo": In(lo) if precise else None,
                "gx": InOut(U((n, oh, ow, cin), dtype=dt)) if accumulate else Out((n, oh, ow, cin), dt)}
        call = lambda t: L.vqseg_conv2d_dgrad_s2_f(ptr(t["gy"]), ptr(t["w_hi"]), ptr(t["w_lo"]), ptr(t["gx"]), n, ho, wo, cout, cin, k, oh, ow, precise,
                                                   accumulate, stream())
        return spec, call, {}, None
    return build


E = "vqseg_conv2d_dgrad_s2_f"
add(E, "k1-accumulate", "3 x 43 -> 5 x 86 (odd and even extent): 129 px a class; 64 -> 72", dgrad_s2(1, 3, 43, 64, 72, 1, 5, 86, 0, 1))
add(E, "k1-accumulate-generic", "3 x 43 -> 6 x 85; 8 -> 40", dgrad_s2(1, 3, 43, 8, 40, 1, 6, 85, 0, 1))
add(E, "k3-generic-cin72", "gy of 8 channels (generic kernel) -> gx of 72 = 64 + 8: conv_igemm_kernel<64, false, 32>; padded 7 x 87", dgrad_s2(1, 3, 43, 8, 72, 3, 7, 87, 0, 0))
add(E, "k1-accumulate-generic-cin136", "gy of 8 channels -> gx of 136: conv_igemm_kernel<128, false, 32>; 5 x 85; accumulate", dgrad_s2(1, 3, 43, 8, 136, 1, 5, 85, 0, 1))
add(E, "k1-overwrite", "3 x 43 -> 5 x 85; 64 -> 8 (memset + one class)", dgrad_s2(1, 3, 43, 64, 8, 1, 5, 85, 0, 0))
add(E, "k3-bf16", "3 x 43 -> padded 8 x 88: classes of 4 x 44, 4 x 44, 4 x 44, 4 x 44 px; 64 -> 72", dgrad_s2(1, 3, 43, 64, 72, 3, 8, 88, 0, 0))
add(E, "k3-bf16-odd", "3 x 43 -> padded 7 x 87: classes 4 x 44 .. 3 x 43; 8 -> 8", dgrad_s2(1, 3, 43, 8, 8, 3, 7, 87, 0, 0))
add(E, "k3-precise", "3 x 43 -> padded 7 x 88; 4 -> 40", dgrad_s2(1, 3, 43, 4, 40, 3, 7, 88, 1, 0))
add(E, "k1-precise", "3 x 43 -> 5 x 85; 4 -> 4", dgrad_s2(1, 3, 43, 4, 4, 1, 5, 85, 1, 0))
add(E, "smallest-k1", "one pixel -> one pixel, 8 -> 8", dgrad_s2(1, 1, 1, 8, 8, 1, 1, 1, 0, 1))
add(E, "smallest-k3", "one pixel -> padded 3 x 3, 8 -> 8", dgrad_s2(1, 1, 1, 8, 8, 3, 3, 3, 0, 0))


def dgrad_s2_fold(n, ho, wo, cout, cin, reflect, opts=None):
    def build(L):
        h, w = 2 * ho, 2 * wo
        rows = int(L.vqseg_conv2d_dgrad_s2_fold_rows(n, h, w, int(reflect)))
        assert rows == n * h * w + (n * (w + 1 + h) if reflect else 0) + 1        # pixel rows + ring + dump row (include/vqseg.h)
        hi, _ = packed_s2(L, weight(cout, cin, 3, 3))
        # the ring and the dump row are scratch inside the promised extent: the result is the n * h * w pixel rows
        spec = {"gy": In(U((n, ho, wo, cout), dtype=BF16)), "w_hi": In(hi), "gx": Out((rows, cin), BF16, compare=n * h * w * cin)}
        call = lambda t: L.vqseg_conv2d_dgrad_s2_fold_f(ptr(t["gy"]), ptr(t["w_hi"]), ptr(t["gx"]), n, ho, wo, cout, cin, h, w, int(reflect), stream())
        return spec, call, opts or {}, None
    return build


E = "vqseg_conv2d_dgrad_s2_fold_f"
for _r in (True, False):
    _t = "reflect" if _r else "zero"
    add(E, f"ragged-{_t}-bn64", "128-px tiles per parity class: 3 x 43 -> 6 x 86 (classes of 4 x 44 = 176 px); Cin 72 = 64 + 8", dgrad_s2_fold(1, 3, 43, 64, 72, _r))
    add(E, f"ragged-{_t}-bn128", "6 x 86, two images; Cout 128, Cin 136 = 128 + 8", dgrad_s2_fold(2, 3, 43, 128, 136, _r))
    add(E, f"ragged-{_t}-double-buffer", "6 x 86; Cout 192 (12 K stages > conv_short_k_single_buffer), Cin 128", dgrad_s2_fold(1, 3, 43, 192, 128, _r))
    add(E, f"smallest-{_t}", "H = W = 4 (the smallest the entry point takes), 64 -> 64", dgrad_s2_fold(1, 2, 2, 64, 64, _r))


# ==============================================================================================================================
# BatchNorm.  Statistics slots of 32 / 64 rows, more than 128 slots: two-level merge in groups of >= 16; channel groups of 64;
# backward: 256 rows a block (BNB_ROWS_MIN); apply: 16-byte vectors (8 bf16 / 4 fp32) when C allows, a fast path when 256 V % C == 0.
# ==============================================================================================================================
def bn_finalize(m, c, training, use_sync):
    def build(L):
        slots = int(L.vqseg_conv_stat_slots(m, c))
        part = torch.stack([U((slots, c), -3, 3), U((slots, c), 0.5, 40)], 1)
        stats = InOut if training else In
        spec = {"partial": InOut(part, 4) if training else None, "gamma": In(U(c, 0.5, 1.5), 4), "beta": In(U(c, -0.5, 0.5), 4),
                "run_mean": stats(U(c, -1, 1), 4), "run_var": stats(U(c, 0.5, 1.5), 4), "nbt": InOut(torch.full((1,), 5, dtype=I64), 8) if training else None,
                "sync": InOut(torch.zeros(L.vqseg_bn_sync_ints(c), dtype=I32), 4) if use_sync else None}
        for name in ("scale", "shift", "save_mean", "save_invstd"):
            spec[name] = Out(c, F32, 4)
        call = lambda t: L.vqseg_bn_finalize_f(ptr(t["partial"]), m, c, ptr(t["gamma"]), ptr(t["beta"]), ptr(t["run_mean"]), ptr(t["run_var"]), 0.1, 1e-5, training,
                                               ptr(t["scale"]), ptr(t["shift"]), ptr(t["save_mean"]), ptr(t["save_invstd"]), ptr(t["nbt"]), ptr(t["sync"]), stream())
        return spec, call, {}, None
    return build


E = "vqseg_bn_finalize_f"
for _sync in (False, True):
    _t = "-sync" if _sync else ""
    add(E, "one-level" + _t, "32-row slots: M = 700 -> 22 slots, the last 28 rows; C = 5", bn_finalize(700, 5, 1, _sync))
    add(E, "two-level" + _t, "64-row slots: 200 slots in groups of 16, the last group 8; C = 72 = 64 + 8", bn_finalize(200 * 64 - 3, 72, 1, _sync))
    add(E, "two-level-129" + _t, "129 slots: the last group a single short slot; C = 65", bn_finalize(129 * 64 - 10, 65, 1, _sync))
    add(E, "smallest" + _t, "M = 1, C = 1", bn_finalize(1, 1, 1, _sync))
    add(E, "eval" + _t, "256 channels a workgroup: C = 257", bn_finalize(700, 257, 0, _sync))
    add(E, "eval-smallest" + _t, "C = 1", bn_finalize(1, 1, 0, _sync))


def bn_apply(bf16, m, c, res, relu):
    def build(L):
        dt = BF16 if bf16 else F32
        al = act_align(bf16, c)
        spec = {"y": In(U((m, c), dtype=dt), al), "res": In(U((m, c), dtype=dt), al) if res else None, "scale": In(U(c, 0.5, 1.5), 4),
                "shift": In(U(c, -0.5, 0.5), 4), "out": Out((m, c), dt, al)}
        return spec, lambda t: L.vqseg_bn_apply_f(bf16, ptr(t["y"]), ptr(t["res"]), ptr(t["scale"]), ptr(t["shift"]), m, c, relu, ptr(t["out"]), stream()), {}, None
    return build


E = "vqseg_bn_apply_f"
for _bf, _cs in ((1, (8, 24, 12)), (0, (4, 12, 5))):
    for _c, _note in zip(_cs, ("16-byte vectors, 256 V % C == 0", "16-byte vectors, 256 V % C != 0", "one channel a thread")):
        _m = 257 if _c <= 8 else 129
        add(E, f"{'bf16' if _bf else 'f32'}-C{_c}", f"{_note}; M = {_m}: more threads than one workgroup of 256", bn_apply(_bf, _m, _c, _c != 12, 1))
    add(E, f"{'bf16' if _bf else 'f32'}-smallest", "M = 1, C = 1", bn_apply(_bf, 1, 1, True, 0))


def bn_apply_bits(m, c, res):
    def build(L):
        spec = {"y": In(U((m, c), dtype=BF16)), "res": In(U((m, c), dtype=BF16)) if res else None, "scale": In(U(c, 0.5, 1.5), 4),
                "shift": In(U(c, -0.5, 0.5), 4), "out": Out((m, c), BF16), "bits": Out(m * c // 8, U8, 1)}
        return spec, lambda t: L.vqseg_bn_apply_bits_f(ptr(t["y"]), ptr(t["res"]), ptr(t["scale"]), ptr(t["shift"]), m, c, ptr(t["out"]), ptr(t["bits"]), stream()), {}, None
    return build


E = "vqseg_bn_apply_bits_f"
add(E, "C8", "8 channels a thread and a byte of bits; M = 257: one workgroup + 1", bn_apply_bits(257, 8, True))
add(E, "C24", "256 V % C != 0; M = 129", bn_apply_bits(129, 24, True))
add(E, "C72-nores", "M = 129", bn_apply_bits(129, 72, False))
add(E, "smallest", "M = 1, C = 8", bn_apply_bits(1, 8, True))


def bn_backward(bf16, m, c, relu, with_out, with_res, training, accumulate, use_sync, opts=None, bits=False):
    def build(L):
        dt = BF16 if bf16 else F32
        nf = int(L.vqseg_bn_backward_workspace_floats(m, c))
        assert nf == (m + 255) // 256 * 2 * c + 3 * c
        al = act_align(bf16, c)
        spec = {"g_out": In(U((m, c), dtype=dt), al), "y": In(U((m, c), dtype=dt), al), "mean": In(U(c, -0.2, 0.2), 4), "invstd": In(U(c, 0.5, 2), 4),
                "gamma": In(U(c, 0.5, 1.5), 4), "ws": Ws(4 * nf), "g_y": Out((m, c), dt, al), "g_res": Out((m, c), dt, al) if with_res else None,
                "sync": InOut(torch.zeros(L.vqseg_bn_sync_ints(c), dtype=I32), 4) if use_sync else None}
        for name in ("dgamma", "dbeta"):
            spec[name] = InOut(U(c), 4) if accumulate else Out(c, F32, 4)
        if bits:
            spec["bits"] = In(U(m * c // 8, 0, 256).to(U8), 1)
            call = lambda t: L.vqseg_bn_backward_bits_f(ptr(t["g_out"]), ptr(t["bits"]), ptr(t["y"]), ptr(t["mean"]), ptr(t["invstd"]), ptr(t["gamma"]), m, c, training,
                                                        accumulate, ptr(t["ws"]), ptr(t["dgamma"]), ptr(t["dbeta"]), ptr(t["g_y"]), ptr(t["g_res"]), ptr(t["sync"]), stream())
            return spec, call, opts or {}, None
        spec["out"] = In(U((m, c), -0.5, 1, dtype=dt).clamp_min(0), al) if with_out else None
        spec["fwd_scale"] = In(U(c, 0.5, 1.5), 4) if not with_out else None
        spec["fwd_shift"] = In(U(c, -0.5, 0.5), 4) if not with_out else None
        call = lambda t: L.vqseg_bn_backward_f(bf16, ptr(t["g_out"]), ptr(t["out"]), ptr(t["y"]), ptr(t["mean"]), ptr(t["invstd"]), ptr(t["gamma"]), ptr(t["fwd_scale"]),
                                               ptr(t["fwd_shift"]), m, c, relu, training, accumulate, ptr(t["ws"]), ptr(t["dgamma"]), ptr(t["dbeta"]), ptr(t["g_y"]),
                                               ptr(t["g_res"]), ptr(t["sync"]), stream())
        return spec, call, opts or {}, None
    return build


E = "vqseg_bn_backward_f"
_G = "256 rows a block: M = 257; "
for _sync in (False, True):
    _t = "-sync" if _sync else ""
    add(E, "bf16-out-res" + _t, _G + "C = 72 = 64 + 8; residual layer, pre-masked", bn_backward(1, 257, 72, 1, True, True, 1, 0, _sync))
    add(E, "bf16-out-res-two-pass" + _t, _G + "C = 72; bn_bwd_premask = 0", bn_backward(1, 257, 72, 1, True, True, 1, 0, _sync, opts={"bn_bwd_premask": 0}))
    add(E, "bf16-noout-acc" + _t, _G + "C = 24: mask from the forward's expression; accumulate", bn_backward(1, 257, 24, 1, False, False, 1, 1, _sync))
    add(E, "bf16-C12-out" + _t, _G + "C = 12: one channel a thread", bn_backward(1, 257, 12, 1, True, False, 1, 0, _sync))
    add(E, "f32-norelu-acc" + _t, _G + "C = 5: one channel a thread; no ReLU; accumulate", bn_backward(0, 257, 5, 0, False, False, 1, 1, _sync))
    add(E, "f32-out-res-eval" + _t, _G + "C = 68 = 64 + 4; eval statistics", bn_backward(0, 257, 68, 1, True, True, 0, 0, _sync))
    add(E, "smallest-bf16" + _t, "M = 1, C = 1", bn_backward(1, 1, 1, 1, True, True, 1, 0, _sync))
    add(E, "smallest-f32" + _t, "M = 1, C = 1", bn_backward(0, 1, 1, 0, False, False, 1, 1, _sync))
add(E, "tall-sync", "sync: rows a block doubles until <= 512 blocks: M = 512 * 256 + 1 -> 512 rows a block; C = 8", bn_backward(1, 512 * 256 + 1, 8, 1, True, False, 1, 0, True))

E = "vqseg_bn_backward_bits_f"
for _sync in (False, True):
    _t = "-sync" if _sync else ""
    add(E, "res" + _t, _G + "C = 72", bn_backward(1, 257, 72, 1, False, True, 1, 0, _sync, bits=True))
    add(E, "nores-acc" + _t, _G + "C = 24; g_res NULL (the consumer applies the bits); accumulate", bn_backward(1, 257, 24, 1, False, False, 1, 1, _sync, bits=True))
    add(E, "smallest" + _t, "M = 1, C = 8", bn_backward(1, 1, 8, 1, False, True, 1, 0, _sync, bits=True))


# ==============================================================================================================================
# Spatial / head / stem.  dispatch_rows (nn_spatial.hip): VC = 8 bf16 / 4 fp32 channels a thread when C allows, else one
# (C = 12 bf16, C = 5 fp32); 256 threads a workgroup.
# ==============================================================================================================================
ROWVEC = [(1, 8, "VC = 8"), (1, 12, "VC = 1 (bf16, C = 12)"), (0, 4, "VC = 4"), (0, 5, "VC = 1 (fp32, C = 5)")]


def pool_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def maxpool(bf16, mode, n, h, w, c):
    """mode: fwd, fwd-idx, bwd-x (arg-max recomputed from x), bwd-idx"""
    def build(L):
        dt = BF16 if bf16 else F32
        al = act_align(bf16, c)
        ho, wo = pool_hw(h, w)
        pos = In(U((n, ho, wo, c), 0, 9).to(U8), 1)
        if mode.startswith("fwd"):
            spec = {"x": In(U((n, h, w, c), dtype=dt), al), "g": None, "out": Out((n, ho, wo, c), dt, al), "idx": Out((n, ho, wo, c), U8, 1) if mode == "fwd-idx" else None}
            back = 0
        else:
            spec = {"x": In(U((n, h, w, c), dtype=dt), al) if mode == "bwd-x" else None, "g": In(U((n, ho, wo, c), dtype=dt), al), "out": Out((n, h, w, c), dt, al),
                    "idx": pos if mode == "bwd-idx" else None}
            back = 1
        return spec, lambda t: L.vqseg_maxpool3x3s2_f(bf16, back, ptr(t["x"]), ptr(t["g"]), n, h, w, c, ptr(t["out"]), ptr(t["idx"]), stream()), {}, None
    return build


E = "vqseg_maxpool3x3s2_f"
for _mode in ("fwd", "fwd-idx", "bwd-x", "bwd-idx"):
    for _bf, _c, _note in ROWVEC:
        add(E, f"{_mode}-{'bf16' if _bf else 'f32'}-C{_c}", _note + "; 9 x 35 -> 5 x 18 (odd extents), three images: more than one workgroup",
            maxpool(_bf, _mode, 3, 9, 35, _c))
    add(E, f"{_mode}-smallest", "one pixel, C = 1", maxpool(1, _mode, 1, 1, 1, 1))


def maxpool_add(bf16, n, h, w, c, with_add):
    def build(L):
        dt = BF16 if bf16 else F32
        ho, wo = pool_hw(h, w)
        al = act_align(bf16, c)
        spec = {"g": In(U((n, ho, wo, c), dtype=dt), al), "idx": In(U((n, ho, wo, c), 0, 9).to(U8), 1), "gx_add": In(U((n, h, w, c), dtype=dt), al) if with_add else None,
                "gx": Out((n, h, w, c), dt, al)}
        return spec, lambda t: L.vqseg_maxpool3x3s2_backward_add_f(bf16, ptr(t["g"]), ptr(t["idx"]), ptr(t["gx_add"]), n, h, w, c, ptr(t["gx"]), stream()), {}, None
    return build


E = "vqseg_maxpool3x3s2_backward_add_f"
for _bf, _c, _note in ROWVEC:
    add(E, f"{'bf16' if _bf else 'f32'}-C{_c}", _note + "; 9 x 35, three images", maxpool_add(_bf, 3, 9, 35, _c, True))
add(E, "noadd-bf16-C8", "gx_add NULL; 8 x 34 (even extents)", maxpool_add(1, 2, 8, 34, 8, False))
add(E, "smallest", "one pixel, C = 1", maxpool_add(0, 1, 1, 1, 1, True))


def bilinear(bf16, backward, n, h, w, c, ho, wo, align, opts=None, s3=False):
    def build(L):
        dt = BF16 if bf16 else F32
        if s3:
            spec = {"src": In(split3(U((n, h, w, c)))), "dst": Out((n, ho, wo, 2 * c), BF16)}
            return spec, lambda t: L.vqseg_s3_bilinear_f(ptr(t["src"]), n, h, w, c, ho, wo, align, ptr(t["dst"]), stream()), opts or {}, None
        al = act_align(bf16, c)
        spec = {"src": In(U((n, ho, wo, c) if backward else (n, h, w, c), dtype=dt), al), "dst": Out((n, h, w, c) if backward else (n, ho, wo, c), dt, al)}
        return spec, lambda t: L.vqseg_bilinear_f(bf16, backward, ptr(t["src"]), n, h, w, c, ho, wo, align, ptr(t["dst"]), stream()), opts or {}, None
    return build


E = "vqseg_bilinear_f"
for _back in (0, 1):
    _d = "bwd" if _back else "fwd"
    for _al in (0, 1):
        for _bf, _c, _note in ROWVEC:
            add(E, f"{_d}-generic-align{_al}-{'bf16' if _bf else 'f32'}-C{_c}", _note + "; 5 x 7 -> 11 x 13, three images", bilinear(_bf, _back, 3, 5, 7, _c, 11, 13, _al))
        add(E, f"{_d}-logits-align{_al}", "C == 3 fp32 (RowVec<float, 3>); 5 x 7 -> 19 x 23", bilinear(0, _back, 2, 5, 7, 3, 19, 23, _al))
        add(E, f"{_d}-down-align{_al}", "11 x 13 -> 5 x 7; bf16 C = 8", bilinear(1, _back, 3, 11, 13, 8, 5, 7, _al))
    for _up in (1, 2, 0):
        add(E, f"{_d}-up2-opt{_up}-bf16", f"exact 2x, powers of two: 4 x 8 -> 8 x 16, C = 16; bilinear_up2 = {_up}", bilinear(1, _back, 3, 4, 8, 16, 8, 16, 0, {"bilinear_up2": _up}))
        add(E, f"{_d}-up2-opt{_up}-f32", f"exact 2x: 8 x 4 -> 16 x 8, C = 4; bilinear_up2 = {_up}", bilinear(0, _back, 3, 8, 4, 4, 16, 8, 0, {"bilinear_up2": _up}))
    add(E, f"{_d}-up2-short", "exact 2x with H = 2 < 4: the one-row backward", bilinear(1, _back, 1, 2, 2, 8, 4, 4, 0))
    add(E, f"{_d}-smallest", "one pixel -> one pixel, C = 1", bilinear(0, _back, 1, 1, 1, 1, 1, 1, 0))

E = "vqseg_s3_bilinear_f"
for _al in (0, 1):
    add(E, f"generic-align{_al}", "VC = 8 (C % 8 checked); 5 x 7 -> 11 x 13, C = 24, three images", bilinear(1, 0, 3, 5, 7, 24, 11, 13, _al, s3=True))
add(E, "up2", "exact 2x: 4 x 8 -> 8 x 16, C = 16", bilinear(1, 0, 3, 4, 8, 16, 8, 16, 0, s3=True))
add(E, "up2-off", "the same with bilinear_up2 = 0", bilinear(1, 0, 3, 4, 8, 16, 8, 16, 0, {"bilinear_up2": 0}, s3=True))
add(E, "smallest", "one pixel, C = 8", bilinear(1, 0, 1, 1, 1, 8, 1, 1, 0, s3=True))


def s3_maxpool(n, h, w, c):
    def build(L):
        ho, wo = pool_hw(h, w)
        spec = {"x": In(split3(U((n, h, w, c)))), "y": Out((n, ho, wo, 2 * c), BF16)}
        return spec, lambda t: L.vqseg_s3_maxpool3x3s2_f(ptr(t["x"]), n, h, w, c, ptr(t["y"]), stream()), {}, None
    return build


add("vqseg_s3_maxpool3x3s2_f", "ragged", "VC = 8; 9 x 35 -> 5 x 18, C = 24, three images", s3_maxpool(3, 9, 35, 24))
add("vqseg_s3_maxpool3x3s2_f", "smallest", "one pixel, C = 8", s3_maxpool(1, 1, 1, 8))


def s3_split(rows, c, merge):
    def build(L):
        v = U((rows, c))
        if merge:
            spec = {"x": In(split3(v)), "y": Out((rows, c), F32)}
            return spec, lambda t: L.vqseg_s3_merge_f(ptr(t["x"]), rows, c, ptr(t["y"]), stream()), {}, None
        spec = {"x": In(v), "y": Out((rows, 2 * c), BF16)}
        return spec, lambda t: L.vqseg_s3_split_f(ptr(t["x"]), rows, c, ptr(t["y"]), stream()), {}, None
    return build


for E, _m in (("vqseg_s3_split_f", False), ("vqseg_s3_merge_f", True)):
    add(E, "ragged", "8 channels a thread, 256 threads: 257 rows of C = 8", s3_split(257, 8, _m))
    add(E, "ragged-C24", "129 rows of C = 24", s3_split(129, 24, _m))
    add(E, "smallest", "one row, C = 8", s3_split(1, 8, _m))


def cast(to_bf16, n):
    def build(L):
        spec = {"x": In(U(n, dtype=F32 if to_bf16 else BF16), 2), "y": Out(n, BF16 if to_bf16 else F32, 2)}
        return spec, lambda t: L.vqseg_cast_f(to_bf16, ptr(t["x"]), n, ptr(t["y"]), stream()), {}, None
    return build


for _to in (0, 1):
    add("vqseg_cast_f", f"to_bf16-{_to}-odd", "n = 2049: odd, past whole workgroups and whole vectors", cast(_to, 2049))
    add("vqseg_cast_f", f"to_bf16-{_to}-smallest", "n = 1", cast(_to, 1))


def head_x(bf16, m, cin):
    return split3(U((m, cin))) if bf16 == 2 else U((m, cin), dtype=BF16 if bf16 else F32)


def head_fwd(bf16, m, cin, cout):
    def build(L):
        spec = {"x": In(head_x(bf16, m, cin)), "w": In(U((cout, cin)), 4), "y": Out((m, cout), F32, 4)}
        return spec, lambda t: L.vqseg_head1x1_forward_f(bf16, ptr(t["x"]), ptr(t["w"]), m, cin, cout, ptr(t["y"]), stream()), {}, None
    return build


E = "vqseg_head1x1_forward_f"
for _bf in (0, 1, 2):
    add(E, f"type{_bf}-ragged", "a row a thread, 256 threads: M = 257; Cin 24, Cout 3 (12-byte rows of logits)", head_fwd(_bf, 257, 24, 3))
    add(E, f"type{_bf}-widest", "M = 129; Cin 64, Cout 4", head_fwd(_bf, 129, 64, 4))
    add(E, f"type{_bf}-smallest", "one row, Cin 8, Cout 1", head_fwd(_bf, 1, 8, 1))


def head_bwd(bf16, m, cin, cout, add_mode):
    """add_mode: None (vqseg_head1x1_backward_f), False / True (vqseg_head1x1_backward_add_f without / with gx_add)"""
    def build(L):
        dt = BF16 if bf16 else F32
        nf = int(L.vqseg_head1x1_backward_workspace_floats(m, cin, cout))
        assert nf == (m + 2047) // 2048 * cin * cout
        spec = {"x": In(head_x(bf16, m, cin)), "w": In(U((cout, cin)), 4), "g": In(U((m, cout)), 4), "gx": Out((m, cin), dt), "gw": Out((cout, cin), F32, 4),
                "ws": Ws(4 * nf), "gx_add": In(U((m, cin), dtype=dt)) if add_mode else None}
        if add_mode is None:
            call = lambda t: L.vqseg_head1x1_backward_f(bf16, ptr(t["x"]), ptr(t["w"]), ptr(t["g"]), m, cin, cout, ptr(t["gx"]), ptr(t["gw"]), ptr(t["ws"]), stream())
        else:
            call = lambda t: L.vqseg_head1x1_backward_add_f(bf16, ptr(t["x"]), ptr(t["w"]), ptr(t["g"]), m, cin, cout, ptr(t["gx"]), ptr(t["gw"]), ptr(t["ws"]),
                                                            ptr(t["gx_add"]), stream())
        return spec, call, {}, None
    return build


for E, _modes in (("vqseg_head1x1_backward_f", (None,)), ("vqseg_head1x1_backward_add_f", (True, False))):
    for _am in _modes:
        _t = "" if _am is None else ("-add" if _am else "-noadd")
        for _bf in (0, 1):
            add(E, f"type{_bf}-ragged{_t}", "HEAD_ROWS = 2048 rows a block: M = 2049; Cin 24, Cout 3", head_bwd(_bf, 2049, 24, 3, _am))
            add(E, f"type{_bf}-widest{_t}", "M = 257; Cin 64, Cout 4 (Cin Cout = 256, the limit)", head_bwd(_bf, 257, 64, 4, _am))
            add(E, f"type{_bf}-smallest{_t}", "one row, Cin 8, Cout 1", head_bwd(_bf, 1, 8, 1, _am))


def im2col(form, n, h, w, cin, k, stride, pad, reflect, kp, opts=None):
    def build(L):
        ho, wo = out_hw(h, w, k, stride, pad)
        al = 16 if (k == 7 and cin == 3 and kp % 8 == 0) else 2          # 16-byte stores on the stem's own shape only
        spec = {"x": In(U((n, h, w, cin)), 4), "out": Out((n * ho * wo, kp * (2 if form == 2 else 1)), F32 if form == 0 else BF16, al)}
        call = lambda t: L.vqseg_im2col_f(form, ptr(t["x"]), n, h, w, cin, k, k, stride, pad, int(reflect), ho, wo, kp, ptr(t["out"]), stream())
        return spec, call, opts or {}, None
    return build


E = "vqseg_im2col_f"
for _form in (0, 1, 2):
    for _r in (False, True):
        _t = f"form{_form}-{'reflect' if _r else 'zero'}"
        add(E, "strip-" + _t, "strips of 64 / 128 output pixels: 9 x 257 -> 5 x 129 = 2 x 64 + 1 = 128 + 1", im2col(_form, 2, 9, 257, 3, 7, 2, 3, _r, 160))
        add(E, "stem7-gather-" + _t, "the same shape with im2col_strip = 0: 8 columns a thread", im2col(_form, 2, 9, 257, 3, 7, 2, 3, _r, 160, {"im2col_strip": 0}))
        add(E, "smallest-" + _t, "4 x 4 -> 2 x 2 (reflect needs pad 3 < H, W)", im2col(_form, 1, 4, 4, 3, 7, 2, 3, _r, 160))
        if _form < 2:
            add(E, "generic-" + _t, "any kernel: 3x3 over 4 channels, kp = 40 = 36 + 4 zero columns; 5 x 7", im2col(_form, 2, 5, 7, 4, 3, 1, 1, _r, 40))
            add(E, "generic-stride2-" + _t, "5x5 stride 2 over 3 channels, kp = 75 (odd); 9 x 11", im2col(_form, 1, 9, 11, 3, 5, 2, 2, _r, 75))
add(E, "strip-form2-kp192", "the split-3 forward's 192-column rows; 5 x 129", im2col(2, 1, 9, 257, 3, 7, 2, 3, True, 192))
add(E, "smallest-one-pixel", "1 x 1 -> 1 x 1, zero padding", im2col(0, 1, 1, 1, 3, 7, 2, 3, False, 160))


def reflect_fold(bf16, n, h, w, c):
    def build(L):
        dt = BF16 if bf16 else F32
        al = act_align(bf16, c)
        spec = {"gp": In(U((n, h + 2, w + 2, c), dtype=dt), al), "gx": Out((n, h, w, c), dt, al)}
        return spec, lambda t: L.vqseg_reflect_fold_f(bf16, ptr(t["gp"]), n, h, w, c, ptr(t["gx"]), stream()), {}, None
    return build


E = "vqseg_reflect_fold_f"
for _bf, _c, _note in ROWVEC:
    add(E, f"{'bf16' if _bf else 'f32'}-C{_c}", _note + "; 9 x 17, three images", reflect_fold(_bf, 3, 9, 17, _c))
    add(E, f"{'bf16' if _bf else 'f32'}-C{_c}-smallest", _note + "; H = W = 2", reflect_fold(_bf, 1, 2, 2, _c))
add(E, "smallest", "H = W = 2, C = 1", reflect_fold(0, 1, 2, 2, 1))


def stem7(s3, n, h, w, reflect, affine, relu):
    def build(L):
        ho, wo = out_hw(h, w, 7, 2, 3)
        m = n * ho * wo
        img = U((64, 2 if s3 else 1, 176), -0.1, 0.1, dtype=BF16)
        spec = {"x": In(U((n, h, w, 3))), "w_img": In(img), "y": Out((m, 128 if s3 else 64), BF16), "stat": None if affine else stat_spec(L, m, 64),
                "scale": In(U(64, 0.5, 1.5), 4) if affine else None, "shift": In(U(64, -0.5, 0.5), 4) if affine else None}
        call = lambda t: L.vqseg_stem7_conv_f(s3, ptr(t["x"]), ptr(t["w_img"]), ptr(t["y"]), ptr(t["stat"]), ptr(t["scale"]), ptr(t["shift"]), relu, n, h, w, int(reflect),
                                              stream())
        return spec, call, {}, None
    return build


E = "vqseg_stem7_conv_f"
for _r in (False, True):
    _t = "reflect" if _r else "zero"
    for _s3, _aff, _name in ((0, False, "stat"), (0, True, "affine"), (1, True, "split3")):
        add(E, f"{_name}-{_t}-ragged", "strips of 128 output pixels (output width % 128 required): 5 x 511 -> 3 x 256, odd extents, two images", stem7(_s3, 2, 5, 511, _r, _aff, 1))
        add(E, f"{_name}-{_t}-smallest", "4 x 255 -> 2 x 128: the narrowest and lowest image the entry point takes", stem7(_s3, 1, 4, 255, _r, _aff, 0))


def reflect_ring(n, h, w, cgy, cgx):
    def build(L):
        rl = 2 * (w + 2) + 2 * h
        t_hi, _ = packed(L, weight(cgy, cgx, 3, 3), 1)
        spec = {"gy": In(U((n, h, w, cgy), dtype=BF16)), "t_hi": In(t_hi), "ring": InOut(U((n * rl, cgx), dtype=BF16)), "gx": InOut(U((n * h * w, cgx), dtype=BF16))}
        return spec, lambda t: L.vqseg_reflect_ring_f(ptr(t["gy"]), ptr(t["t_hi"]), ptr(t["ring"]), ptr(t["gx"]), n, h, w, cgy, cgx, stream()), {}, None
    return build


E = "vqseg_reflect_ring_f"
add(E, "ragged-bn64", "128 ring pixels a tile: 4 x 59 -> ring of 130; Cgx 72 = 64 + 8", reflect_ring(1, 4, 59, 64, 72))
add(E, "ragged-bn128", "5 x 7, five images: ring of 5 x 28 = 140; Cgy 128, Cgx 136", reflect_ring(5, 5, 7, 128, 136))
add(E, "ragged-bn32", "4 x 59; Cgx 40 = 32 + 8", reflect_ring(1, 4, 59, 64, 40))
add(E, "smallest", "H = W = 4, Cgy 64, Cgx 8", reflect_ring(1, 4, 4, 64, 8))


# ==============================================================================================================================
# VQ.  Distance + arg-min: 128 rows a workgroup (ROWS_PER_WG), 32-code tiles, 4-channel interleave (fp32) / 8 (bf16, split-3);
# candidate filter: 128 x 256 tiles, K % 256 == 0 and C % 32 == 0; gather: 16 rows a block; k-means / code sums: KM_RB = 1024
# rows a block, KM_SEG = 128 members a segment.
# ==============================================================================================================================
def codebook(k, c, collapsed=False):
    """collapsed: every code equals code 0 (tests/test_vq_filter_gpu.py, "collapsed"): the bf16 filter cannot tell the codes apart,
    every row keeps ~K candidates, the candidate pair list -- 8 sub-lists of 1024 pairs in use at N = 129 -- overflows, the appends
    are clamped at the list's capacity, the overflow flag is set and the gated launch of the exact kernel serves the level"""
    cb = U((k, c), -1, 1)
    if collapsed:
        cb[:] = cb[0].clone()
    return cb


def overflowed(n, c, k, ws="ws"):
    """POST check: the filter's overflow flag (the 65th int at vqseg_vq_filter_counter_offset) is set after the call"""
    def check(L, t):
        off = L.vqseg_vq_filter_counter_offset(n, c, k)
        assert off, "the shape does not take the filter"
        state = t[ws].reshape(-1).view(U8)[off:off + 260].cpu().view(I32)
        assert int(state[64]) != 0, f"the candidate list did not overflow ({int(state[:64].sum())} pairs): the gated exact launch did not run"
    return check


def prepared_blob(L, cb):
    k, c = cb.shape
    nb = L.vqseg_vq_prepared_bytes(c, k)
    cbd = cb.to(dev())
    blob = torch.zeros(nb, dtype=U8, device=dev())
    ok(L.vqseg_vq_prepare_f32(cbd.data_ptr(), c, k, blob.data_ptr(), nb, stream()))
    torch.cuda.synchronize()
    return blob.cpu()


def vq_rows(kind, n, c, cb):
    """rows near codes (so that the arg-min is not a lottery of ties), in the row type of `kind` (0 f32, 1 bf16, 2 split-3)"""
    k = cb.shape[0]
    pick = (U(n, 0, k)).long().clamp(0, k - 1)
    v = cb[pick] + U((n, c), -0.05, 0.05)
    return split3(v) if kind == 2 else v.to(BF16 if kind == 1 else F32)


def prepared_content(c, k, nb):
    """The byte ranges of a prepared codebook that hold something (vq_host.hip, prepared_layout): the 4-channel interleaved copy
    [C][Kp] fp32 and |e_k|^2 [Kp] fp32, Kp = K rounded up to 32 -- what the header documents; then, 256-byte aligned, a slot of 256
    bytes whose first float is the filter's largest norm, and the filter's bf16 image [hi | lo][C][Kp] for the shapes that take the
    filter (K % 256 == 0, C % 32 == 0).  The gaps are alignment padding that nothing writes or reads."""
    kp = (k + 31) // 32 * 32
    up256 = lambda v: (v + 255) // 256 * 256
    head = (c * kp + kp) * 4
    off_enmax = up256(head)
    off_eb = off_enmax + 256
    if k % 256 == 0 and c % 32 == 0:
        assert nb == up256(off_eb + 2 * c * kp * 2)
        return [(0, head), (off_enmax, off_enmax + 4), (off_eb, off_eb + 2 * c * kp * 2)]
    assert nb == off_eb
    return [(0, head)]


def vq_prepare(c, k):
    def build(L):
        nb = L.vqseg_vq_prepared_bytes(c, k)
        spec = {"codebook": In(codebook(k, c)), "prepared": Out(nb, U8, compare=prepared_content(c, k, nb))}
        call = lambda t, short=0: L.vqseg_vq_prepare_f32(ptr(t["codebook"]), c, k, ptr(t["prepared"]), nb - short, stream())
        return spec, call, {}, lambda t: call(t, 1)
    return build


E = "vqseg_vq_prepare_f32"
add(E, "ragged", "32-code padding, 4-channel interleave: K = 33, C = 36", vq_prepare(36, 33))
add(E, "ragged-C4", "K = 33, C = 4", vq_prepare(4, 33))
add(E, "filter-shape", "K = 256, C = 32 (the shape the bf16 filter takes)", vq_prepare(32, 256))
add(E, "smallest", "one code, C = 4", vq_prepare(4, 1))

ASSIGN = {0: "vqseg_vq_assign_f32", 1: "vqseg_vq_assign_bf16", 2: "vqseg_vq_assign_s3"}
FORWARD = {0: "vqseg_vq_forward_f32", 1: "vqseg_vq_forward_bf16"}


def vq_assign(kind, n, c, k, with_prepared, with_dmin, opts=None, collapsed=False):
    def build(L):
        cb = codebook(k, c, collapsed)
        nb = L.vqseg_vq_workspace_bytes(n, c, k)
        spec = {"x": In(vq_rows(kind, n, c, cb)), "codebook": In(cb), "prepared": In(prepared_blob(L, cb)) if with_prepared else None,
                "idx": Out(n, I64, 8), "dmin": Out(n, F32, 4) if with_dmin else None, "ws": Ws(nb)}
        fn = getattr(L, ASSIGN[kind])
        call = lambda t, short=0: fn(ptr(t["x"]), ptr(t["codebook"]), ptr(t["prepared"]), n, c, k, ptr(t["idx"]), ptr(t["dmin"]), ptr(t["ws"]), nb - short, stream())
        return spec, call, opts or {}, lambda t: call(t, 1)
    return build


def vq_forward(kind, n, c, k, with_prepared, training, with_dmin, opts=None, collapsed=False):
    def build(L):
        cb = codebook(k, c, collapsed)
        nb = L.vqseg_vq_workspace_bytes(n, c, k)
        spec = {"x": In(vq_rows(kind, n, c, cb)), "codebook": In(cb), "prepared": In(prepared_blob(L, cb)) if with_prepared else None,
                "quant": Out((n, c), BF16 if kind else F32), "idx": Out(n, I64, 8), "loss": Out(1, F32, 4), "dead_pct": Out(1, F32, 4),
                "dmin": Out(n, F32, 4) if with_dmin else None, "ws": Ws(nb)}
        fn = getattr(L, FORWARD[kind])
        call = lambda t, short=0: fn(ptr(t["x"]), ptr(t["codebook"]), ptr(t["prepared"]), n, c, k, training, 0.25, ptr(t["quant"]), ptr(t["idx"]), ptr(t["loss"]),
                                     ptr(t["dead_pct"]), ptr(t["dmin"]), ptr(t["ws"]), nb - short, stream())
        return spec, call, opts or {}, lambda t: call(t, 1)
    return build


_VQG = "128 rows a workgroup: N = 129; 32-code tiles: K = 33; "
for _kind in (0, 1, 2):
    E = ASSIGN[_kind]
    _cs = (4, 36) if _kind == 0 else (8, 40)
    for _c in _cs:
        add(E, f"ragged-C{_c}", _VQG + f"C = {_c}", vq_assign(_kind, 129, _c, 33, False, True))
        add(E, f"ragged-C{_c}-prepared", _VQG + f"C = {_c}; prepared codebook, no dmin", vq_assign(_kind, 129, _c, 33, True, False))
    add(E, "smallest", f"one row, one code, C = {_cs[0]}", vq_assign(_kind, 1, _cs[0], 1, False, True))
    add(E, "tiles-cap-1", _VQG + "vq_max_tiles_per_wave = 1; K = 65", vq_assign(_kind, 129, _cs[1], 65, True, True, {"vq_max_tiles_per_wave": 1}))
    if _kind:
        _f = "vq_bf16_filter" if _kind == 1 else "vq_s3_filter"
        add(E, "filter-on", "filter tile 128 x 256: N = 129, K = 256, C = 32", vq_assign(_kind, 129, 32, 256, True, True, {_f: 1}))
        add(E, "filter-off", "the same shape on the exact kernel", vq_assign(_kind, 129, 32, 256, True, True, {_f: 0}))
        add(E, "filter-force-all", "the same shape, every row re-scored", vq_assign(_kind, 129, 32, 256, False, True, {_f: 1, "vq_filter_force_all": 1}))
        add(E, "filter-K512-C64", "N = 257, K = 512, C = 64", vq_assign(_kind, 257, 64, 512, True, False, {_f: 1}))
        for _prep in (True, False):
            _n = "filter-overflow-exact-fallback" + ("" if _prep else "-unprepared")
            add(E, _n, "collapsed codebook at N = 129, K = 256, C = 32: pair list clamped at its capacity, gated exact launch", vq_assign(_kind, 129, 32, 256, _prep, True, {_f: 1}, True))
            POST[(E, _n)] = overflowed(129, 32, 256)
for _kind in (0, 1):
    E = FORWARD[_kind]
    _cs = (4, 36) if _kind == 0 else (8, 40)
    for _train in (0, 1):
        add(E, f"ragged-C{_cs[0]}-train{_train}", _VQG + f"gather: 16 rows a block; C = {_cs[0]}", vq_forward(_kind, 129, _cs[0], 33, False, _train, True))
        add(E, f"ragged-C{_cs[1]}-train{_train}-prepared", _VQG + f"C = {_cs[1]}; no dmin", vq_forward(_kind, 129, _cs[1], 33, True, _train, False))
        add(E, f"smallest-train{_train}", "one row, one code", vq_forward(_kind, 1, _cs[0], 1, False, _train, True))
    if _kind:
        add(E, "filter-on", "N = 129, K = 256, C = 32", vq_forward(_kind, 129, 32, 256, True, 1, False, {"vq_bf16_filter": 1}))
        add(E, "filter-off", "the same on the exact kernel", vq_forward(_kind, 129, 32, 256, True, 1, False, {"vq_bf16_filter": 0}))
        for _train in (0, 1):
            _n = f"filter-overflow-exact-fallback-train{_train}"
            add(E, _n, "collapsed codebook at N = 129, K = 256, C = 32: pair list clamped, gated exact launch", vq_forward(_kind, 129, 32, 256, bool(_train), _train, True, {"vq_bf16_filter": 1}, True))
            POST[(E, _n)] = overflowed(129, 32, 256)


def vq_group(kind, levels, training, with_prepared, opts=None, collapsed=()):
    """levels: (n, c, k) each.  The pointer and size arrays are host arrays (include/vqseg.h); they are built per call."""
    def build(L):
        nl = len(levels)
        spec, nbs = {}, []
        for i, (n, c, k) in enumerate(levels):
            cb = codebook(k, c, i in collapsed)
            nbs.append(L.vqseg_vq_workspace_bytes(n, c, k))
            spec.update({f"x{i}": In(vq_rows(kind, n, c, cb)), f"codebook{i}": In(cb), f"prepared{i}": In(prepared_blob(L, cb)) if with_prepared else None,
                         f"quant{i}": Out((n, 2 * c if kind == 2 else c), BF16 if kind else F32), f"idx{i}": Out(n, I64, 8), f"loss{i}": Out(1, F32, 4),
                         f"dead_pct{i}": Out(1, F32, 4), f"ws{i}": Ws(nbs[-1])})

        def call(t, short=0):
            arr = lambda name: (ctypes.c_void_p * nl)(*[ptr(t[f"{name}{i}"]) for i in range(nl)])
            ns = (ctypes.c_int64 * nl)(*[lv[0] for lv in levels])
            cs = (ctypes.c_int * nl)(*[lv[1] for lv in levels])
            ks = (ctypes.c_int * nl)(*[lv[2] for lv in levels])
            cw = (ctypes.c_float * nl)(*[0.25] * nl)
            wsb = (ctypes.c_size_t * nl)(*[nb - (short if i == nl - 1 else 0) for i, nb in enumerate(nbs)])
            keep = (arr("x"), arr("codebook"), arr("prepared") if with_prepared else None, arr("quant"), arr("idx"), arr("loss"), arr("dead_pct"), arr("ws"))
            a = lambda v: ctypes.cast(v, ctypes.c_void_p)
            return L.vqseg_vq_forward_group(nl, kind, a(keep[0]), a(keep[1]), a(keep[2]) if with_prepared else None, a(ns), a(cs), a(ks), training, a(cw),
                                            a(keep[3]), a(keep[4]), a(keep[5]), a(keep[6]), a(keep[7]), a(wsb), stream())
        return spec, call, opts or {}, lambda t: call(t, 1)
    return build


E = "vqseg_vq_forward_group"
_LV = "three levels of different N and K: "
add(E, "f32-train", _LV + "(129, 4, 33), (17, 36, 5), (300, 8, 65)", vq_group(0, [(129, 4, 33), (17, 36, 5), (300, 8, 65)], 1, False))
add(E, "f32-eval-prepared", _LV + "(129, 36, 33), (1, 4, 1), (257, 4, 100)", vq_group(0, [(129, 36, 33), (1, 4, 1), (257, 4, 100)], 0, True))
add(E, "bf16-train", _LV + "(129, 8, 33), (17, 40, 5), (300, 16, 65)", vq_group(1, [(129, 8, 33), (17, 40, 5), (300, 16, 65)], 1, True))
# the grouped launch takes the filter only when EVERY level has a filter shape (launch_assign_group): K % 256 == 0, C % 32 == 0
_FL = [(129, 32, 256), (17, 32, 256), (257, 64, 512)]
_FS = [(17, 64, 256), (257, 32, 512), (129, 32, 256)]
add(E, "bf16-filter", _LV + "all filtered: (129, 32, 256), (17, 32, 256), (257, 64, 512)", vq_group(1, _FL, 1, True))
add(E, "bf16-filter-off", "the same levels, vq_bf16_filter = 0", vq_group(1, _FL, 1, True, {"vq_bf16_filter": 0}))
add(E, "split3", _LV + "(129, 8, 33), (17, 40, 5), (129, 32, 256): one level without a filter shape, so the exact kernel on all", vq_group(2, [(129, 8, 33), (17, 40, 5), (129, 32, 256)], 0, True))
add(E, "split3-filter", _LV + "all filtered: (17, 64, 256), (257, 32, 512), (129, 32, 256)", vq_group(2, _FS, 0, True))
add(E, "split3-filter-off", "the same levels, vq_s3_filter = 0", vq_group(2, _FS, 0, False, {"vq_s3_filter": 0}))
_OV = "on a collapsed codebook: pair list clamped at its capacity, gated exact launch; the other two filtered levels do not overflow"
add(E, "bf16-filter-overflow-exact-fallback", "level (129, 32, 256), the first, " + _OV, vq_group(1, _FL, 1, True, collapsed=(0,)))
add(E, "split3-filter-overflow-exact-fallback", "level (129, 32, 256), the last, " + _OV, vq_group(2, _FS, 0, False, collapsed=(2,)))
POST[(E, "bf16-filter-overflow-exact-fallback")] = overflowed(129, 32, 256, "ws0")
POST[(E, "split3-filter-overflow-exact-fallback")] = overflowed(129, 32, 256, "ws2")
add(E, "smallest", "one level, one row, one code", vq_group(0, [(1, 4, 1)], 1, False))


def vq_backward(bf16, n, c, k, with_gloss):
    def build(L):
        dt = BF16 if bf16 else F32
        cb = codebook(k, c)
        idx = U(n, 0, k).long().clamp(0, k - 1)
        spec = {"gq": In(U((n, c), dtype=dt)), "gloss": In(U(1, 0.5, 1.5), 4) if with_gloss else None, "x": In(U((n, c), dtype=dt)), "gx": Out((n, c), dt)}
        if bf16:
            spec.update({"idx": In(idx, 8), "codebook": In(cb)})
            call = lambda t: L.vqseg_vq_backward_bf16(ptr(t["gq"]), ptr(t["gloss"]), ptr(t["x"]), ptr(t["idx"]), ptr(t["codebook"]), n, c, 0.25, ptr(t["gx"]), stream())
        else:
            spec["quant"] = In(cb[idx].contiguous())
            call = lambda t: L.vqseg_vq_backward_f32(ptr(t["gq"]), ptr(t["gloss"]), ptr(t["x"]), ptr(t["quant"]), n, c, 0.25, ptr(t["gx"]), stream())
        return spec, call, {}, None
    return build


for _bf, E in ((0, "vqseg_vq_backward_f32"), (1, "vqseg_vq_backward_bf16")):
    _c = 8 if _bf else 4
    add(E, "ragged", f"16-byte vectors, 256 threads: N = 257 rows of C = {_c}", vq_backward(_bf, 257, _c, 33, True))
    add(E, "ragged-wide-nogloss", f"N = 129, C = {_c + 32}; grad_loss NULL", vq_backward(_bf, 129, _c + 32, 33, False))
    add(E, "smallest", f"one row, C = {_c}", vq_backward(_bf, 1, _c, 1, True))


def km_assignment(n, k):
    """an assignment with an empty cluster (the last but one) and a cluster of KM_SEG + 1 = 129 members (cluster 0)"""
    idx = torch.zeros(n, dtype=I64)
    if k > 2 and n > 129:
        others = [j for j in range(1, k) if j != k - 2]
        idx[129:] = torch.tensor(others)[torch.arange(n - 129) % len(others)]
        idx = idx[torch.randperm(n, generator=torch.Generator().manual_seed(n + k))]
    return idx


def code_sums(bf16, n, c, k):
    def build(L):
        nb = L.vqseg_kmeans_workspace_bytes(n, c, k)
        spec = {"x": In(U((n, c), dtype=BF16 if bf16 else F32), 2), "idx": In(km_assignment(n, k), 8), "sums": Out((k, c), F32, 4), "counts": Out(k, I64, 8),
                "ws": Ws(nb)}
        call = lambda t, short=0: L.vqseg_vq_code_sums(bf16, ptr(t["x"]), ptr(t["idx"]), n, c, k, ptr(t["sums"]), ptr(t["counts"]), ptr(t["ws"]), nb - short, stream())
        return spec, call, {}, lambda t: call(t, 1)
    return build


_KMG = "KM_RB = 1024 rows a block: N = 1025; an empty cluster and one of KM_SEG + 1 = 129 members; K = 33; "
E = "vqseg_vq_code_sums"
for _bf in (0, 1):
    _t = "bf16" if _bf else "f32"
    add(E, f"{_t}-ragged", _KMG + f"C = {8 if _bf else 4}", code_sums(_bf, 1025, 8 if _bf else 4, 33))
    add(E, f"{_t}-ragged-wide", _KMG + f"C = {40 if _bf else 36}", code_sums(_bf, 1025, 40 if _bf else 36, 33))
    add(E, f"{_t}-smallest", "one row, one code", code_sums(_bf, 1, 8 if _bf else 4, 1))


def km_samples(n, c, k):
    """means 10 apart along the first channel, samples within 0.05 of the mean of km_assignment's cluster: the assignment IS that one"""
    means = U((k, c), -0.5, 0.5)
    means[:, 0] += 10.0 * torch.arange(k)
    return means[km_assignment(n, k)] + U((n, c), -0.05, 0.05), means + U((k, c), -0.01, 0.01)


def kmeans(n, c, k, iters):
    def build(L):
        nb = L.vqseg_kmeans_workspace_bytes(n, c, k)
        samples, means = km_samples(n, c, k)
        spec = {"samples": In(samples), "means": InOut(means), "bins": Out(k, I64, 8), "ws": Ws(nb)}
        call = lambda t, short=0: L.vqseg_kmeans_f32(ptr(t["samples"]), ptr(t["means"]), ptr(t["bins"]), n, c, k, iters, ptr(t["ws"]), nb - short, stream())
        return spec, call, {}, lambda t: call(t, 1)
    return build


def kmeans_accumulate(n, c, k):
    def build(L):
        nb = L.vqseg_kmeans_workspace_bytes(n, c, k)
        samples, means = km_samples(n, c, k)
        spec = {"samples": In(samples), "means": In(means), "sums": Out((k, c), F32, 4), "counts": Out(k, I64, 8), "ws": Ws(nb)}
        call = lambda t, short=0: L.vqseg_kmeans_accumulate_f32(ptr(t["samples"]), ptr(t["means"]), n, c, k, ptr(t["sums"]), ptr(t["counts"]), ptr(t["ws"]), nb - short,
                                                                stream())
        return spec, call, {}, lambda t: call(t, 1)
    return build


def kmeans_finalize(c, k):
    def build(L):
        counts = U(k, 0, 5).long()
        counts[k // 2] = 0                                      # a cluster with no member keeps its mean
        spec = {"sums": In(U((k, c)), 4), "counts": In(counts, 8), "means": InOut(U((k, c)), 4)}
        return spec, lambda t: L.vqseg_kmeans_finalize_f32(ptr(t["sums"]), ptr(t["counts"]), ptr(t["means"]), c, k, stream()), {}, None
    return build


for _c in (4, 36):
    add("vqseg_kmeans_f32", f"ragged-C{_c}", _KMG + f"C = {_c}; two iterations", kmeans(1025, _c, 33, 2))
    add("vqseg_kmeans_accumulate_f32", f"ragged-C{_c}", _KMG + f"C = {_c}", kmeans_accumulate(1025, _c, 33))
    add("vqseg_kmeans_finalize_f32", f"ragged-C{_c}", f"K = 33 with an empty cluster, C = {_c}", kmeans_finalize(_c, 33))
add("vqseg_kmeans_f32", "smallest", "one row, one code, one iteration", kmeans(1, 4, 1, 1))
add("vqseg_kmeans_accumulate_f32", "smallest", "one row, one code", kmeans_accumulate(1, 4, 1))
add("vqseg_kmeans_finalize_f32", "smallest", "one code, C = 4", kmeans_finalize(4, 1))
add("vqseg_kmeans_finalize_f32", "ragged-K257", "K = 257, C = 4", kmeans_finalize(4, 257))


def ema_state(k, c):
    return {"cluster_size": InOut(U(k, 0, 4), 4), "embed_avg": InOut(U((k, c), -2, 2), 4), "codebook": InOut(U((k, c)), 4), "sums": In(U((k, c), -3, 3), 4),
            "counts": In(U(k, 0, 6).long(), 8)}


def ema_update(c, k):
    def build(L):
        spec = dict(ema_state(k, c), scratch=Ws(4, 4))
        call = lambda t: L.vqseg_vq_ema_update_f32(ptr(t["cluster_size"]), ptr(t["embed_avg"]), ptr(t["codebook"]), ptr(t["sums"]), ptr(t["counts"]), c, k, 0.99, 1e-5,
                                                   ptr(t["scratch"]), stream())
        return spec, call, {}, None
    return build


def ema_update_revive(c, k):
    def build(L):
        ok_k = (U(k) > -0.5).float()
        spec = dict(ema_state(k, c), scratch=Ws(4 * (1 + k), 4), cand=In(U((k, c)), 4), ok=In(ok_k, 4), counter=InOut(torch.full((1,), 7, dtype=I64), 8),
                    revived=Out(1, I64, 8))
        call = lambda t: L.vqseg_vq_ema_update_revive_f32(ptr(t["cluster_size"]), ptr(t["embed_avg"]), ptr(t["codebook"]), ptr(t["sums"]), ptr(t["counts"]), c, k, 0.5,
                                                          1e-5, ptr(t["scratch"]), ptr(t["cand"]), ptr(t["ok"]), 1.5, ptr(t["counter"]), ptr(t["revived"]), stream())
        return spec, call, {}, None
    return build


def revive_candidates(bf16, n, c, k, rank, world):
    def build(L):
        x = U((n, c), dtype=BF16 if bf16 else F32)
        x[n // 2] = float("inf")                                # a row that is not entirely finite: ok = 0 for the codes that draw it
        spec = {"x": In(x), "counter": In(torch.full((1,), 3, dtype=I64), 8), "cand": Out((k, c), F32), "ok": Out(k, F32, 4)}
        call = lambda t: L.vqseg_vq_revive_candidates(bf16, ptr(t["x"]), n, c, k, 0x1234567890ABCDEF, ptr(t["counter"]), rank, world, ptr(t["cand"]), ptr(t["ok"]),
                                                      stream())
        return spec, call, {}, None
    return build


for E, _mk in (("vqseg_vq_ema_update_f32", ema_update), ("vqseg_vq_ema_update_revive_f32", ema_update_revive)):
    add(E, "ragged", "K = 257 = 256 + 1 (the reduction of S over the codes), C = 4", _mk(4, 257))
    add(E, "ragged-wide", "K = 33, C = 36", _mk(36, 33))
    add(E, "ragged-C5", "C = 5 (the entry point asks no multiple of 4), K = 65", _mk(5, 65))
    add(E, "smallest", "one code, one channel", _mk(1, 1))
E = "vqseg_vq_revive_candidates"
for _bf in (0, 1):
    _t = "bf16" if _bf else "f32"
    add(E, f"{_t}-ragged", f"K = 257, N = 129, C = {8 if _bf else 4}", revive_candidates(_bf, 129, 8 if _bf else 4, 257, 0, 1))
    add(E, f"{_t}-ragged-rank1of2", f"K = 33, N = 129, C = {40 if _bf else 36}; rank 1 of 2: the other rank's codes get zeros", revive_candidates(_bf, 129, 40 if _bf else 36, 33, 1, 2))
    add(E, f"{_t}-smallest", "one row, one code", revive_candidates(_bf, 1, 8 if _bf else 4, 1, 0, 1))

# pointers the header asks 16-byte alignment for and the entry point checks (nn_abi.hip): at 8 mod 16 they are refused
UNALIGNED += [(e, n, q) for e, n, ps in [
    ("vqseg_bn_apply_f", "bf16-C8", "y res out"), ("vqseg_bn_apply_f", "f32-C12", "y out"), ("vqseg_bn_apply_bits_f", "C24", "y res out"),
    ("vqseg_bn_backward_f", "bf16-out-res", "g_out out y g_y g_res ws"), ("vqseg_bn_backward_f", "f32-out-res-eval", "g_out out y g_y g_res ws"),
    ("vqseg_bn_backward_f", "f32-norelu-acc", "ws"), ("vqseg_bn_backward_bits_f", "res", "g_out y g_y g_res ws"),
    ("vqseg_maxpool3x3s2_f", "fwd-idx-bf16-C8", "x out"), ("vqseg_maxpool3x3s2_f", "bwd-x-f32-C4", "x g out"),
    ("vqseg_maxpool3x3s2_backward_add_f", "bf16-C8", "g gx_add gx"), ("vqseg_bilinear_f", "fwd-generic-align0-bf16-C8", "src dst"),
    ("vqseg_bilinear_f", "bwd-up2-opt1-f32", "src dst"), ("vqseg_reflect_fold_f", "bf16-C8", "gp gx"), ("vqseg_reflect_fold_f", "f32-C4", "gp gx"),
    ("vqseg_im2col_f", "strip-form0-zero", "out"), ("vqseg_im2col_f", "stem7-gather-form1-reflect", "out"), ("vqseg_im2col_f", "strip-form2-kp192", "out"),
    ("vqseg_conv2d_wgrad_f", "pertap-bf16-acc-concat", "gy x x2 ws"), ("vqseg_conv2d_wgrad2_f", "ninetap-nb1", "gy x gy_b x_b ws"),
    ("vqseg_conv_pack_weights_f32", "ragged-flip1-lo1", "hi lo"), ("vqseg_conv_pack_weights_s3_f32", "ragged", "out"),
    ("vqseg_conv_pack_weights_s2_f32", "ragged-k3", "hi lo"), ("vqseg_conv_pack_all_f32", "ragged-fwd+tr+s3", "fwd tr s3"),
    ("vqseg_kmeans_accumulate_f32", "ragged-C36", "samples means ws"), ("vqseg_kmeans_f32", "ragged-C4", "samples means ws"),
    ("vqseg_head1x1_backward_f", "type1-ragged", "ws"), ("vqseg_head1x1_backward_add_f", "type0-widest-add", "ws"),
] for q in ps.split()]


def check_table():
    """every entry point of ENTRY_POINTS has a ragged and a smallest case, every case names its granule, no name twice"""
    by_entry = collections.defaultdict(list)
    for c in CASES:
        by_entry[c.entry].append(c.name)
    assert len(ENTRY_POINTS) == len(set(ENTRY_POINTS)) == 47
    for name in ENTRY_POINTS:
        names = by_entry.get(name, [])
        assert names, f"{name}: no case in tests/extent_cases.py"
        assert any("smallest" in n for n in names), f"{name}: no smallest-shape case"
        assert any("smallest" not in n for n in names), f"{name}: no ragged case"
    assert set(by_entry) == set(ENTRY_POINTS), sorted(set(by_entry) ^ set(ENTRY_POINTS))
    assert all(c.granule for c in CASES), "every shape names the granule it is ragged against"
    assert len({(c.entry, c.name) for c in CASES}) == len(CASES), "duplicate case name"
    for key in list(POST) + [(e, n) for e, n, _ in UNALIGNED]:
        assert [c for c in CASES if (c.entry, c.name) == key], f"{key}: no such case"
