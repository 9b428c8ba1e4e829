"""Functional building blocks of the encoder/decoder, executed by the gfx950 HIP kernels behind
include/vqseg.h (conv_*.hip, nn_*.hip).  torch only owns memory and the autograd tape.

Layout: activations are NHWC in memory ("channels_last" views of logically NCHW tensors).
Precision follows the activation dtype: float32 -> "precise" kernels (bf16x3 split MFMA, fp32 storage;
the parity mode), bfloat16 -> "fast" kernels (bf16 storage and operands, fp32 accumulate).

Every function here has exactly one implementation; CPU tensors are refused (no fallback).  The one exception is the
prediction path's `resize_argmax`, which restates itself with torch ops for tensors that are not on the GPU, the way
measurement.confusion_matrix_device and evaluate.test_loop treat them.
"""
from __future__ import annotations

from collections import namedtuple
import contextlib
import ctypes
from typing import Optional
import weakref

import numpy as np
import torch
import torch.nn.functional as F

from . import _hip
from ._hip import lib
from ._wcache import cache_of as _cache_of, invalidate as invalidate_weight_caches  # noqa: F401


# ------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------
def _rows(x: torch.Tensor) -> torch.Tensor:
    """logical (N, C, H, W) -> contiguous (N, H, W, C) view (free for channels_last tensors)."""
    v = x.permute(0, 2, 3, 1)
    return v if v.is_contiguous() else v.contiguous()


def _nchw(rows: torch.Tensor) -> torch.Tensor:
    return rows.permute(0, 3, 1, 2)


def _is_bf16(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return 1
    if t.dtype == torch.float32:
        return 0
    raise _hip.HipLibraryError(f"activations must be float32 (precise mode) or bfloat16 (fast mode), got {t.dtype}")


_T = _hip.tptr                # every tensor handed to the library goes through this (dtype / density / element count / device checks)
_launch = _hip.launch         # ... and every kernel launch through this (device guard, current stream, return code)


def _w16(t, name, numel=None, at_least=False):
    """packed bf16 weight images travel as int16 tensors"""
    return _T(t, name, dtype=torch.int16, numel=numel, at_least=at_least)


def _f32(t, name, numel=None):
    return _T(t, name, dtype=torch.float32, numel=numel)


def _strided_f32(t, name, numel):
    """(B, C, H, W) fp32 logits addressed through the explicit (batch, class, pixel) strides passed along (NCHW and NHWC storage both
    qualify): a valid torch view bounds every such address by construction, so only type, element count and device are checked."""
    return _T(t, name, dtype=torch.float32, numel=numel, dense=False)


def act_dtype() -> torch.dtype:
    """bf16 'fast' mode under torch.autocast (the reference trainer's `autocast(enabled=half)`,
    train_vqreptunet1x1v2.py:151 -- fp16 there, bf16 here: the ROCm-native half type), else fp32."""
    if torch.is_autocast_enabled():
        return torch.bfloat16
    return torch.float32


def _pack_all(weight: torch.Tensor, kind):
    """bf16-mode images of a k x k (k = 1 or 3) conv weight -- kind "fwd", "tr" (data gradient) or ("s3", c1) -- built together
    in ONE launch (vqseg_conv_pack_all_f32) with every other kind this weight has been asked for before (the set survives the
    invalidation after each optimiser step, so from the second step on a layer costs one pack launch per step instead of three).
    None: not that kind of weight (the caller packs the single image)."""
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3] or weight.shape[2] not in (1, 3) or not py_opt("py_pack_all", 1):
        return None
    kinds = getattr(weight, "_vq_kinds", None)
    if kinds is None:
        kinds = weight._vq_kinds = set()
    if kind not in kinds:
        if isinstance(kind, tuple) and any(isinstance(k, tuple) and k != kind for k in kinds):
            return None                                      # a second concat split for the same weight: single-image path
        kinds.add(kind)
    cache = _cache_of(weight)
    imgs = cache.get("all")
    if imgs is None or kind not in imgs:
        w = weight.detach()
        w = w if w.is_contiguous() else w.contiguous()
        cout, cin, k, _ = w.shape
        cin_p, cout_p = _pad32(cin), _pad32(cout)
        s3k = next((kk for kk in kinds if isinstance(kk, tuple)), None)
        if s3k is not None and (cin % 32 or s3k[1] % 32):
            return None
        imgs = {}
        if "fwd" in kinds:
            imgs["fwd"] = torch.empty(cout * k * k * cin_p, dtype=torch.int16, device=w.device)
        if "tr" in kinds:
            imgs["tr"] = torch.empty(cin * k * k * cout_p, dtype=torch.int16, device=w.device)
        if s3k is not None:
            imgs[s3k] = torch.empty(cout * k * k * 3 * cin, dtype=torch.int16, device=w.device)
        _launch("vqseg_conv_pack_all_f32", w.device, _f32(w, "weight", cout * cin * k * k), cout, cin, k, s3k[1] if s3k is not None else cin,
                _w16(imgs.get("fwd"), "fwd image", cout * k * k * cin_p), _w16(imgs.get("tr"), "transposed image", cin * k * k * cout_p),
                _w16(imgs.get(s3k), "split-3 image", cout * k * k * 3 * cin) if s3k is not None else None)
        cache["all"] = imgs
    return imgs[kind]


def packed_weights(weight: torch.Tensor, precise: bool, transpose_flip: bool):
    """MFMA-side image of an nn.Conv2d weight, rebuilt only when the parameter changes (_wcache: version counter, storage,
    and every optimiser step)."""
    if not precise:
        img = _pack_all(weight, "tr" if transpose_flip else "fwd")
        if img is not None:
            return img, None
    cache = _cache_of(weight)
    k = (precise, transpose_flip)
    if k not in cache:
        w = weight.detach()
        w = w if w.is_contiguous() else w.contiguous()
        cout, cin, kh, kw = w.shape
        n = lib().vqseg_conv_packed_elems(cout, cin, kh, kw, int(transpose_flip))
        hi = torch.empty(n, dtype=torch.int16, device=w.device)
        lo = torch.empty(n, dtype=torch.int16, device=w.device) if precise else None
        _launch("vqseg_conv_pack_weights_f32", w.device, _f32(w, "weight", cout * cin * kh * kw), cout, cin, kh, kw, int(transpose_flip),
                _w16(hi, "packed hi", n), _w16(lo, "packed lo", n))
        cache[k] = (hi, lo)
    return cache[k]


def _pad32(c: int) -> int:
    return (c + 31) // 32 * 32


def _packed_elems(rows: int, kh: int, kw: int, cols: int) -> int:
    """elements of a packed weight image [rows][KH][KW][cols ^ 32] (vqseg_conv_packed_elems): THE size every kernel that reads one
    is bounded by"""
    return rows * kh * kw * _pad32(cols)


class ConvGeom(namedtuple("ConvGeom", "n h w c1 cin cout kh kw stride pad reflect ho wo")):
    """One convolution as the C entry points see it: input (n, h, w, cin) -- its first c1 channels from x, the rest from x2 -- to
    output (n, ho, wo, cout).  A data gradient is one too (its input is the output gradient).  Immutable, compared by value."""
    __slots__ = ()

    @property
    def m(self) -> int:
        return self.n * self.ho * self.wo

    @property
    def packed(self) -> int:
        return _packed_elems(self.cout, self.kh, self.kw, self.cin)


class StemGeom(namedtuple("StemGeom", "kh kw cin stride pad reflect h w fused", defaults=(None,))):
    """The 7x7 stem behind a 1x1 convolution over im2col patch columns: the kernel and the (h, w) image the patches come from.
    `fused` = (ho, wo, kp): the forward reads the IMAGE (vqseg_stem7_conv_f) and only backward builds the patch matrix."""
    __slots__ = ()

    @property
    def is_fused(self) -> bool:
        return self.fused is not None


# what two uses of a weight must share to go into one weight-gradient launch: everything but the batch size (geom.n = 0)
_WgradKey = namedtuple("_WgradKey", "geom precise stem")


_MODE_BF = (1, 0, 2)          # the convolutions' `precise` argument (0 bf16, 1 fp32 on split operands, 2 split-3 rows) -> tptr's `bf` flag


def _stat_elems(m: int, cout: int) -> int:
    return lib().vqseg_conv_stat_slots(m, cout) * 2 * cout


def _conv_raw(x_rows, x2_rows, w_hi, w_lo, stat, g: ConvGeom, up=1, w_offset_elems=0):
    """vqseg_conv2d_f -> y, BatchNorm partial sums into `stat`.  `up`: zero-dilation of the input (a strided layer's data gradient);
    `w_offset_elems`: where the [Cout][KH][KW][Cin ^ 32] slice the kernel reads starts in the weight image."""
    precise = x_rows.dtype == torch.float32
    y = torch.empty((g.n, g.ho, g.wo, g.cout), dtype=x_rows.dtype, device=x_rows.device)
    esz = 2
    bfa = 0 if precise else 1
    wneed = w_offset_elems + g.packed
    nin = g.n * g.h * g.w
    _launch("vqseg_conv2d_f", x_rows.device, _T(x_rows, "conv input", bf=bfa, numel=nin * g.c1),
            _T(x2_rows, "conv input 2", bf=bfa, numel=nin * (g.cin - g.c1)), g.c1,
            _w16(w_hi, "packed weights", wneed, at_least=True) + w_offset_elems * esz,
            (_w16(w_lo, "packed weights (lo)", wneed, at_least=True) + w_offset_elems * esz) if w_lo is not None else None,
            _T(y, "conv output", bf=bfa, numel=g.m * g.cout), _f32(stat, "BN partials", _stat_elems(g.m, g.cout) if stat is not None else None),
            g.n, g.h, g.w, g.cin, g.cout, g.kh, g.kw, g.stride, g.pad, int(g.reflect), up, g.ho, g.wo, int(precise))
    return y


def _conv_affine(x_rows, x2_rows, w_hi, w_lo, scale, shift, res, relu, g: ConvGeom, mode: int):
    """vqseg_conv2d_affine_f -> relu?(conv * scale + shift [+ res]) in one launch.  mode: the entry point's `precise` (_MODE_BF);
    split-3 rows hold [hi | lo] (twice the channels in memory) and read the [w_hi | w_hi | w_lo] weight image."""
    bf, f = _MODE_BF[mode], 2 if mode == 2 else 1
    wneed = g.cout * g.kh * g.kw * 3 * g.cin if mode == 2 else g.packed
    out = torch.empty((g.n, g.ho, g.wo, f * g.cout), dtype=_hip._BF_DTYPE[bf], device=x_rows.device)
    nin = g.n * g.h * g.w * f
    _launch("vqseg_conv2d_affine_f", x_rows.device, _T(x_rows, "conv input", bf=bf, numel=nin * g.c1),
            _T(x2_rows, "conv input 2", bf=bf, numel=nin * (g.cin - g.c1)), g.c1, _w16(w_hi, "packed weights", wneed),
            _w16(w_lo, "packed weights (lo)", wneed), _f32(scale, "scale", g.cout), _f32(shift, "shift", g.cout),
            _T(res, "residual", bf=bf, numel=g.m * g.cout * f), int(relu), _T(out, "conv output", bf=bf, numel=g.m * g.cout * f), g.n, g.h, g.w,
            g.cin, g.cout, g.kh, g.kw, g.stride, g.pad, int(g.reflect), g.ho, g.wo, mode)
    return out


def _conv_affine_bits(x_rows, w_hi, scale, shift, res, bits, g: ConvGeom):
    """vqseg_conv2d_affine_bits_f (bf16, stride 1, zero padding) -> conv * scale + shift + res .* bits (a ReLU mask bit field)"""
    out = torch.empty((g.n, g.ho, g.wo, g.cout), dtype=torch.bfloat16, device=x_rows.device)
    _launch("vqseg_conv2d_affine_bits_f", x_rows.device, _T(x_rows, "conv input", bf=1, numel=g.n * g.h * g.w * g.cin),
            _w16(w_hi, "packed weights", g.packed), _f32(scale, "scale", g.cout), _f32(shift, "shift", g.cout),
            _T(res, "residual", bf=1, numel=g.m * g.cout), _T(bits, "ReLU mask bits", dtype=torch.uint8, numel=g.m * g.cout // 8),
            _T(out, "conv output", bf=1, numel=g.m * g.cout), g.n, g.h, g.w, g.cin, g.cout, g.kh, g.kw, g.pad, g.ho, g.wo)
    return out


def _stem7_conv(xr, w_img, stat, coef, relu, stem: StemGeom, cout: int, s3: bool = False):
    """vqseg_stem7_conv_f -> the stem's output straight from the fp32 image rows: raw + BatchNorm partial sums (`stat`), or with the
    affine + ReLU epilogue (`coef`); s3: [hi | lo] weights and output rows."""
    n, f = xr.shape[0], 2 if s3 else 1
    m = n * stem.fused[0] * stem.fused[1]
    out = torch.empty((n, stem.fused[0], stem.fused[1], f * cout), dtype=torch.bfloat16, device=xr.device)
    scale, shift = (coef[0], coef[1]) if coef is not None else (None, None)
    _launch("vqseg_stem7_conv_f", xr.device, int(s3), _f32(xr, "image", n * stem.h * stem.w * stem.cin),
            _w16(w_img, "stem weight image", cout * f * 176), _T(out, "conv output", bf=2 if s3 else 1, numel=m * cout * f),
            _f32(stat, "BN partials", _stat_elems(m, cout) if stat is not None else None), _f32(scale, "scale", cout), _f32(shift, "shift", cout),
            int(relu), n, stem.h, stem.w, int(stem.reflect))
    return out


def _bn_finalize(stat, m, cout, gamma, beta, bn, training, dev):
    """vqseg_bn_finalize_f -> coef (4, C) f32 = scale, shift, mean, invstd: from the convolution's partial sums (`stat`; training also
    updates the running statistics and num_batches_tracked in the kernel) or, stat None, from the running statistics."""
    coef = torch.empty(4, cout, dtype=torch.float32, device=dev)
    _check_fused_bn(
        "vqseg_bn_finalize_f", dev, bn, _f32(stat, "BN partials", _stat_elems(m, cout) if stat is not None else None), m, cout,
        _f32(gamma, "bn.weight", cout), _f32(beta, "bn.bias", cout), _f32(bn.running_mean, "bn.running_mean", cout),
        _f32(bn.running_var, "bn.running_var", cout), float(bn.momentum), float(bn.eps), int(training), _f32(coef[0], "scale", cout),
        _f32(coef[1], "shift", cout), _f32(coef[2], "mean", cout), _f32(coef[3], "invstd", cout),
        _T(bn.num_batches_tracked, "bn.num_batches_tracked", dtype=torch.int64, numel=1) if training else None,
        _T(_bn_sync(bn, False), "bn sync", dtype=torch.int32) if training else None)
    return coef


def _bn_apply(y, rr, coef, m, cout, relu):
    """vqseg_bn_apply_f -> relu?(y * scale + shift [+ rr])"""
    bf = _is_bf16(y)
    out = torch.empty_like(y)
    _launch("vqseg_bn_apply_f", y.device, bf, _T(y, "conv output", bf=bf, numel=m * cout), _T(rr, "residual", bf=bf, numel=m * cout),
            _f32(coef[0], "scale", cout), _f32(coef[1], "shift", cout), m, cout, int(relu), _T(out, "BN output", bf=bf, numel=m * cout))
    return out


def _bn_apply_bits(y, rr, coef, m, cout):
    """vqseg_bn_apply_bits_f (bf16) -> relu(y * scale + shift + rr) and its ReLU mask as a bit field (1/16 of the output's bytes)"""
    out = torch.empty_like(y)
    bits = torch.empty(m * cout // 8, dtype=torch.uint8, device=y.device)
    _launch("vqseg_bn_apply_bits_f", y.device, _T(y, "conv output", bf=1, numel=m * cout), _T(rr, "residual", bf=1, numel=m * cout),
            _f32(coef[0], "scale", cout), _f32(coef[1], "shift", cout), m, cout, _T(out, "BN output", bf=1, numel=m * cout),
            _T(bits, "ReLU mask bits", dtype=torch.uint8, numel=m * cout // 8))
    return out, bits


def _bn_backward(g, out, bits, y, coef, gamma, m, cout, relu, training, sink, dgamma, dbeta, g_res, bn):
    """vqseg_bn_backward_f / vqseg_bn_backward_bits_f (`bits`: the forward's ReLU mask bit field instead of its output) -> g_y; dgamma /
    dbeta are written (sink: added to), g_res (if given) gets the residual branch's gradient.  Without a residual `out` is None: the
    ReLU mask is recomputed from y with the forward's scale / shift."""
    L = lib()
    bf = _is_bf16(y)
    g_y = torch.empty_like(y)
    nws = L.vqseg_bn_backward_workspace_floats(m, cout)
    ws = torch.empty(nws, dtype=torch.float32, device=y.device)
    if bits is not None:
        _check_fused_bn(
            "vqseg_bn_backward_bits_f", y.device, bn, _T(g, "output gradient", bf=1, numel=m * cout),
            _T(bits, "ReLU mask bits", dtype=torch.uint8, numel=m * cout // 8), _T(y, "conv output", bf=1, numel=m * cout),
            _f32(coef[2], "mean", cout), _f32(coef[3], "invstd", cout), _f32(gamma.detach(), "bn.weight", cout), m, cout, int(training),
            int(sink), _f32(ws, "BN backward workspace", nws), _f32(dgamma, "bn.weight.grad", cout), _f32(dbeta, "bn.bias.grad", cout),
            _T(g_y, "conv output gradient", bf=1, numel=m * cout), _T(g_res, "residual gradient", bf=1, numel=m * cout),
            _T(_bn_sync(bn, True), "bn sync", dtype=torch.int32))
    else:
        _check_fused_bn(
            "vqseg_bn_backward_f", y.device, bn, bf, _T(g, "output gradient", bf=bf, numel=m * cout),
            _T(out, "BN output", bf=bf, numel=m * cout), _T(y, "conv output", bf=bf, numel=m * cout), _f32(coef[2], "mean", cout),
            _f32(coef[3], "invstd", cout), _f32(gamma.detach(), "bn.weight", cout), _f32(coef[0], "scale", cout), _f32(coef[1], "shift", cout),
            m, cout, int(relu), int(training), int(sink), _f32(ws, "BN backward workspace", nws), _f32(dgamma, "bn.weight.grad", cout),
            _f32(dbeta, "bn.bias.grad", cout), _T(g_y, "conv output gradient", bf=bf, numel=m * cout),
            _T(g_res, "residual gradient", bf=bf, numel=m * cout), _T(_bn_sync(bn, True), "bn sync", dtype=torch.int32))
    return g_y


def _reflect_ring(g_y, t_hi, gp, dg: ConvGeom):
    """vqseg_reflect_ring_f: the border ring of a 3x3 / stride-1 reflect-padded layer's data gradient `dg`, evaluated as a full
    correlation and folded onto rows 1 / H-2 and columns 1 / W-2 of gp (the zero-padded data gradient) in place"""
    n, h, w, c = dg.n, dg.ho, dg.wo, dg.cout
    rbuf = torch.empty((n, 2 * (w + 2) + 2 * h, c), dtype=g_y.dtype, device=g_y.device)
    _launch("vqseg_reflect_ring_f", g_y.device, _T(g_y, "conv output gradient", bf=1, numel=n * dg.h * dg.w * dg.cin),
            _w16(t_hi, "transposed image", dg.packed), _T(rbuf, "gradient ring", bf=1, numel=rbuf.numel()),
            _T(gp, "input gradient", bf=1, numel=n * h * w * c), n, h, w, dg.cin, c)


def _reflect_fold(gp, g: ConvGeom, c: int):
    """vqseg_reflect_fold_f: gradient of the reflect-padded (pad 1) input (n, h + 2, w + 2, c) -> gradient of the input (n, h, w, c);
    zero padding: gp is that gradient already"""
    if not g.reflect:
        return gp
    if g.pad != 1:
        raise NotImplementedError("reflect-padding data gradient is implemented for pad == 1")
    bf = _is_bf16(gp)
    gx = torch.empty((g.n, g.h, g.w, c), dtype=gp.dtype, device=gp.device)
    _launch("vqseg_reflect_fold_f", gp.device, bf, _T(gp, "padded input gradient", bf=bf, numel=g.n * (g.h + 2) * (g.w + 2) * c), g.n, g.h, g.w, c,
            _T(gx, "input gradient", bf=bf, numel=g.n * g.h * g.w * c))
    return gx


def _dgrad_s2(g_y, s_hi, s_lo, acc, g: ConvGeom, c: int, gh: int, gw: int):
    """vqseg_conv2d_dgrad_s2_f: data gradient (n, gh, gw, c) of the stride-2 layer `g` by parity classes of the output pixel, written
    into a fresh tensor or accumulated into `acc` in place"""
    L = lib()
    bf = _is_bf16(g_y)
    gp = acc if acc is not None else torch.empty((g.n, gh, gw, c), dtype=g_y.dtype, device=g_y.device)
    sneed = L.vqseg_conv_packed_s2_elems(g.cout, c, g.kh)
    _launch("vqseg_conv2d_dgrad_s2_f", g_y.device, _T(g_y, "conv output gradient", bf=bf, numel=g.m * g.cout),
            _w16(s_hi, "parity-class image", sneed), _w16(s_lo, "parity-class image (lo)", sneed),
            _T(gp, "input gradient", bf=bf, numel=g.n * gh * gw * c), g.n, g.ho, g.wo, g.cout, c, g.kh, gh, gw, int(not bf), int(acc is not None))
    return gp


def _dgrad_s2_fold(g_y, s_hi, g: ConvGeom, c: int):
    """vqseg_conv2d_dgrad_s2_fold_f (bf16, 3x3 / stride 2 / pad 1): the four parity classes in ONE launch, written straight into the
    unpadded gradient (reflect padding: the padded top row / left column go to a small ring behind the pixel rows and are added onto
    row 1 / column 1) -- no (H+2) x (W+2) tensor, no fold / crop pass over it"""
    L = lib()
    rows = int(L.vqseg_conv2d_dgrad_s2_fold_rows(g.n, g.h, g.w, int(g.reflect)))
    buf = torch.empty((rows, c), dtype=g_y.dtype, device=g_y.device)
    _launch("vqseg_conv2d_dgrad_s2_fold_f", g_y.device, _T(g_y, "conv output gradient", bf=1, numel=g.m * g.cout),
            _w16(s_hi, "parity-class image", L.vqseg_conv_packed_s2_elems(g.cout, c, 3)), _T(buf, "input gradient (+ ring)", bf=1, numel=rows * c),
            g.n, g.ho, g.wo, g.cout, c, g.h, g.w, int(g.reflect))
    return buf[:g.n * g.h * g.w].view(g.n, g.h, g.w, c)


def _bn_sync(bn, backward: bool):
    """The BatchNorm module's own hand-over counters for the fused merge + finalize / reduce + finalize launches (include/vqseg.h,
    `sync`): zeros between launches, never shared by concurrent launches -- one buffer per module, one half per direction (a
    module's forwards and backwards are ordered on its network's stream).  OFF by default: measured on the bench step (r3, same
    box, alternating) the one-launch forms are 0.3-2 % SLOWER than the two-launch ones -- the last workgroup's fold is a serial
    tail read through device-coherent loads, and the launches it saves were not on the critical path (the other network's stream
    covers them).  VQSEG_OPTS=py_bn_fused=1 switches them on."""
    if not py_opt("py_bn_fused", 0):
        return None
    c = bn.num_features
    g = lib().vqseg_bn_sync_ints(c)
    buf = getattr(bn, "_vq_sync", None)
    dev = bn.weight.device
    if buf is None or buf.device != dev or buf.numel() != 2 * g:
        buf = bn._vq_sync = torch.zeros(2 * g, dtype=torch.int32, device=dev)
    return buf[g:] if backward else buf[:g]


def _check_fused_bn(name: str, dev, bn, *args) -> None:
    """`_launch` for the entry points that take a module's hand-over counters: a launch that failed midway may leave them non-zero,
    and every later fused launch on that module would then never elect a last workgroup (scale / shift / dgamma / dbeta silently
    stale).  When the launch raises, the module's counters are zeroed before the error propagates."""
    try:
        _launch(name, dev, *args)
    except _hip.HipLibraryError:
        buf = getattr(bn, "_vq_sync", None)
        if buf is not None:
            buf.zero_()
        raise


# Side streams for the weight-gradient kernels: {cuda_stream handle of a network's stream: torch.cuda.Stream}.  A trainer that owns
# the parameters' .grad storage registers one per network stream (trainer.CPSTrainer), adds it to the buckets' producer streams
# and joins it before the optimiser step.  Empty: everything stays on the calling stream.
WGRAD_SIDE_STREAMS: dict = {}


def _wgrad_side_stream(dev):
    if not WGRAD_SIDE_STREAMS:
        return None
    return WGRAD_SIDE_STREAMS.get(torch.cuda.current_stream(dev).cuda_stream)


def _out_size(h, k, s, p):
    return (h + 2 * p - k) // s + 1


# ------------------------------------------------------------------------------------------------
# Gradient sinks.  A trainer that owns the parameters' .grad storage (grad_buckets.GradBuckets: flat fp32 buckets) marks a
# parameter with `p._vq_grad_sink = callback-or-None`; the weight-gradient kernels then ADD into p.grad themselves
# (`accumulate` flag of the C entry points) and autograd gets None for that parameter -- one tiny add kernel per
# parameter and backward pass less.  The callback (if any) is told, as a post-accumulate-grad hook would be.
# ------------------------------------------------------------------------------------------------
def py_opt(key: str, default: int) -> int:
    """host-side A/B switch from VQSEG_OPTS ("py_<name>=<int>", see _hip.lib)"""
    lib()
    return _hip.PY_OPTS.get(key, default)


# Parameters with a queued first use of a two-use weight gradient (see _ConvBNAct.backward); flush_pending_wgrads() launches
# whatever is still queued (a forward whose output did not reach the loss) -- trainers call it after backward().
_PENDING_WGRADS: set = set()


def _wgrad_launch(key: _WgradKey, a, b, gw, accumulate, stream):
    """vqseg_conv2d_wgrad2_f over use `a` = (g_y, x, x2, n) [and use `b`] into gw; `stream`: the stream a queued use belongs to."""
    g, precise, stem = key
    g_y, xr, x2r, n = a
    gb, xb, x2b, nb = b if b is not None else (None, None, None, 0)
    L = lib()
    dev = g_y.device
    bf = 0 if precise else 1
    nout, nin = g.ho * g.wo * g.cout, g.h * g.w
    with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
        if stem is not None:                                 # x is the stem's patch matrix: the gradient of the 7x7 weight itself
            okh, okw, wkh, wkw = stem.kh, stem.kw, 1, 1
            im2col, cin_out, st_, pd_, rf_ = 1, stem.cin, 1, 0, 0
        else:
            okh, okw, wkh, wkw = g.kh, g.kw, g.kh, g.kw
            im2col, cin_out, st_, pd_, rf_ = 0, g.cin, g.stride, g.pad, int(g.reflect)
        nbytes = L.vqseg_conv2d_wgrad_workspace_bytes(n + nb, g.h, g.w, g.cin, g.ho, g.wo, g.cout, wkh, wkw)
        wsw = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _launch("vqseg_conv2d_wgrad2_f", dev, _T(g_y, "conv output gradient", bf=bf, numel=n * nout),
                _T(xr, "conv input", bf=bf, numel=n * nin * g.c1), _T(x2r, "conv input 2", bf=bf, numel=n * nin * (g.cin - g.c1)), n,
                _T(gb, "conv output gradient (second use)", bf=bf, numel=nb * nout), _T(xb, "conv input (second use)", bf=bf, numel=nb * nin * g.c1),
                _T(x2b, "conv input 2 (second use)", bf=bf, numel=nb * nin * (g.cin - g.c1)), nb, g.c1, g.h, g.w, g.cin, g.ho, g.wo, g.cout, okh, okw,
                st_, pd_, rf_, int(precise), cin_out, im2col, int(accumulate), _T(wsw, "wgrad workspace", dtype=torch.uint8, numel=nbytes), nbytes,
                _f32(gw, "weight gradient", g.cout * cin_out * okh * okw))


def flush_pending_wgrads() -> int:
    """Launch every queued first use that never met its second (returns how many).  After this no Parameter holds activations."""
    n = 0
    for p in list(_PENDING_WGRADS):
        pend = getattr(p, "_vq_wgrad_pending", None)
        p._vq_wgrad_pending = None
        if pend is not None:
            _wgrad_launch(pend[0], pend[1], None, p.grad, True, pend[2])
            n += 1
    _PENDING_WGRADS.clear()
    return n


def drop_pending_wgrads() -> None:
    """forget queued uses without launching them (start of a step: whatever an aborted backward left behind)"""
    for p in list(_PENDING_WGRADS):
        p._vq_wgrad_pending = None
    _PENDING_WGRADS.clear()


class GradLink:
    """Carries the gradient of a block's identity branch from the backward of its LAST conv (`link_out`: where the
    residual add happened) to the backward of its FIRST conv (`link_in`), whose data-gradient kernel adds it in its
    epilogue -- instead of autograd materialising both gradients of the block input and adding them in a separate
    pass.  Valid when both convolutions read the same tensor (identity shortcut).
    Projection shortcut: the shortcut's convolution sends the gradient of ITS input (`link_x`) the same way.  Its backward
    has no dependency on the first conv's, so the order is the autograd engine's choice: a producer that arrives after the
    consumer has run (`closed`) simply returns its gradient to autograd."""
    __slots__ = ("g", "closed", "leftover", "bits", "takes_bits", "__weakref__")

    def __init__(self):
        self.g = None
        self.closed = False
        self.leftover = None
        self.bits = None            # `g` is the block output's UNMASKED gradient, `bits` the ReLU mask of the block's last BatchNorm
        self.takes_bits = False     # set by the first conv's forward: its data-gradient epilogue can apply `bits` itself


def _mask_with_bits(g, bits):
    """g .* bits (bit i % 8 of byte i / 8 over the flat index) with stock operators -- the fallback of a bit-field shortcut gradient
    whose consumer turned out not to fuse it"""
    sh = torch.arange(8, device=g.device, dtype=torch.uint8)
    keep = torch.bitwise_and(torch.bitwise_right_shift(bits.view(-1, 1), sh), 1).view(g.shape).to(torch.bool)
    return torch.where(keep, g, torch.zeros((), dtype=g.dtype, device=g.device))


# ------------------------------------------------------------------------------------------------
# Fan-in fusion.  A tensor with TWO consumers (an encoder feature feeds the next encoder stage AND the decoder / its VQ layer;
# the decoder output feeds the head AND the prototype loss) gets two gradients that autograd adds in a separate pass over the
# tensor (5 such adds per backward pass, ~2 ms per training step).  With fusion on, the producer of the tensor tags it with a
# GradLink (`t._vq_fanin`); the consumer whose backward runs FIRST deposits its gradient there (and returns nothing to autograd),
# the one that runs LAST adds it inside its own kernel: the stride-2 1x1 projection's data gradient accumulates in place
# (vqseg_conv2d_dgrad_s2_f accumulate), the max-pool and head backward kernels take an addend.  Results are bit-identical to
# autograd's add.  Order is a data dependency for the encoder features (the decoder's backward is upstream of the encoder's) and
# the engine's priority order for the decoder output; a depositor that comes after the absorber (`closed`) returns its gradient
# to autograd as usual.  A deposit that nobody absorbs would be a lost gradient: only callers that check for it after backward
# (trainer.CPSTrainer: check_fanin_consumed) switch the fusion on.
# ------------------------------------------------------------------------------------------------
_FANIN_ON = False
_FANIN_OPEN: set = set()                                  # links holding a deposited, not yet absorbed gradient


def set_fanin_fusion(on: bool) -> bool:
    global _FANIN_ON
    prev = _FANIN_ON
    _FANIN_ON = bool(on) and py_opt("py_fanin", 1) == 1
    return prev


def fanin_tag(t):
    """producer side: mark `t` (a tensor with two consumers) for fan-in fusion in the coming backward"""
    if _FANIN_ON and torch.is_tensor(t) and t.requires_grad and torch.is_grad_enabled():
        t._vq_fanin = GradLink()
    return t


def _fanin_of(t):
    return getattr(t, "_vq_fanin", None) if (_FANIN_ON and torch.is_tensor(t)) else None


def _fanin_deposit(link, g_rows) -> bool:
    """first consumer: hand the gradient (NHWC rows) to the link; False: the absorber has already run"""
    if link is None or link.closed or link.g is not None:
        return False
    link.g = g_rows
    _FANIN_OPEN.add(link)
    return True


def _fanin_take(link, shape, dtype):
    """last consumer: the deposited gradient if it fits (shape, dtype, dense), else None; either way the link is closed.
    A deposit that does not fit is returned through `link.leftover` for a plain add."""
    if link is None:
        return None
    link.closed = True
    g, link.g = link.g, None
    _FANIN_OPEN.discard(link)
    if g is None:
        return None
    if tuple(g.shape) == tuple(shape) and g.dtype == dtype and g.is_contiguous():
        return g
    link.leftover = g
    return None


def check_fanin_consumed() -> None:
    """after backward: every deposited gradient must have been absorbed (else it never reached its tensor)"""
    if _FANIN_OPEN:
        n = len(_FANIN_OPEN)
        for l_ in list(_FANIN_OPEN):
            l_.g = None
        _FANIN_OPEN.clear()
        raise RuntimeError(f"fan-in fusion: {n} deposited gradient(s) were never absorbed -- a consumer's backward did not run; "
                           f"switch the fusion off (VQSEG_OPTS=py_fanin=0) for graphs that use only part of the model's outputs")


_UNIT_AFFINE = {}


def _unit_affine(dev, c):
    key = (str(dev), c)
    if key not in _UNIT_AFFINE:
        _UNIT_AFFINE[key] = (torch.ones(c, dtype=torch.float32, device=dev), torch.zeros(c, dtype=torch.float32, device=dev))
        torch.cuda.current_stream(dev).synchronize()       # once per (device, width): other streams may read them next
    return _UNIT_AFFINE[key]


def _sink_ready(p) -> bool:
    g = getattr(p, "grad", None)
    return hasattr(p, "_vq_grad_sink") and g is not None and g.dtype == torch.float32 and g.is_contiguous() and g.is_cuda


def _sink_use(*params) -> None:
    """forward (called where the grad mode is still visible): one more gradient contribution will arrive for each
    of these parameters in the coming backward"""
    if torch.is_grad_enabled():
        for p in params:
            if p.requires_grad and hasattr(p, "_vq_grad_sink"):
                p._vq_uses = getattr(p, "_vq_uses", 0) + 1


def _sink_done(p) -> None:
    """backward: one contribution has been added into p.grad; the callback fires with the last one"""
    p._vq_uses = getattr(p, "_vq_uses", 1) - 1
    cb = p._vq_grad_sink
    if cb is not None and p._vq_uses <= 0:
        cb(p)


# ------------------------------------------------------------------------------------------------
# "Split-3" activations: the fp32-precision no-grad eval forward on the bf16 kernels (include/vqseg.h, "Split-3").
# The reference trainers run their two pseudo-label forwards in fp32, OUTSIDE autocast (train_vqreptunet1x1v2.py:143-149).
# The "precise" kernels do that with on-the-fly bf16 hi/lo splits inside a register-staged kernel; here the SAME three products
# run on the LDS-DMA / patch-reuse bf16 kernels by keeping every activation of such a forward as [hi | lo] bf16 (the
# convolution's K loop runs over [hi | lo | hi], reading hi twice, against weights [w_hi | w_hi | w_lo]).
# An `S3` object stands in for the logical (N, C, H, W) fp32 tensor between the layers of ONE model forward; it never leaves
# the model (the model's `encode` opens the scope, the 1x1 head / the VQ layers merge back to fp32).
# ------------------------------------------------------------------------------------------------
class S3:
    """rows: (N, H, W, 2C) bf16 contiguous = [hi | lo] of the logical fp32 tensor (N, C, H, W)."""
    __slots__ = ("rows", "c")

    def __init__(self, rows: torch.Tensor, c: int):
        self.rows, self.c = rows, c

    @property
    def shape(self):
        n, h, w, _ = self.rows.shape
        return torch.Size((n, self.c, h, w))

    dtype = torch.float32                                    # what the tensor logically is
    is_cuda = True
    requires_grad = False

    @property
    def device(self):
        return self.rows.device

    def float(self) -> torch.Tensor:
        """merge back: logical (N, C, H, W) fp32 tensor (channels_last in memory)"""
        n, h, w, _ = self.rows.shape
        out = torch.empty((n, h, w, self.c), dtype=torch.float32, device=self.rows.device)
        _launch("vqseg_s3_merge_f", out.device, _T(self.rows, "split-3 rows", bf=2, numel=n * h * w * 2 * self.c), n * h * w, self.c,
                _f32(out, "merged rows", n * h * w * self.c))
        return _nchw(out)


_S3_SCOPE = False


class s3_scope:
    """Inside this scope a no-grad, eval-mode, fp32 (not autocast) stem starts a split-3 forward (opened by the VQ-UNet's own
    `encode`; a bare `model.encoder(x)` call therefore keeps returning plain fp32 tensors).  VQSEG_OPTS=py_s3_eval=0 disables."""

    def __init__(self, enabled: bool = True):
        self.enabled = bool(enabled) and py_opt("py_s3_eval", 1) == 1

    def __enter__(self):
        global _S3_SCOPE
        self.prev = _S3_SCOPE
        _S3_SCOPE = self.enabled
        return self

    def __exit__(self, *exc):
        global _S3_SCOPE
        _S3_SCOPE = self.prev
        return False


def to_s3(x) -> "S3":
    """logical (N, C, H, W) fp32 (or bf16) tensor -> split-3"""
    if isinstance(x, S3):
        return x
    xr = _rows(x.float())
    n, h, w, c = xr.shape
    out = torch.empty((n, h, w, 2 * c), dtype=torch.bfloat16, device=xr.device)
    _launch("vqseg_s3_split_f", xr.device, _f32(xr, "rows", n * h * w * c), n * h * w, c, _T(out, "split-3 rows", bf=2, numel=n * h * w * 2 * c))
    return S3(out, c)


def s3_from_rows(rows: torch.Tensor, c: int) -> "S3":
    """the split-3 tensor a kernel wrote as rows (N, H, W, 2C) bf16 = [hi | lo] (the VQ layers' quantised features)"""
    if rows.dim() != 4 or rows.dtype != torch.bfloat16 or rows.shape[-1] != 2 * c or not rows.is_contiguous():
        raise ValueError(f"split-3 rows must be contiguous (N, H, W, {2 * c}) bf16, got {tuple(rows.shape)} {rows.dtype}")
    return S3(rows, c)


def from_s3(x):
    return x.float() if isinstance(x, S3) else x


def _s3_weights(weight: torch.Tensor, c1: int, as_1x1_cols: int = 0) -> torch.Tensor:
    """[w_hi | w_hi | w_lo] image per concat segment (vqseg_conv_pack_weights_s3_f32), cached on the Parameter."""
    if not as_1x1_cols:
        img = _pack_all(weight, ("s3", c1))
        if img is not None:
            return img
    cache = _cache_of(weight)
    k = ("s3", c1, as_1x1_cols)
    if k not in cache:
        w = weight.detach()
        if as_1x1_cols:                                      # the stem: [64][3][7][7] as a 1x1 convolution over kp patch columns
            cout, cin, kh, kw = w.shape
            w2 = torch.zeros(cout, as_1x1_cols, 1, 1, dtype=torch.float32, device=w.device)
            w2[:, :kh * kw * cin, 0, 0] = w.permute(0, 2, 3, 1).reshape(cout, kh * kw * cin)
            w = w2
        w = w if w.is_contiguous() else w.contiguous()
        cout, cin, kh, kw = w.shape
        out = torch.empty(cout * kh * kw * 3 * cin, dtype=torch.int16, device=w.device)
        _launch("vqseg_conv_pack_weights_s3_f32", w.device, _f32(w, "weight", cout * cin * kh * kw), cout, cin, c1, kh, kw,
                _w16(out, "split-3 image", cout * kh * kw * 3 * cin))
        cache[k] = out
    return cache[k]


def _conv_bn_act_s3(x: "S3", x2, residual, conv, bn, relu, kernel_1x1_cols: int = 0) -> "S3":
    """eval-mode Conv -> BN -> [+ residual] -> [ReLU] on split-3 tensors: the convolution's fused epilogue (precise = 2)."""
    n, h, w, _ = x.rows.shape
    c1 = x.c
    x2s = to_s3(x2) if x2 is not None else None
    cin = c1 + (x2s.c if x2s is not None else 0)
    cout = conv.weight.shape[0]
    if kernel_1x1_cols:
        kh = kw = 1
        stride, pad, reflect = 1, 0, False
    else:
        kh, kw = conv.weight.shape[2], conv.weight.shape[3]
        stride, pad = conv.stride[0], conv.padding[0]
        reflect = conv.padding_mode == "reflect" and pad > 0
    g = ConvGeom(n, h, w, c1, cin, cout, kh, kw, stride, pad, reflect, _out_size(h, kh, stride, pad), _out_size(w, kw, stride, pad))
    wimg = _s3_weights(conv.weight, c1, kernel_1x1_cols)
    res = to_s3(residual) if residual is not None else None
    coef = _bn_finalize(None, g.m, cout, bn.weight, bn.bias, bn, False, x.rows.device)
    out = _conv_affine(x.rows, x2s.rows if x2s is not None else None, wimg, None, coef[0], coef[1], res.rows if res is not None else None,
                       relu, g, 2)
    return S3(out, cout)


# ------------------------------------------------------------------------------------------------
# Conv (no bias) -> BatchNorm -> [+ residual] -> [ReLU], optional channel concat of two inputs
# ------------------------------------------------------------------------------------------------
def _residual_rows(residual, dtype):
    rr = _rows(residual) if residual is not None else None
    if rr is not None and rr.dtype != dtype:
        raise _hip.HipLibraryError("residual dtype differs from the activation dtype")
    return rr


def _forward_eval(xr, x2r, residual, w_hi, w_lo, gamma, beta, bn, relu, g: ConvGeom, bf, stem):
    """eval-mode BatchNorm is a fixed per-channel affine map: it rides in the convolution's epilogue together with the residual add
    and the ReLU (the no-grad pseudo-label passes; nothing is kept for a backward)"""
    rr = _residual_rows(residual, xr.dtype)
    coef = _bn_finalize(None, g.m, g.cout, gamma, beta, bn, False, xr.device)
    if stem is not None and stem.is_fused:
        return _stem7_conv(xr, w_hi, None, coef, relu, stem, g.cout)
    return _conv_affine(xr, x2r, w_hi, w_lo, coef[0], coef[1], rr, relu, g, int(not bf))


class _ConvBNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, x2, residual, weight, gamma, beta, bn, stride, pad, reflect, relu, stem, fuse_eval=False,
                link_in=None, link_out=None, link_x=None, fan_x=None, fan_x2=None):
        """x (N,C1,H,W) [+ x2 (N,C2,H,W)] -> out (N,Cout,Ho,Wo).  `stem` (a StemGeom): x is the stem's im2col patch matrix and the
        convolution itself 1x1 -- or, `stem.is_fused`, x is the fp32 IMAGE: the convolution gathers its operands from it
        (vqseg_stem7_conv_f, bit-identical to the 1x1 convolution over the patch matrix), the activations are bf16, and backward
        builds the patch matrix for the weight gradient (shared between the two networks like the forward's)."""
        xr = _rows(x)
        x2r = _rows(x2) if x2 is not None else None
        bf = _is_bf16(xr)
        n, h, w, c1 = xr.shape
        fused = stem is not None and stem.is_fused
        stem_x = None
        if fused:
            stem_x, _STEM_X_ARG[0] = _STEM_X_ARG[0], None
            (h, w, c1), bf = stem.fused, 1
        cin = c1 + (x2r.shape[3] if x2r is not None else 0)
        cout = weight.shape[0]
        kh, kw = (1, 1) if stem is not None else (weight.shape[2], weight.shape[3])
        g = ConvGeom(n, h, w, c1, cin, cout, kh, kw, stride, pad, bool(reflect), _out_size(h, kh, stride, pad), _out_size(w, kw, stride, pad))
        training = bool(bn.training)
        if fused:
            w_hi, w_lo = _stem_weights_fused(weight, False), None
        elif stem is not None:
            w_hi, w_lo = _stem_weights(weight, not bf, cin)
        else:
            w_hi, w_lo = packed_weights(weight, not bf, False)
        if bn.momentum is None:
            raise NotImplementedError("BatchNorm2d(momentum=None) (cumulative average) is not used by the path")
        if fuse_eval and not training:
            return _nchw(_forward_eval(xr, x2r, residual, w_hi, w_lo, gamma, beta, bn, relu, g, bf, stem))
        stat = torch.empty(_stat_elems(g.m, cout), dtype=torch.float32, device=xr.device) if training else None
        y = _stem7_conv(xr, w_hi, stat, None, False, stem, cout) if fused else _conv_raw(xr, x2r, w_hi, w_lo, stat, g)
        coef = _bn_finalize(stat, g.m, cout, gamma, beta, bn, training, xr.device)          # scale, shift, mean, invstd
        rr = _residual_rows(residual, y.dtype)
        # residual layers in bf16: the ReLU mask goes to the backward as a bit field (1/16 of `out`'s bytes), see vqseg.h
        if rr is not None and relu and bf and cout % 8 == 0 and training and any(ctx.needs_input_grad) and py_opt("py_bn_bits", 1):
            out, bits = _bn_apply_bits(y, rr, coef, g.m, cout)
        else:
            out, bits = _bn_apply(y, rr, coef, g.m, cout, relu), None
        ctx.mask_bits = bits is not None
        if link_in is not None:                                             # see _dgrad_shortcut: the zero-padded stride-1 data gradient + shortcut
            link_in.takes_bits = bool(bf and x2r is None and stride == 1 and not reflect and cin % 8 == 0 and py_opt("py_gres_bits", 1))
        ctx.save_for_backward(xr, x2r, y, bits if bits is not None else out, coef, weight, gamma)
        ctx.stem_x = stem_x                                                 # the image tensor OBJECT the patch matrix is shared under
        ctx.params = (weight, gamma, beta)                                  # the Parameter objects (see grad sinks)
        ctx.bn = bn
        ctx.links = (link_in, link_out, link_x)
        ctx.fans = (fan_x, fan_x2)                                          # fan-in links: absorb into x's gradient / deposit x2's
        ctx.geom, ctx.stem = g, stem
        ctx.relu, ctx.training, ctx.has_res = bool(relu), training, residual is not None
        return _nchw(out)

    @staticmethod
    def backward(ctx, g_out):
        xr, x2r, y, out, coef, weight, gamma = ctx.saved_tensors
        g, stem = ctx.geom, ctx.stem
        if stem is not None and stem.is_fused:                              # forward ran from the image: the weight gradient's patch matrix now
            img = xr
            xr = _shared_stem_patches(ctx.stem_x if ctx.stem_x is not None else img,
                                      (torch.bfloat16, stem.kh, stem.kw, stem.stride, stem.pad, stem.reflect),
                                      lambda: _stem_patches(img, torch.bfloat16, stem.kh, stem.kw, stem.stride, stem.pad, stem.reflect, g.ho, g.wo, g.cin))
        g_y, g_res, dgamma, dbeta = _bn_backward_step(ctx, g_out, y, out, coef, gamma)
        gw = _wgrad_step(ctx, g_y, xr, x2r, weight)
        gx = gx2 = None
        if (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]) and stem is None:
            gx, gx2 = _dgrad_step(ctx, g_y, x2r, weight)
        g_res_out = _nchw(g_res) if (ctx.has_res and ctx.links[1] is None) else None
        # one entry per argument of forward (after ctx): the six tensors above, None for the rest
        return (gx, gx2, g_res_out, gw, dgamma, dbeta) + (None,) * (_ConvBNAct.forward.__code__.co_argcount - 7)


def _bn_backward_step(ctx, g_out, y, out, coef, gamma):
    """BatchNorm (+ ReLU, + residual split) backward -> (g_y, g_res, dgamma, dbeta); with grad sinks dgamma / dbeta are added into the
    parameters' .grad and come back None.  A block's last conv hands the residual branch's gradient to `link_out` (GradLink)."""
    g = ctx.geom
    gr = _rows(g_out)
    if gr.dtype != y.dtype:
        gr = gr.to(y.dtype)
    link_out = ctx.links[1]
    # the residual branch's gradient g_out .* mask is not stored when the block's first conv will apply the mask bits itself
    bits_to_link = bool(ctx.has_res and ctx.mask_bits and link_out is not None and link_out.takes_bits and not link_out.closed)
    g_res = torch.empty_like(y) if (ctx.has_res and not bits_to_link) else None
    _, p_g, p_b = ctx.params
    sink = _sink_ready(p_g) and _sink_ready(p_b) and ctx.needs_input_grad[4] and ctx.needs_input_grad[5]
    dgb = None if sink else torch.empty(2, g.cout, dtype=torch.float32, device=y.device)
    dgamma, dbeta = (p_g.grad, p_b.grad) if sink else (dgb[0], dgb[1])
    g_y = _bn_backward(gr, out if (ctx.has_res and not ctx.mask_bits) else None, out if ctx.mask_bits else None, y, coef, gamma,
                       g.m, g.cout, ctx.relu, ctx.training, sink, dgamma, dbeta, g_res, ctx.bn)
    if sink:
        _sink_done(p_g), _sink_done(p_b)
    if link_out is not None and ctx.has_res:
        link_out.g = gr if bits_to_link else g_res                          # picked up by the block's first conv
        link_out.bits = out if bits_to_link else None
    return (g_y, g_res, None, None) if sink else (g_y, g_res, dgb[0], dgb[1])


def _wgrad_step(ctx, g_y, xr, x2r, weight):
    """Weight gradient -> gw (None with a grad sink: the result is ADDED into the trainer's bucket, nothing returns to autograd).
    With a sink and a registered side stream the kernel and its slab sum leave the network's stream: nothing downstream in backward
    depends on them, and as filler work they cover the latency-bound links of the main chain (BatchNorm statistics folds,
    finalizes, packs: skipping those ~950 launches -- wrong results, timing only -- was worth 11 ms of a 163 ms step)."""
    g, dev = ctx.geom, g_y.device
    p_w = ctx.params[0]
    sink_w = _sink_ready(p_w) and ctx.needs_input_grad[3]
    gw = p_w.grad if sink_w else torch.empty(weight.shape, dtype=torch.float32, device=dev)
    wside = _wgrad_side_stream(dev) if sink_w else None
    if wside is not None:
        main_s = torch.cuda.current_stream(dev)
        wside.wait_event(main_s.record_event())                             # g_y (BatchNorm backward) is complete
        for t_ in (g_y, xr, x2r):
            if t_ is not None:
                t_.record_stream(wside)                                     # allocator: not reusable before the side stream is done
    key = _WgradKey(g._replace(n=0), not _is_bf16(g_y), ctx.stem)
    use = (g_y, xr, x2r, g.n)
    # two-use weights: a weight used by two training forwards of the step (the labelled and the unlabelled batch of a CPS iteration)
    # gets ONE launch over both uses -- the first use is queued on the Parameter, the second runs vqseg_conv2d_wgrad2_f over the
    # virtual batch: twice the contraction length per workgroup, half the slab sums
    pend = getattr(p_w, "_vq_wgrad_pending", None) if sink_w else None
    if pend is not None:
        p_w._vq_wgrad_pending = None
        _PENDING_WGRADS.discard(p_w)
    if pend is not None and (pend[0] != key or pend[2] != torch.cuda.current_stream(dev) or wside is not None):
        _wgrad_launch(pend[0], pend[1], None, p_w.grad, True, pend[2])      # not pairable after all: the queued use on its own
        pend = None
    if sink_w and pend is None and wside is None and getattr(p_w, "_vq_uses", 1) >= 2 and py_opt("py_wgrad_pair", 1):
        p_w._vq_wgrad_pending = (key, use, torch.cuda.current_stream(dev))
        _PENDING_WGRADS.add(p_w)
    else:
        with (torch.cuda.stream(wside) if wside is not None else contextlib.nullcontext()):
            _wgrad_launch(key, pend[1] if pend is not None else use, use if pend is not None else None, gw, sink_w, None)
    if sink_w:
        _sink_done(p_w)
    return None if sink_w else gw


# What the data-gradient paths of one backward share: g the forward convolution, single: one input (no channel concat), t_hi / t_lo the
# [Cin][kh][kw][Cout] tap-flipped weight image (the same implicit-GEMM kernels run on g_y with it), fan_x the input's fan-in link
_Dgrad = namedtuple("_Dgrad", "g g_y bf single weight t_hi t_lo fan_x")


def _dgrad_geom(g: ConvGeom, c_cnt, hp, wp, pad) -> ConvGeom:
    """the stride-1 convolution g_y (n, ho, wo, cout) -> gradient (n, hp, wp, c_cnt) of (a channel range of) g's input"""
    return ConvGeom(g.n, g.ho, g.wo, g.cout, g.cout, c_cnt, g.kh, g.kw, 1, pad, False, hp, wp)


# Every path(d, c_lo, c_cnt, extra, ebits) -> (gradient rows of input channels [c_lo, c_lo + c_cnt), extra), or None where it does not
# apply (its first statement).  `extra` is the shortcut gradient of the same block input (GradLink), `ebits` its ReLU mask bit field;
# a path that adds `extra` in its kernel returns None for it.
def _dgrad_ring(d, c_lo, c_cnt, extra, ebits):
    """reflect padding, 3x3 / stride 1 (every Bottleneck conv2): the padded gradient's INTERIOR is the zero-padded data gradient (fast
    patch kernel, unpadded grid); only its border ring is evaluated as a full correlation and folded onto it (_reflect_ring) -- no
    (H+2) x (W+2) tensor, no fold pass over it"""
    g = d.g
    if not (g.reflect and g.stride == 1 and (g.kh, g.kw, g.pad) == (3, 3, 1) and d.bf and d.single and g.cout % 64 == 0
            and c_cnt % 8 == 0 and g.h >= 4 and g.w >= 4 and py_opt("py_reflect_ring", 1) == 1):
        return None
    dg = _dgrad_geom(g, c_cnt, g.h, g.w, 1)
    if extra is not None and extra.shape == (g.n, g.h, g.w, c_cnt):
        one, zero = _unit_affine(d.g_y.device, c_cnt)
        gp, extra = _conv_affine(d.g_y, None, d.t_hi, None, one, zero, extra, False, dg, 0), None
    else:
        gp = _conv_raw(d.g_y, None, d.t_hi, d.t_lo, None, dg)
    _reflect_ring(d.g_y, d.t_hi, gp, dg)
    return gp, extra


def _shortcut_ok(d, c_cnt, extra):
    g = d.g
    return extra is not None and not g.reflect and g.stride == 1 and d.single and extra.shape == (g.n, g.h, g.w, c_cnt)


def _dgrad_shortcut(d, c_lo, c_cnt, extra, ebits):
    """the data gradient and the residual-branch gradient meet in the convolution's epilogue (one add pass less); with `ebits` the
    epilogue also applies the block's last ReLU mask to the shortcut gradient"""
    if not _shortcut_ok(d, c_cnt, extra):
        return None
    g = d.g
    dg = _dgrad_geom(g, c_cnt, g.h, g.w, g.kh - 1 - g.pad)
    one, zero = _unit_affine(d.g_y.device, c_cnt)
    if ebits is not None:
        return _conv_affine_bits(d.g_y, d.t_hi, one, zero, extra, ebits, dg), None
    return _conv_affine(d.g_y, None, d.t_hi, d.t_lo, one, zero, extra, False, dg, int(not d.bf)), None


def _dgrad_s2_folded(d, c_lo, c_cnt, extra, ebits):
    g = d.g
    if not (g.stride == 2 and d.single and (g.kh, g.kw, g.pad) == (3, 3, 1) and d.bf and g.h == 2 * g.ho and g.w == 2 * g.wo and g.h >= 4
            and g.w >= 4 and g.cout % 64 == 0 and c_cnt % 8 == 0 and c_cnt >= 64 and py_opt("py_dgrad_s2", 1) and py_opt("py_dgrad_s2_fold", 1)):
        return None
    s_hi, _s_lo = _s2_weights(d.weight, not d.bf)
    return _dgrad_s2_fold(d.g_y, s_hi, d.g, c_cnt), extra


def _dgrad_s2_classes(d, c_lo, c_cnt, extra, ebits):
    """stride-2 layer: parity classes of the output pixel instead of a dilated gradient grid"""
    g = d.g
    if not (g.stride == 2 and d.single and g.kh == g.kw and ((g.kh == 1 and g.pad == 0) or (g.kh == 3 and g.pad == 1)) and py_opt("py_dgrad_s2", 1)):
        return None
    s_hi, s_lo = _s2_weights(d.weight, not d.bf)
    gh, gw = (g.h + 2, g.w + 2) if g.kh == 3 else (g.h, g.w)         # k = 3: the padded input's grid
    # fan-in (1x1 projection of a stage's first block): the input's OTHER consumer (decoder skip / VQ layer) has deposited its
    # gradient; this data gradient accumulates into it in place -- no memset, no add pass
    acc = _fanin_take(d.fan_x, (g.n, gh, gw, c_cnt), d.g_y.dtype) if (g.kh == 1 and c_cnt <= 4096) else None
    gp = _dgrad_s2(d.g_y, s_hi, s_lo, acc, g, c_cnt, gh, gw)
    if g.kh == 3 and not g.reflect:                                  # zero padding: the gradient of the padded border is dropped
        return gp[:, 1:g.h + 1, 1:g.w + 1, :].contiguous(), extra
    return _reflect_fold(gp, g, c_cnt), extra


def _dgrad_generic(d, c_lo, c_cnt, extra, ebits):
    g = d.g
    hp, wp = (g.h + 2 * g.pad, g.w + 2 * g.pad) if g.reflect else (g.h, g.w)      # reflect: gradient of the padded input first
    dg = _dgrad_geom(g, c_cnt, hp, wp, (g.kh - 1) if g.reflect else (g.kh - 1 - g.pad))
    gp = _conv_raw(d.g_y, None, d.t_hi, d.t_lo, None, dg, up=g.stride, w_offset_elems=_packed_elems(c_lo, g.kh, g.kw, g.cout))
    return _reflect_fold(gp, g, c_cnt), extra


def _dgrad(d, c_lo, c_cnt, extra, ebits):
    """the first path that applies, in this order"""
    for path in (_dgrad_ring, _dgrad_shortcut, _dgrad_s2_folded, _dgrad_s2_classes, _dgrad_generic):
        res = path(d, c_lo, c_cnt, extra, ebits)
        if res is not None:
            return res


def _dgrad_step(ctx, g_y, x2r, weight):
    """Data gradients -> (gx, gx2), either None when not needed or handed over through a GradLink / fan-in link instead."""
    g = ctx.geom
    link_in, _, link_x = ctx.links
    fan_x, fan_x2 = ctx.fans
    bf = _is_bf16(g_y)
    d = _Dgrad(g, g_y, bf, x2r is None, weight, *packed_weights(weight, not bf, True), fan_x)
    extra = ebits = None                                            # residual-branch gradient of the same block input
    if link_in is not None:
        extra, ebits = link_in.g, link_in.bits
        link_in.g = link_in.bits = None
        link_in.closed = True
    if ebits is not None and not (bf and _shortcut_ok(d, g.c1, extra)):
        extra, ebits = _mask_with_bits(extra, ebits), None          # not the fusing path after all
    gx = gx2 = None
    if ctx.needs_input_grad[0]:
        g1, extra = _dgrad(d, 0, g.c1, extra, ebits)
        if extra is not None:                                       # link not fusable here: plain add
            g1 = g1 + extra
        if fan_x is not None:                                       # a deposit the kernel path above could not absorb
            rest = _fanin_take(fan_x, g1.shape, g1.dtype)
            rest = rest if rest is not None else fan_x.leftover
            fan_x.leftover = None
            if rest is not None:
                g1 = g1 + rest.reshape(g1.shape).to(g1.dtype)
        if link_x is not None and not link_x.closed and x2r is None:
            link_x.g = g1                                           # the block's first conv adds it (GradLink)
        else:
            gx = _nchw(g1)
    if ctx.needs_input_grad[1] and x2r is not None:
        g2, _ = _dgrad(d, g.c1, g.cin - g.c1, None, None)
        if not (g2.dtype == x2r.dtype and _fanin_deposit(fan_x2, g2)):     # else x2's other consumer adds it inside its own kernel
            gx2 = _nchw(g2)
    return gx, gx2


def _s2_weights(weight, precise):
    """parity-class sub-images of a stride-2 layer's weight for its data gradient (vqseg_conv_pack_weights_s2_f32)"""
    cache = _cache_of(weight)
    k = ("s2", precise)
    if k not in cache:
        w = weight.detach()
        w = w if w.is_contiguous() else w.contiguous()
        cout, cin, kh, _kw = w.shape
        nel = lib().vqseg_conv_packed_s2_elems(cout, cin, kh)
        hi = torch.empty(nel, dtype=torch.int16, device=w.device)
        lo = torch.empty(nel, dtype=torch.int16, device=w.device) if precise else None
        _launch("vqseg_conv_pack_weights_s2_f32", w.device, _f32(w, "weight", cout * cin * kh * kh), cout, cin, kh,
                _w16(hi, "parity-class image", nel), _w16(lo, "parity-class image (lo)", nel))
        cache[k] = (hi, lo)
    return cache[k]


def _stem_weights(weight, precise, kp):
    """[64][3][7][7] -> packed [64][kp] rows ((kh, kw, ci) columns, zero padded to kp)."""
    cache = _cache_of(weight)
    k = ("stem", precise, kp)
    if k not in cache:
        # view the [Cout][Cin][KH][KW] stem weight as a 1x1 convolution over kp = pad32(KH*KW*Cin) patch columns
        cout, cin, kh, kw = weight.shape
        w2 = torch.zeros(cout, kp, 1, 1, dtype=torch.float32, device=weight.device)
        w2[:, :kh * kw * cin, 0, 0] = weight.detach().permute(0, 2, 3, 1).reshape(cout, kh * kw * cin)
        cache[k] = packed_weights(w2, precise, False)
        cache[("stem_keepalive", precise, kp)] = w2
    return cache[k]


def conv_bn_act(x, conv, bn, training=None, relu=True, residual=None, x2=None, link_in=None, link_out=None, link_x=None, absorb_fanin=False):
    """Conv2d (no bias; zero or reflect padding) -> BatchNorm2d -> [+ residual] -> [ReLU] on the HIP kernels.
    `x2`: second input whose channels follow x's (the decoder's concat).  `training` is ignored: the
    BatchNorm module's own mode decides (nn.BatchNorm2d semantics)."""
    if conv.bias is not None:
        raise NotImplementedError("conv_bn_act: the reference's fused blocks have no conv bias")
    if isinstance(x, S3) or isinstance(x2, S3) or isinstance(residual, S3):
        # the split-3 kernels take 32-channel K chunks per concat segment and 16-byte [hi | lo] output rows (vqseg_conv2d_affine_f,
        # precise == 2); any other width (e.g. decoder_channels ending in 16) merges back to fp32 and runs on the precise kernels,
        # which handle every Cin % 4 == 0 -- same values to 2^-16, just slower
        c1 = x.shape[1]
        c2 = x2.shape[1] if x2 is not None else 0
        s3_ok = c1 % 32 == 0 and c2 % 32 == 0 and conv.weight.shape[0] % 8 == 0
        if not bn.training and not torch.is_grad_enabled() and s3_ok:
            return _conv_bn_act_s3(to_s3(x), x2, residual, conv, bn, relu)
        x, x2, residual = from_s3(x), (from_s3(x2) if x2 is not None else None), (from_s3(residual) if residual is not None else None)
    if not x.is_cuda:
        raise _hip.HipLibraryError(f"the HIP path needs 'cuda' (ROCm) tensors, got {x.device}; there is no CPU fallback")
    pad = conv.padding[0]
    _sink_use(conv.weight, bn.weight, bn.bias)
    # fan-in links (see set_fanin_fusion): `absorb_fanin` -- this convolution's data gradient takes in the gradient x's other
    # consumer deposited; a tagged x2 (the decoder's skip input) gets ITS gradient deposited instead of returned to autograd
    return _ConvBNAct.apply(x, x2, residual, conv.weight, bn.weight, bn.bias, bn, conv.stride[0], pad,
                            conv.padding_mode == "reflect" and pad > 0, relu, None, not bn.training and not torch.is_grad_enabled(),
                            link_in, link_out, link_x, _fanin_of(x) if absorb_fanin else None, _fanin_of(x2))


# Within ONE training step the same image tensor goes through several stems: both networks of a CPS pair see the same
# batches, and the unlabelled batch passes twice (pseudo-label forward, training forward).  The patch matrix depends on the
# image alone, so a caller may open a sharing scope for the step (trainer.CPSTrainer does): forwards on the SAME tensor
# object (same version) inside the scope reuse one matrix.  Nothing is kept across scopes -- every step's images are
# unfolded in that step.
_STEM_SHARE = None


def stem_share_begin():
    global _STEM_SHARE
    _STEM_SHARE = []


def stem_share_end():
    global _STEM_SHARE
    _STEM_SHARE = None


def _shared_stem_patches(x, cfg, make):
    if _STEM_SHARE is None:
        return make()
    cur = torch.cuda.current_stream(x.device)
    for ref, ver, key, patches, ev, st in _STEM_SHARE:
        if ref() is x and ver == x._version and key == cfg:
            if st != cur:                                   # produced on the other network's stream
                cur.wait_event(ev)
                patches.record_stream(cur)
            return patches
    patches = make()
    ev = torch.cuda.Event()
    ev.record(cur)
    _STEM_SHARE.append((weakref.ref(x), x._version, cfg, patches, ev, cur))
    return patches


_STEM_X_ARG = [None]            # hands the image tensor OBJECT (patch-sharing identity) to _ConvBNAct.forward past autograd's argument handling


def _stem_patches(xr, dt, kh, kw, s, p, reflect, ho, wo, kp):
    """the stem's im2col patch matrix [n][ho][wo][kp] of the fp32 image rows xr"""
    n, h, w, cin = xr.shape
    out = torch.empty((n, ho, wo, kp), dtype=dt, device=xr.device)
    _launch("vqseg_im2col_f", xr.device, int(dt == torch.bfloat16), _f32(xr, "image", n * h * w * cin), n, h, w, cin, kh, kw, s, p, int(reflect), ho,
            wo, kp, _T(out, "patches", bf=int(dt == torch.bfloat16), numel=n * ho * wo * kp))
    return out


def _stem_weights_fused(weight, s3: bool):
    """vqseg_stem7_conv_f's weight image: [64][176] bf16, column kh * 24 + kw * 3 + ci (each kernel row's 21 taps padded to 24), zeros
    elsewhere; split-3: [64][2][176] = hi | lo.  Cached on the Parameter (_wcache: rebuilt after every optimiser step)."""
    cache = _cache_of(weight)
    k = ("stem_fused", bool(s3))
    if k not in cache:
        cout, cin, kh, kw = weight.shape
        w = weight.detach().float().permute(0, 2, 3, 1).reshape(cout, kh, kw * cin)           # [co][kh][(kw, ci)]
        wp = torch.zeros(cout, 176, dtype=torch.float32, device=weight.device)
        wp[:, :kh * 24].view(cout, kh, 24)[:, :, :kw * cin] = w
        hi = wp.to(torch.bfloat16)
        img = torch.cat([hi, (wp - hi.float()).to(torch.bfloat16)], dim=1) if s3 else hi
        cache[k] = img.contiguous().view(torch.int16)
    return cache[k]


def stem_conv_bn_act(x, conv, bn):
    """7x7 stride-2 stem on a 3-channel fp32 image: im2col patch matrix (zero / reflect padding) + 1x1 MFMA conv."""
    if not x.is_cuda:
        raise _hip.HipLibraryError(f"the HIP path needs 'cuda' (ROCm) tensors, got {x.device}; there is no CPU fallback")
    xr = _rows(x.float())
    n, h, w, cin = xr.shape
    kh, kw = conv.kernel_size
    s, p = conv.stride[0], conv.padding[0]
    reflect = conv.padding_mode == "reflect"
    ho, wo = _out_size(h, kh, s, p), _out_size(w, kw, s, p)
    kp = _pad32(kh * kw * cin)
    stem = StemGeom(kh, kw, cin, s, p, reflect, h, w)
    dt = act_dtype()
    # The convolution straight from the image (vqseg_stem7_conv_f) where its tiling fits: 128 output pixels of one row per workgroup.
    # It removes 7.5 GB of patch-matrix traffic per step and its kernel takes 197 us against 318 us; -0.9 ms of a 146 ms step (LEDGER
    # r4).  The patch-matrix path (VQSEG_OPTS=py_stem_fused=0) stays for output widths that are not multiples of 128 and for the
    # weight gradient
    fused_ok = ((kh, kw, cin) == (7, 7, 3) and s == 2 and p == 3 and wo % 128 == 0 and h >= 4 and w >= 4 and conv.weight.shape[0] == 64
                and py_opt("py_stem_fused", 1) == 1)
    if _S3_SCOPE and dt == torch.float32 and not bn.training and not torch.is_grad_enabled() and (kh, kw, cin) == (7, 7, 3):
        # fp32-precision eval forward: split-3 patch rows (64-column multiple: the LDS-DMA kernels), then everything stays split-3
        kp3 = (kh * kw * cin + 63) // 64 * 64

        def make3():
            out = torch.empty((n, ho, wo, 2 * kp3), dtype=torch.bfloat16, device=x.device)
            _launch("vqseg_im2col_f", x.device, 2, _f32(xr, "image", n * h * w * cin), n, h, w, cin, kh, kw, s, p, int(reflect), ho, wo, kp3,
                    _T(out, "split-3 patches", bf=2, numel=n * ho * wo * 2 * kp3))
            return out

        if fused_ok:                                             # no split-3 patch matrix (1.6 GB written, read by both networks)
            cout = conv.weight.shape[0]
            coef = _bn_finalize(None, n * ho * wo, cout, bn.weight, bn.bias, bn, False, x.device)
            out = _stem7_conv(xr, _stem_weights_fused(conv.weight, True), None, coef, True, stem._replace(fused=(ho, wo, kp)), cout, s3=True)
            return S3(out, cout)
        patches = _shared_stem_patches(x, ("s3", kh, kw, s, p, reflect), make3)
        return _conv_bn_act_s3(S3(patches, kp3), None, None, conv, bn, True, kernel_1x1_cols=kp3)

    fuse_eval = not bn.training and not torch.is_grad_enabled()
    if fused_ok and dt == torch.bfloat16 and kp == 160:
        _sink_use(conv.weight, bn.weight, bn.bias)
        _STEM_X_ARG[0] = x
        return _ConvBNAct.apply(_nchw(xr), None, None, conv.weight, bn.weight, bn.bias, bn, 1, 0, False, True,
                                stem._replace(fused=(ho, wo, kp)), fuse_eval)
    patches = _shared_stem_patches(x, (dt, kh, kw, s, p, reflect), lambda: _stem_patches(xr, dt, kh, kw, s, p, reflect, ho, wo, kp))
    _sink_use(conv.weight, bn.weight, bn.bias)
    return _ConvBNAct.apply(_nchw(patches), None, None, conv.weight, bn.weight, bn.bias, bn, 1, 0, False, True, stem, fuse_eval)


# ------------------------------------------------------------------------------------------------
class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fan=None):
        xr = _rows(x)
        n, h, w, c = xr.shape
        ho, wo = _out_size(h, 3, 2, 1), _out_size(w, 3, 2, 1)
        y = torch.empty((n, ho, wo, c), dtype=xr.dtype, device=xr.device)
        idx = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=xr.device) if ctx.needs_input_grad[0] else None
        bf = _is_bf16(xr)
        _launch("vqseg_maxpool3x3s2_f", xr.device, bf, 0, _T(xr, "pool input", bf=bf, numel=n * h * w * c), None, n, h, w, c,
                _T(y, "pool output", bf=bf, numel=n * ho * wo * c), _T(idx, "pool argmax", dtype=torch.uint8, numel=n * ho * wo * c))
        ctx.save_for_backward(idx)                          # window position of every maximum: the input is not kept
        ctx.cfg = (n, h, w, c, xr.dtype)
        ctx.fan = fan
        return _nchw(y)

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        n, h, w, c, dt = ctx.cfg
        gr = _rows(g).to(dt)
        gx = torch.empty((n, h, w, c), dtype=dt, device=gr.device)
        bf = int(dt == torch.bfloat16)
        add = _fanin_take(ctx.fan, (n, h, w, c), dt)       # the pooled tensor's other consumer deposited its gradient: added in the kernel
        if add is not None:
            _launch("vqseg_maxpool3x3s2_backward_add_f", gr.device, bf, _T(gr, "pool output gradient", bf=bf, numel=idx.numel()),
                    _T(idx, "pool argmax", dtype=torch.uint8), _T(add, "fan-in gradient", bf=bf, numel=n * h * w * c), n, h, w, c,
                    _T(gx, "pool input gradient", bf=bf, numel=n * h * w * c))
        else:
            _launch("vqseg_maxpool3x3s2_f", gr.device, bf, 1, None, _T(gr, "pool output gradient", bf=bf, numel=idx.numel()), n, h, w, c,
                    _T(gx, "pool input gradient", bf=bf, numel=n * h * w * c), _T(idx, "pool argmax", dtype=torch.uint8))
        if ctx.fan is not None and ctx.fan.leftover is not None:
            gx = gx + ctx.fan.leftover.reshape(gx.shape).to(dt)
            ctx.fan.leftover = None
        return _nchw(gx), None


def max_pool_3x3_s2(x):
    if isinstance(x, S3):
        n, h, w, _ = x.rows.shape
        ho, wo = _out_size(h, 3, 2, 1), _out_size(w, 3, 2, 1)
        y = torch.empty((n, ho, wo, 2 * x.c), dtype=torch.bfloat16, device=x.rows.device)
        _launch("vqseg_s3_maxpool3x3s2_f", y.device, _T(x.rows, "split-3 pool input", bf=2, numel=n * h * w * 2 * x.c), n, h, w, x.c,
                _T(y, "split-3 pool output", bf=2, numel=n * ho * wo * 2 * x.c))
        return S3(y, x.c)
    return _MaxPool.apply(x, _fanin_of(x))


class _Bilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ho, wo, align):
        xr = _rows(x)
        n, h, w, c = xr.shape
        y = torch.empty((n, ho, wo, c), dtype=xr.dtype, device=xr.device)
        bf = _is_bf16(xr)
        _launch("vqseg_bilinear_f", xr.device, bf, 0, _T(xr, "resize input", bf=bf, numel=n * h * w * c), n, h, w, c, ho, wo, int(align),
                _T(y, "resize output", bf=bf, numel=n * ho * wo * c))
        ctx.cfg = (n, h, w, c, ho, wo, int(align), xr.dtype)
        return _nchw(y)

    @staticmethod
    def backward(ctx, g):
        n, h, w, c, ho, wo, align, dt = ctx.cfg
        gr = _rows(g).to(dt)
        gx = torch.empty((n, h, w, c), dtype=dt, device=gr.device)
        bf = int(dt == torch.bfloat16)
        _launch("vqseg_bilinear_f", gr.device, bf, 1, _T(gr, "resize output gradient", bf=bf, numel=n * ho * wo * c), n, h, w, c, ho, wo, align,
                _T(gx, "resize input gradient", bf=bf, numel=n * h * w * c))
        return _nchw(gx), None, None, None


def upsample_bilinear(x, size=None, scale_factor=None, align_corners=False):
    if size is None:
        size = (int(x.shape[-2] * scale_factor), int(x.shape[-1] * scale_factor))
    if isinstance(x, S3):
        n, h, w, _ = x.rows.shape
        y = torch.empty((n, int(size[0]), int(size[1]), 2 * x.c), dtype=torch.bfloat16, device=x.rows.device)
        _launch("vqseg_s3_bilinear_f", y.device, _T(x.rows, "split-3 resize input", bf=2, numel=n * h * w * 2 * x.c), n, h, w, x.c, int(size[0]),
                int(size[1]), int(bool(align_corners)), _T(y, "split-3 resize output", bf=2, numel=y.numel()))
        return S3(y, x.c)
    return _Bilinear.apply(x, int(size[0]), int(size[1]), bool(align_corners))


class _Head1x1(torch.autograd.Function):
    """nn.Conv2d(Cin, num_classes <= 4, 1, bias=False): fp32 logits whatever the activation dtype."""

    @staticmethod
    def forward(ctx, x, weight, fan=None):
        ctx.fan = fan
        xr = _rows(x)
        n, h, w, cin = xr.shape
        cout = weight.shape[0]
        wt = weight.detach().reshape(cout, cin).contiguous()
        y = torch.empty((n, h, w, cout), dtype=torch.float32, device=xr.device)
        bf = _is_bf16(xr)
        _launch("vqseg_head1x1_forward_f", xr.device, bf, _T(xr, "head input", bf=bf, numel=n * h * w * cin), _f32(wt, "head weight", cout * cin),
                n * h * w, cin, cout, _f32(y, "logits", n * h * w * cout))
        ctx.save_for_backward(xr, wt)
        return _nchw(y)

    @staticmethod
    def backward(ctx, g):
        xr, wt = ctx.saved_tensors
        n, h, w, cin = xr.shape
        cout = wt.shape[0]
        m = n * h * w
        gr = _rows(g).float()
        gx = torch.empty_like(xr)
        gw = torch.empty((cout, cin), dtype=torch.float32, device=xr.device)
        ws = torch.empty(lib().vqseg_head1x1_backward_workspace_floats(m, cin, cout), dtype=torch.float32, device=xr.device)
        add = _fanin_take(ctx.fan, xr.shape, xr.dtype)      # the prototype loss's gradient of the same decoder output, if it came first
        bf = _is_bf16(xr)
        _launch("vqseg_head1x1_backward_add_f", xr.device, bf, _T(xr, "head input", bf=bf, numel=m * cin), _f32(wt, "head weight", cout * cin),
                _f32(gr, "logit gradient", m * cout), m, cin, cout, _T(gx, "head input gradient", bf=bf, numel=m * cin),
                _f32(gw, "head weight gradient", cout * cin), _f32(ws, "head workspace"), _T(add, "fan-in gradient", bf=bf, numel=m * cin))
        if ctx.fan is not None and ctx.fan.leftover is not None:
            gx = gx + ctx.fan.leftover.reshape(gx.shape).to(gx.dtype)
            ctx.fan.leftover = None
        return _nchw(gx), gw.reshape(cout, cin, 1, 1), None


def head_conv1x1(x, weight):
    if isinstance(x, S3) and not torch.is_grad_enabled():    # split-3 eval forward: the head reads hi + lo itself
        n, h, w, _ = x.rows.shape
        cout = weight.shape[0]
        wt = weight.detach().reshape(cout, x.c).contiguous()
        y = torch.empty((n, h, w, cout), dtype=torch.float32, device=x.rows.device)
        _launch("vqseg_head1x1_forward_f", y.device, 2, _T(x.rows, "split-3 head input", bf=2, numel=n * h * w * 2 * x.c),
                _f32(wt, "head weight", cout * x.c), n * h * w, x.c, cout, _f32(y, "logits", n * h * w * cout))
        return _nchw(y)
    return _Head1x1.apply(from_s3(x), weight, _fanin_of(x))


class _Cast(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src = x.dtype
        if x.dtype == dtype:
            return x
        xr = _rows(x)
        y = torch.empty(xr.shape, dtype=dtype, device=xr.device)
        to_bf = int(dtype == torch.bfloat16)
        _launch("vqseg_cast_f", xr.device, to_bf, _T(xr, "cast input", bf=1 - to_bf), xr.numel(), _T(y, "cast output", bf=to_bf, numel=xr.numel()))
        return _nchw(y)

    @staticmethod
    def backward(ctx, g):
        return _Cast.apply(g, ctx.src), None


def cast_act(x, dtype):
    """f32 <-> bf16 activation cast (NHWC), differentiable."""
    if isinstance(x, S3):
        return x if dtype == torch.float32 else cast_act(x.float(), dtype)
    if x.dtype == dtype:
        return x
    if {x.dtype, dtype} != {torch.float32, torch.bfloat16}:
        return x.to(dtype)
    return _Cast.apply(x, dtype)


# ------------------------------------------------------------------------------------------------
# Reliable prototype losses (models/modules/prototype.py): fused forward / backward over the decoder features
# ------------------------------------------------------------------------------------------------
class _ProtoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, proto, labels, keep, conf, variant, scale, margin, easy_margin, fan=None):
        ctx.fan = fan
        xr = _rows(x)
        n, h, w, c = xr.shape
        m, k = n * h * w, proto.shape[0]
        L = lib()
        proto = proto.detach().float().contiguous()
        labels = labels.reshape(-1).long().contiguous()
        keep = keep.reshape(-1).to(torch.uint8).contiguous() if keep is not None else None
        conf = conf.reshape(-1).float().contiguous() if conf is not None else None
        nbytes = L.vqseg_proto_loss_workspace_bytes(m, c, k)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=xr.device)
        loss = torch.empty((), dtype=torch.float64, device=xr.device)
        bf = _is_bf16(xr)
        _launch("vqseg_proto_loss_forward_f", xr.device, bf, _T(xr, "decoder features", bf=bf, numel=m * c), _f32(proto, "prototypes", k * c),
                _T(labels, "labels", dtype=torch.int64, numel=m), _T(keep, "keep mask", dtype=torch.uint8, numel=m), _f32(conf, "confidence", m), m,
                c, k, variant, float(scale), float(margin), int(easy_margin), _T(ws, "workspace", dtype=torch.uint8, numel=nbytes), nbytes,
                _T(loss, "loss", dtype=torch.float64, numel=1))
        ctx.save_for_backward(xr, proto, labels, keep, conf)
        ctx.cfg = (m, c, k, variant, float(scale), float(margin), int(easy_margin))
        return loss

    @staticmethod
    def backward(ctx, g):
        xr, proto, labels, keep, conf = ctx.saved_tensors
        m, c, k, variant, scale, margin, easy = ctx.cfg
        L = lib()
        g32 = g.detach().float().reshape(1).contiguous()
        gx = torch.empty_like(xr)
        gproto = torch.empty_like(proto) if ctx.needs_input_grad[1] else None
        nbytes = L.vqseg_proto_loss_workspace_bytes(m, c, k)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=xr.device)
        bf = _is_bf16(xr)
        _launch("vqseg_proto_loss_backward_f", xr.device, bf, _T(xr, "decoder features", bf=bf, numel=m * c), _f32(proto, "prototypes", k * c),
                _T(labels, "labels", dtype=torch.int64, numel=m), _T(keep, "keep mask", dtype=torch.uint8, numel=m), _f32(conf, "confidence", m), m,
                c, k, variant, scale, margin, easy, _f32(g32, "loss gradient", 1), _T(gx, "feature gradient", bf=bf, numel=m * c),
                _f32(gproto, "prototype gradient", k * c), _T(ws, "workspace", dtype=torch.uint8, numel=nbytes), nbytes)
        if _fanin_deposit(ctx.fan, gx):                      # the head's backward (same decoder output) adds it in its kernel
            return None, gproto, None, None, None, None, None, None, None, None
        return _nchw(gx), gproto, None, None, None, None, None, None, None, None


def proto_loss_supported(x, num_classes: int) -> bool:
    return x.is_cuda and x.dim() == 4 and x.shape[1] % 8 == 0 and x.shape[1] <= 64 and num_classes <= 4 and \
        x.dtype in (torch.float32, torch.bfloat16)


def proto_loss(x, proto, labels, keep=None, conf=None, variant=1, scale=1.0, margin=0.0, easy_margin=True):
    """-mean( log( exp(S) / (sum_c exp(z_c) + 1e-7) + 1e-7 ) * w ) of the reliable prototype losses (float64 scalar);
    x (N, C, H, W) decoder features, proto (K, C) L2-normalised, labels / keep / conf per pixel in (n, h, w) order."""
    return _ProtoLoss.apply(x, proto, labels, keep, conf, variant, scale, margin, easy_margin, _fanin_of(x))


# ------------------------------------------------------------------------------------------------
# Soft Dice sums (loss/dice_loss.py): inter / sets per (image, class) in one pass, closed-form backward
# ------------------------------------------------------------------------------------------------
class _DiceSums(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, ignore_index, want_ce=False):
        b, c, h, w = pred.shape
        sb, sc, sh, sw = pred.stride()
        if sh != w * sw:                                   # pixels must be linear in memory (NCHW and NHWC both are)
            pred = pred.contiguous()
            sb, sc, sh, sw = pred.stride()
        tgt = target.reshape(b, h * w).long().contiguous()
        L = lib()
        nbytes = L.vqseg_dice_workspace_bytes(b, c, h * w)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
        out = torch.empty(2, b, c, dtype=torch.float32, device=pred.device)
        ce = torch.empty(b, 2, dtype=torch.float32, device=pred.device) if want_ce else None
        ign = -(1 << 62) if ignore_index is None else int(ignore_index)
        _launch("vqseg_dice_ce_sums_forward_f", pred.device, _strided_f32(pred, "logits", b * c * h * w), sb, sc, sw,
                _T(tgt, "targets", dtype=torch.int64, numel=b * h * w), b, c, h * w, ign, _T(ws, "workspace", dtype=torch.uint8, numel=nbytes),
                nbytes, _f32(out[0], "intersections", b * c), _f32(out[1], "set sizes", b * c), _f32(ce, "cross-entropy sums", b * 2))
        ctx.save_for_backward(pred, tgt)
        ctx.cfg = (b, c, h * w, ign, (sb, sc, sw), want_ce)
        if want_ce:
            return out[0], out[1], ce
        return out[0], out[1]

    @staticmethod
    def backward(ctx, g_inter, g_sets, g_ce=None):
        pred, tgt = ctx.saved_tensors
        b, c, hw, ign, (sb, sc, sw), want_ce = ctx.cfg
        g = torch.empty_strided(pred.shape, pred.stride(), dtype=torch.float32, device=pred.device)
        gi, gs = g_inter.float().contiguous(), g_sets.float().contiguous()
        gc = g_ce.float().contiguous() if (want_ce and g_ce is not None) else None
        _launch("vqseg_dice_ce_sums_backward_f", pred.device, _strided_f32(pred, "logits", b * c * hw), sb, sc, sw,
                _T(tgt, "targets", dtype=torch.int64, numel=b * hw), b, c, hw, ign, _f32(gi, "d intersections", b * c),
                _f32(gs, "d set sizes", b * c), _f32(gc, "d cross-entropy sums", b * 2), _strided_f32(g, "logit gradient", b * c * hw))
        return g, None, None, None


def dice_sums_supported(pred, num_classes: int) -> bool:
    return pred.is_cuda and pred.dim() == 4 and pred.dtype == torch.float32 and 2 <= num_classes <= 4 and pred.shape[1] == num_classes


def dice_sums(pred, target, ignore_index):
    """(inter, sets), each (B, C) float32: sum over pixels of softmax * onehot and of softmax + onehot (dice_loss.py:24-26)."""
    return _DiceSums.apply(pred, target, ignore_index)


def dice_ce_sums(pred, target, ignore_index):
    """(inter, sets, ce): the Dice sums plus ce (B, 2) = (sum of -log softmax[target], number of pixels) over the pixels whose
    target != ignore_index -- nn.CrossEntropyLoss(ignore_index)'s mean is ce[:, 0].sum() / ce[:, 1].sum() -- in the same pass
    over the logits, forward and backward (vqseg_dice_ce_sums_*)."""
    return _DiceSums.apply(pred, target, ignore_index, True)


def _loss_inputs(pred, target, ignore_index):
    """what every pass over (B, C, H, W) logits + targets takes: the logits with linear pixels, the (B, HW) int64 targets, the
    (batch, class, pixel) strides and the ignore index as an integer (None: a value no label has)"""
    b, c, h, w = pred.shape
    sb, sc, sh, sw = pred.stride()
    if sh != w * sw:                                       # pixels must be linear in memory (NCHW and NHWC both are)
        pred = pred.contiguous()
        sb, sc, sh, sw = pred.stride()
    tgt = target.reshape(b, h * w).long().contiguous()
    ign = -(1 << 62) if ignore_index is None else int(ignore_index)
    return pred, tgt, (sb, sc, sw), ign


def _class_weights(weight, c, dev):
    """the C class weights as the kernels read them: float32 on the logits' device (a device tensor stays where it is)"""
    if weight is None:
        return None
    w = weight.detach().to(device=dev, dtype=torch.float32).contiguous()
    if w.numel() != c:
        raise _hip.HipLibraryError(f"class weights: the sizes passed along need {c} elements, the tensor has {w.numel()} (shape {tuple(w.shape)})")
    return w


# ------------------------------------------------------------------------------------------------
# Focal loss (loss/focal_loss.py): one pass forward, one backward (vqseg_focal_*)
# ------------------------------------------------------------------------------------------------
class _Focal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weight, alpha, gamma, ignore_index, reduction, pre_softmax):
        if reduction not in ("none", "mean", "sum"):
            raise NotImplementedError(f"Invalid reduction mode: {reduction}")
        b, c, h, w = pred.shape
        hw = h * w
        pred, tgt, (sb, sc, sw), ign = _loss_inputs(pred, target, ignore_index)
        dev = pred.device
        wt = _class_weights(weight, c, dev)
        L = lib()
        nbytes = L.vqseg_focal_workspace_bytes(b, hw)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        per_image = torch.empty(b, dtype=torch.float64, device=dev)
        loss2 = torch.empty(2, dtype=torch.float32, device=dev)
        lmap = torch.empty(b, hw, dtype=torch.float32, device=dev) if reduction == "none" else None
        _launch("vqseg_focal_forward_f", dev, _strided_f32(pred, "logits", b * c * hw), sb, sc, sw, _T(tgt, "targets", dtype=torch.int64, numel=b * hw),
                b, c, hw, ign, _f32(wt, "class weights", c), float(alpha), float(gamma), int(bool(pre_softmax)),
                _T(ws, "workspace", dtype=torch.uint8, numel=nbytes), nbytes, _T(per_image, "per-image sums", dtype=torch.float64, numel=b),
                _f32(loss2, "loss", 2), _f32(lmap, "loss map", b * hw))
        ctx.save_for_backward(pred, tgt, wt)
        ctx.cfg = (b, c, hw, ign, (sb, sc, sw), float(alpha), float(gamma), int(bool(pre_softmax)), reduction)
        if reduction == "none":
            return lmap                                        # (B, HW), as the reference returns it
        return loss2[0] if reduction == "sum" else loss2[1]

    @staticmethod
    def backward(ctx, g_out):
        pred, tgt, wt = ctx.saved_tensors
        b, c, hw, ign, (sb, sc, sw), alpha, gamma, pre, reduction = ctx.cfg
        g = torch.empty_strided(pred.shape, pred.stride(), dtype=torch.float32, device=pred.device)
        if reduction == "none":
            g_scalar, scale, g_map = None, 0.0, g_out.float().contiguous()
        else:
            g_scalar, scale, g_map = g_out.float().reshape(1).contiguous(), (1.0 if reduction == "sum" else 1.0 / (b * hw)), None
        _launch("vqseg_focal_backward_f", pred.device, _strided_f32(pred, "logits", b * c * hw), sb, sc, sw,
                _T(tgt, "targets", dtype=torch.int64, numel=b * hw), b, c, hw, ign, _f32(wt, "class weights", c), alpha, gamma, pre,
                _f32(g_scalar, "loss gradient", 1), scale, _f32(g_map, "loss map gradient", b * hw), _strided_f32(g, "logit gradient", b * c * hw))
        return g, None, None, None, None, None, None, None


def focal(pred, target, alpha, gamma, ignore_index, reduction="sum", weight=None, pre_softmax=False):
    """focal_loss (loss/focal_loss.py:6-50; `pre_softmax`: the module FocalLoss.forward, :62-68) of (B, C, H, W) float32 logits that pass
    dice_sums_supported, gamma == 0 or >= 1: a 0-d float32 tensor ('sum', 'mean') or the (B, HW) map ('none')."""
    return _Focal.apply(pred, target, weight, alpha, gamma, ignore_index, reduction, pre_softmax)


class _WceSums(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weight, ignore_index):
        b, c, h, w = pred.shape
        hw = h * w
        pred, tgt, (sb, sc, sw), ign = _loss_inputs(pred, target, ignore_index)
        dev = pred.device
        wt = _class_weights(weight, c, dev)
        L = lib()
        nbytes = L.vqseg_focal_workspace_bytes(b, hw)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        ce = torch.empty(b, 2, dtype=torch.float32, device=dev)
        _launch("vqseg_wce_sums_forward_f", dev, _strided_f32(pred, "logits", b * c * hw), sb, sc, sw, _T(tgt, "targets", dtype=torch.int64, numel=b * hw),
                b, c, hw, ign, _f32(wt, "class weights", c), _T(ws, "workspace", dtype=torch.uint8, numel=nbytes), nbytes,
                _f32(ce, "cross-entropy sums", b * 2))
        ctx.save_for_backward(pred, tgt, wt)
        ctx.cfg = (b, c, hw, ign, (sb, sc, sw))
        return ce

    @staticmethod
    def backward(ctx, g_ce):
        pred, tgt, wt = ctx.saved_tensors
        b, c, hw, ign, (sb, sc, sw) = ctx.cfg
        g = torch.empty_strided(pred.shape, pred.stride(), dtype=torch.float32, device=pred.device)
        gc = g_ce.float().contiguous()
        _launch("vqseg_wce_sums_backward_f", pred.device, _strided_f32(pred, "logits", b * c * hw), sb, sc, sw,
                _T(tgt, "targets", dtype=torch.int64, numel=b * hw), b, c, hw, ign, _f32(wt, "class weights", c),
                _f32(gc, "d cross-entropy sums", b * 2), _strided_f32(g, "logit gradient", b * c * hw))
        return g, None, None, None


def wce_sums(pred, target, weight, ignore_index):
    """ce (B, 2) = (sum of w[t] * -log softmax[t], sum of w[t]) over the pixels whose target != ignore_index:
    F.cross_entropy(pred, target, weight=w, ignore_index)'s mean is ce[:, 0].sum() / ce[:, 1].sum() (vqseg_wce_sums_*)."""
    if weight is None:
        raise _hip.HipLibraryError("class weights: expected a tensor, got None")
    return _WceSums.apply(pred, target, weight, ignore_index)


def class_weight(num_classes: int, y):
    """(weight (num_classes,) f32, counts (num_classes + 1,) i64) of the labels `y` on their device, no host synchronisation
    (vqseg_class_weight_f): counts[c] for c < num_classes, counts[-1] = the labels >= 0, weight = 1 - counts[:-1] / counts[-1]."""
    nc = int(num_classes)
    labels = y.reshape(-1)
    if labels.dtype != torch.int64 or not labels.is_contiguous():
        labels = labels.long().contiguous()
    n = labels.numel()
    counts = torch.empty(nc + 1, dtype=torch.int64, device=labels.device)
    weight = torch.empty(nc, dtype=torch.float32, device=labels.device)
    _launch("vqseg_class_weight_f", labels.device, _T(labels, "labels", dtype=torch.int64, numel=n), n, nc,
            _T(counts, "class counts", dtype=torch.int64, numel=nc + 1), _f32(weight, "class weights", nc))
    return weight, counts


# ------------------------------------------------------------------------------------------------
# Pixel-pair supervised contrastive loss (loss/contrastive_loss.py): fused forward / backward over all pixel pairs of images 0 and 1
# (vqseg_supcon_*), no (HW, HW) matrix
# ------------------------------------------------------------------------------------------------
def _supcon_targets(x, target):
    """the (B, Ht, Wt) int64 targets of a (B, C, H, W) feature tensor, or a HipLibraryError saying what is wrong"""
    if not torch.is_tensor(target) or target.dim() not in (3, 4) or (target.dim() == 4 and target.shape[1] != 1):
        raise _hip.HipLibraryError(f"supcon: targets must be a (B, Ht, Wt) or (B, 1, Ht, Wt) tensor, got {tuple(getattr(target, 'shape', ()))}")
    if target.is_floating_point() or target.dtype == torch.bool:
        raise _hip.HipLibraryError(f"supcon: targets must be integer class labels, got {target.dtype}")
    if target.shape[0] < 2 or target.shape[0] != x.shape[0]:
        raise _hip.HipLibraryError(f"supcon: one target per image of the batch of {x.shape[0]} (at least 2) required, got {target.shape[0]}")
    tgt = target.reshape(target.shape[0], target.shape[-2], target.shape[-1])
    return tgt if tgt.dtype == torch.int64 and tgt.is_contiguous() else tgt.long().contiguous()


def _supcon_forward(x, target, temperature):
    """-> the feature rows (B, H, W, C), the (B, Ht, Wt) int64 targets and the forward's 8-float result block (include/vqseg.h)"""
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[0] < 2:
        raise _hip.HipLibraryError(f"supcon: features must be a (B >= 2, C, H, W) tensor, got {tuple(getattr(x, 'shape', ()))}")
    xr = _rows(x.detach())
    bf = _is_bf16(xr)
    b, h, w, c = xr.shape
    if c % 16 or not 16 <= c <= 128:
        raise _hip.HipLibraryError(f"supcon: channels must be a multiple of 16 up to 128, got {c}")
    tgt = _supcon_targets(x, target)
    ht, wt = tgt.shape[1:]
    hw, dev = h * w, xr.device
    nbytes = lib().vqseg_supcon_workspace_bytes(hw)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(8, dtype=torch.float32, device=dev)
    _launch("vqseg_supcon_forward_f", dev, bf, _T(xr[0], "features of image 0", bf=bf, numel=hw * c), _T(xr[1], "features of image 1", bf=bf, numel=hw * c),
            c, h, w, c, _T(tgt[0], "targets of image 0", dtype=torch.int64, numel=ht * wt), _T(tgt[1], "targets of image 1", dtype=torch.int64, numel=ht * wt),
            ht, wt, float(temperature), _T(ws, "workspace", dtype=torch.uint8, numel=nbytes), nbytes, _f32(out, "loss", 8))
    return xr, tgt, out


class _SupCon(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target, temperature):
        xr, tgt, out = _supcon_forward(x, target, temperature)
        ctx.save_for_backward(xr, tgt, out)
        ctx.temperature = float(temperature)
        return out[0]

    @staticmethod
    def backward(ctx, g_out):
        xr, tgt, out = ctx.saved_tensors
        b, h, w, c = xr.shape
        ht, wt = tgt.shape[1:]
        hw, bf = h * w, _is_bf16(xr)
        g32 = g_out.detach().float().reshape(1).contiguous()   # stays on the device: under a gradient scaler it holds the scale
        gx = torch.empty_like(xr)
        gx[2:].zero_()                                         # only images 0 and 1 enter the loss
        _launch("vqseg_supcon_backward_f", xr.device, bf, _T(xr[0], "features of image 0", bf=bf, numel=hw * c),
                _T(xr[1], "features of image 1", bf=bf, numel=hw * c), c, h, w, c, _T(tgt[0], "targets of image 0", dtype=torch.int64, numel=ht * wt),
                _T(tgt[1], "targets of image 1", dtype=torch.int64, numel=ht * wt), ht, wt, ctx.temperature, _f32(out, "forward statistics", 8),
                _f32(g32, "loss gradient", 1), _T(gx[0], "feature gradient of image 0", bf=bf, numel=hw * c),
                _T(gx[1], "feature gradient of image 1", bf=bf, numel=hw * c), c)
        return _nchw(gx), None, None


def supcon_supported(x, target) -> bool:
    """what the fused contrastive pass takes: (B >= 2, C, H, W) float32 / bfloat16 GPU features with C a multiple of 16 up to 128 and
    integer (B, Ht, Wt) or (B, 1, Ht, Wt) targets on the same device; everything else is SupConLoss's torch-op form"""
    return (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.shape[0] >= 2 and x.dtype in (torch.float32, torch.bfloat16)
            and x.shape[1] % 16 == 0 and 16 <= x.shape[1] <= 128 and x.shape[2] * x.shape[3] >= 1
            and torch.is_tensor(target) and target.device == x.device and not target.is_floating_point() and target.dtype != torch.bool
            and (target.dim() == 3 or (target.dim() == 4 and target.shape[1] == 1)) and target.shape[0] == x.shape[0])


def supcon(x, target, temperature=0.04):
    """SupConLoss.forward (loss/contrastive_loss.py:13-30) of (B, C, H, W) features and their integer targets: a 0-d float32 tensor,
    (logA - logP) / (HW * HW) over all pixel pairs of images 0 and 1, finite wherever the inputs are and a positive pair exists.  The
    gradient with respect to x is zero outside images 0 and 1 and returns to autograd in the ordinary way (no fan-in deposit).  The
    value's companions logA and logP are `supcon_stats`'s."""
    return _SupCon.apply(x, target, temperature)


def supcon_stats(x, target, temperature=0.04):
    """(loss, logA, logP) as a float32 device tensor, no gradient (tests, profiles)"""
    return _supcon_forward(x, target, temperature)[2][:3]


# ------------------------------------------------------------------------------------------------
# Confidence-weighted soft CPS loss (conf_ce_loss of deprecated/train_vq_pt_unet_conf_ce.py:50-113): one pass forward, one backward
# over input AND target logits (vqseg_conf_ce_*); the pair form gives both directions from one read of the two tensors
# ------------------------------------------------------------------------------------------------
CONF_CE_STATS = ("sum_pos", "sum_neg", "sum_p2", "m", "mn", "inv_m", "inv_mn", "loss")      # the columns of the stats record


def conf_ce_supported(x, t) -> bool:
    """what the fused pass takes: two (B, C, H, W) float32 GPU logit tensors of one shape and device, 2..4 classes (the shapes and
    layouts of dice_sums_supported); everything else is loss.conf_ce_loss's torch-op form"""
    return (torch.is_tensor(x) and torch.is_tensor(t) and x.dim() == 4 and dice_sums_supported(x, x.shape[1]) and t.shape == x.shape
            and t.dtype == torch.float32 and t.device == x.device and x.numel() > 0 and x.shape[0] <= 65535)


def _conf_logits(v, name):
    """dense logits, NCHW or channels_last (the gradient is allocated with the same strides), and their (batch, class, pixel) strides"""
    if not torch.is_tensor(v) or v.dim() != 4:
        raise _hip.HipLibraryError(f"conf_ce: {name} must be a (B, C, H, W) tensor, got {tuple(getattr(v, 'shape', ()))}")
    if not (v.is_contiguous() or v.is_contiguous(memory_format=torch.channels_last)):
        v = v.contiguous()
    sb, sc, _sh, sw = v.stride()
    return v, (sb, sc, sw)


def _conf_forward(x, t, threshold, threshold_neg, temperature, pair):
    x, xs = _conf_logits(x.detach(), "inputs")
    t, ts = _conf_logits(t.detach(), "targets")
    if t.shape != x.shape:
        raise _hip.HipLibraryError(f"conf_ce: inputs and targets must have one shape, got {tuple(x.shape)} and {tuple(t.shape)}")
    b, c, h, w = x.shape
    hw, dev, nd = h * w, x.device, 2 if pair else 1
    nbytes = lib().vqseg_conf_ce_workspace_bytes(b, hw)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)     # (8-byte aligned)
    stats = torch.empty(nd, len(CONF_CE_STATS), dtype=torch.float64, device=dev)
    loss = torch.empty(nd, dtype=torch.float32, device=dev)
    cfg = (b, c, hw, xs, ts, float(threshold), float(threshold_neg), float(temperature), int(bool(pair)))
    _launch("vqseg_conf_ce_forward_f", dev, _strided_f32(x, "input logits", b * c * hw), *xs, _strided_f32(t, "target logits", b * c * hw), *ts,
            b, c, hw, cfg[5], cfg[6], cfg[7], cfg[8], _T(ws, "workspace", dtype=torch.float64, numel=nbytes // 8), nbytes,
            _T(stats, "statistics", dtype=torch.float64, numel=nd * len(CONF_CE_STATS)), _f32(loss, "loss", nd))
    return x, t, stats, loss, cfg


def _conf_backward(x, t, stats, cfg, g, want_t):
    """-> (g_x, g_t or None): each with its tensor's strides.  `g`: the upstream scalar of each slot, on the device"""
    b, c, hw, xs, ts, threshold, threshold_neg, temperature, pair = cfg
    nd = pair + 1
    g_x = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=x.device)
    g_t = torch.empty_strided(t.shape, t.stride(), dtype=torch.float32, device=t.device) if (want_t or pair) else None
    _launch("vqseg_conf_ce_backward_f", x.device, _strided_f32(x, "input logits", b * c * hw), *xs, _strided_f32(t, "target logits", b * c * hw), *ts,
            b, c, hw, threshold, threshold_neg, temperature, pair, int(not want_t),
            _T(stats, "statistics", dtype=torch.float64, numel=nd * len(CONF_CE_STATS)), _f32(g, "loss gradient", nd),
            _strided_f32(g_x, "input gradient", b * c * hw), _strided_f32(g_t, "target gradient", b * c * hw))
    return g_x, g_t


class _ConfCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, threshold, threshold_neg, temperature, detach_targets):
        xd, td, stats, loss, cfg = _conf_forward(x, t, threshold, threshold_neg, temperature, False)
        ctx.save_for_backward(xd, td, stats)
        ctx.cfg, ctx.detach = cfg, bool(detach_targets)
        return loss[0]

    @staticmethod
    def backward(ctx, g_out):
        xd, td, stats = ctx.saved_tensors
        g = g_out.detach().float().reshape(1).contiguous()       # stays on the device: this is where a weight on the term enters
        g_x, g_t = _conf_backward(xd, td, stats, ctx.cfg, g, not ctx.detach and ctx.needs_input_grad[1])
        return g_x, g_t, None, None, None, None


class _ConfCEPair(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, threshold, threshold_neg, temperature, detach_targets):
        ad, bd, stats, loss, cfg = _conf_forward(a, b, threshold, threshold_neg, temperature, True)
        ctx.save_for_backward(ad, bd, stats)
        ctx.cfg, ctx.detach = cfg, bool(detach_targets)
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g_ab, g_ba):
        ad, bd, stats = ctx.saved_tensors
        g = torch.stack([g_ab.detach().float().reshape(()), g_ba.detach().float().reshape(())])
        g_a, g_b = _conf_backward(ad, bd, stats, ctx.cfg, g, not ctx.detach)
        return g_a, g_b, None, None, None, None


def conf_ce(x, t, threshold=0.6, threshold_neg=0.0, temperature=1.0, detach_targets=False):
    """conf_ce_loss of input logits x against target LOGITS t (both pass conf_ce_supported): a 0-d float32 tensor.  The targets are
    not detached unless asked: their gradient is the path through the per-pixel weight max softmax(t).  M == 0 gives an attached 0
    with zero gradients, Mn == 0 a zero negative term (include/vqseg.h)."""
    return _ConfCE.apply(x, t, threshold, threshold_neg, temperature, detach_targets)


def conf_ce_pair(a, b, threshold=0.6, threshold_neg=0.0, temperature=1.0, detach_targets=False):
    """(conf_ce(a <- b), conf_ce(b <- a)): one forward launch reads a and b once for both directions, one backward launch writes both
    gradients, each the sum over the two directions scaled by that direction's own upstream scalar (read on the device).  Bit for bit
    the values of two conf_ce calls, and with unit upstream scalars their summed gradients."""
    return _ConfCEPair.apply(a, b, threshold, threshold_neg, temperature, detach_targets)


def conf_ce_stats(x, t, threshold=0.6, threshold_neg=0.0, temperature=1.0, pair=False):
    """the forward's statistics record, (1 or 2, 8) float64 on the device with the columns CONF_CE_STATS, no gradient (tests, profiles)"""
    return _conf_forward(x, t, threshold, threshold_neg, temperature, pair)[2]


class _ConvBias(torch.autograd.Function):
    """k x k / stride 1 convolution WITH bias and a handful of output channels, fp32 (the plain Unet's segmentation head: 32 -> 3,
    segmentation_head.py:78-83) on the precise-mode kernels: output channels zero-padded to the kernels' 4-channel granule, the bias in
    the convolution's fused epilogue (vqseg_conv2d_affine_f: scale 1, shift = bias); backward = the data-gradient / weight-gradient
    kernels on the padded gradient, the bias gradient a plain sum."""

    @staticmethod
    def forward(ctx, x, weight, bias, pad):
        xr = _rows(x.float())
        n, h, w, cin = xr.shape
        cout, _, kh, kw = weight.shape
        cp = (cout + 3) // 4 * 4
        dev = xr.device
        wp = torch.zeros(cp, cin, kh, kw, dtype=torch.float32, device=dev)
        wp[:cout] = weight.detach()
        shift = torch.zeros(cp, dtype=torch.float32, device=dev)
        if bias is not None:
            shift[:cout] = bias.detach()
        one = torch.ones(cp, dtype=torch.float32, device=dev)
        L = lib()

        def pack(tr):
            ne = L.vqseg_conv_packed_elems(cp, cin, kh, kw, int(tr))
            hi, lo = torch.empty(ne, dtype=torch.int16, device=dev), torch.empty(ne, dtype=torch.int16, device=dev)
            _launch("vqseg_conv_pack_weights_f32", dev, _f32(wp, "weight", cp * cin * kh * kw), cp, cin, kh, kw, int(tr), _w16(hi, "packed hi", ne),
                    _w16(lo, "packed lo", ne))
            return hi, lo

        g = ConvGeom(n, h, w, cin, cin, cp, kh, kw, 1, pad, False, _out_size(h, kh, 1, pad), _out_size(w, kw, 1, pad))
        y = _conv_affine(xr, None, *pack(False), one, shift, None, False, g, 1)
        ctx.save_for_backward(xr)
        ctx.geom, ctx.cout, ctx.has_bias = g, cout, bias is not None
        ctx.pack = pack
        return y[..., :cout].permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, grad):
        (xr,) = ctx.saved_tensors
        g, cout = ctx.geom, ctx.cout
        n, h, w, cin, cp, kh, kw, pad, ho, wo = g.n, g.h, g.w, g.cin, g.cout, g.kh, g.kw, g.pad, g.ho, g.wo
        dev = xr.device
        L = lib()
        g4 = torch.zeros((n, ho, wo, cp), dtype=torch.float32, device=dev)
        g4[..., :cout] = grad.permute(0, 2, 3, 1)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            t_hi, t_lo = ctx.pack(True)                         # [Cin][kh][kw][cp], taps flipped
            gx = _nchw(_conv_raw(g4, None, t_hi, t_lo, None, _dgrad_geom(g, cin, h, w, kh - 1 - pad)))
        if ctx.needs_input_grad[1]:
            nbytes = L.vqseg_conv2d_wgrad_workspace_bytes(n, h, w, cin, ho, wo, cp, kh, kw)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            gw4 = torch.empty((cp, cin, kh, kw), dtype=torch.float32, device=dev)
            _launch("vqseg_conv2d_wgrad_f", dev, _T(g4, "conv output gradient", bf=0, numel=n * ho * wo * cp),
                    _T(xr, "conv input", bf=0, numel=n * h * w * cin), None, cin, n, h, w, cin, ho, wo, cp, kh, kw, 1, pad, 0, 1, cin, 0, 0,
                    _T(ws, "wgrad workspace", dtype=torch.uint8, numel=nbytes), nbytes, _f32(gw4, "weight gradient", cp * cin * kh * kw))
            gw = gw4[:cout]
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = grad.sum(dim=(0, 2, 3))
        return gx, gw, gb, None


def conv2d_bias(x, weight, bias, padding: int):
    """F.conv2d(x.float(), weight, bias, stride 1, padding) on the HIP kernels (few output channels; fp32 like the reference's head)."""
    return _ConvBias.apply(x, weight, bias, int(padding))


class _CPSCombine(torch.autograd.Function):
    """vqseg_cps_loss_combine_f: total = sup terms + cps_w * cps terms + commitment + prototype from the Dice (+ CE) sums, in one launch,
    with the gradient of the total with respect to every input written in the same launch (backward = one scaling)."""

    @staticmethod
    def forward(ctx, spec, *ts):
        n_sup, n_cps, has_ce, cps_w, ce_w, eps, commit_w, proto_w, n_commit, n_proto = spec
        nt, per = n_sup + n_cps, (3 if has_ce else 2)
        terms = [ts[i * per:(i + 1) * per] for i in range(nt)]
        commits = ts[nt * per: nt * per + n_commit]
        protos = ts[nt * per + n_commit:]
        dev = terms[0][0].device
        c = terms[0][0].shape[1]
        bs = [int(t[0].shape[0]) for t in terms]
        levels = int(commits[0].numel()) if commits else 0
        sizes = []
        for b in bs:
            sizes += [b * c, b * c] + ([b * 2] if has_ce else [])
        gbuf = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
        views = list(torch.split(gbuf, sizes))
        out = torch.empty(4 + nt, dtype=torch.float32, device=dev)
        P4 = ctypes.c_void_p * 4

        def arr(tensors, what, dtype=torch.float32):
            a = P4()
            for i, t in enumerate(tensors):
                a[i] = _hip.on_gpu(_T(t, what, dtype=dtype))
            return a

        inter = arr([t[0] for t in terms], "intersections")
        sets = arr([t[1] for t in terms], "set sizes")
        ce = arr([t[2] for t in terms], "cross-entropy sums") if has_ce else None
        g_inter = arr(views[0::per], "gradient of the intersections")
        g_sets = arr(views[1::per], "gradient of the set sizes")
        g_ce = arr(views[2::per], "gradient of the cross-entropy sums") if has_ce else None
        b_arr = (ctypes.c_int * 4)(*(bs + [0] * (4 - nt)))
        _launch("vqseg_cps_loss_combine_f", dev, n_sup, n_cps, c, inter, sets, ce, b_arr, float(cps_w), float(ce_w), float(eps),
                arr(commits, "commitment losses"), n_commit, levels, float(commit_w), arr(protos, "prototype losses", dtype=torch.float64), n_proto,
                float(proto_w), g_inter, g_sets, g_ce, _f32(out, "loss terms", 4 + nt))
        ctx.gbuf, ctx.sizes, ctx.shapes = gbuf, sizes, [tuple(x.shape) for t in terms for x in t]
        ctx.tail = (n_commit, n_proto, levels, float(commit_w), float(proto_w), [tuple(x.shape) for x in commits])
        total = out[0].clone()
        ctx.mark_non_differentiable(out)
        return total, out

    @staticmethod
    def backward(ctx, g, _g_stats):
        n_commit, n_proto, levels, commit_w, proto_w, cshapes = ctx.tail
        gb = ctx.gbuf * g
        grads = [v.reshape(sh) for v, sh in zip(torch.split(gb, ctx.sizes), ctx.shapes)]
        gc = (g * commit_w)
        gp = (g.double() * proto_w)
        return (None, *grads, *[gc.expand(sh) for sh in cshapes], *[gp for _ in range(n_proto)])


def cps_loss_combine(sup_terms, cps_terms, cps_weight, ce_weight, commits, commit_weight, protos, proto_weight, eps=1e-6):
    """-> (total, stats) with stats = [total, commitment, prototype, cps_1 + cps_2, sup_1, .., cps_1, ..] (no gradient through stats).
    `sup_terms` / `cps_terms`: lists of (inter, sets) or (inter, sets, ce) from dice_sums / dice_ce_sums; `commits`: fp32 vectors of
    one length; `protos`: float64 scalars.  None when the inputs are not what the kernel takes (the caller combines with torch ops)."""
    terms = list(sup_terms) + list(cps_terms)
    if not terms or len(terms) > 4 or len(commits) > 4 or len(protos) > 4 or not py_opt("py_loss_combine", 1):
        return None
    has_ce = len(terms[0]) == 3
    flat = []
    for t in terms:
        if len(t) != (3 if has_ce else 2) or not all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() for x in t):
            return None
        if t[0].dim() != 2 or t[0].shape != t[1].shape or t[0].shape[1] != terms[0][0].shape[1] or (has_ce and tuple(t[2].shape) != (t[0].shape[0], 2)):
            return None
        flat += list(t)
    if not all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 1 and x.shape == commits[0].shape for x in commits):
        return None
    if not all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float64 and x.numel() == 1 for x in protos):
        return None
    spec = (len(sup_terms), len(cps_terms), has_ce, float(cps_weight), float(ce_weight), float(eps), float(commit_weight), float(proto_weight),
            len(commits), len(protos))
    return _CPSCombine.apply(spec, *flat, *commits, *protos)


def softmax_stats(logits, want_label=True, want_entropy=True, want_top=False):
    """(label (B, H, W) i64, entropy (B, H, W) f32, top-probability (B, H, W) f32) of softmax(logits, dim=1) in one HIP pass
    (None for outputs not wanted).  No gradient flows (the callers detach / use them as masks and targets)."""
    x = logits.detach()
    if x.dtype != torch.float32:
        x = x.float()
    b, c, h, w = x.shape
    sb, sc, sh, sw = x.stride()
    if sh != w * sw:
        x = x.contiguous()
        sb, sc, sh, sw = x.stride()
    dev = x.device
    label = torch.empty((b, h, w), dtype=torch.int64, device=dev) if want_label else None
    ent = torch.empty((b, h, w), dtype=torch.float32, device=dev) if want_entropy else None
    top = torch.empty((b, h, w), dtype=torch.float32, device=dev) if want_top else None
    _launch("vqseg_softmax_stats_f", dev, _strided_f32(x, "logits", b * c * h * w), sb, sc, sw, b, c, h * w,
            _T(label, "labels", dtype=torch.int64, numel=b * h * w), _f32(ent, "entropy", b * h * w), _f32(top, "top probability", b * h * w))
    return label, ent, top


def percentile(values, percent: float):
    """np.percentile(values, percent) (linear interpolation) as a 0-d device tensor, for any number of fp32 values below 2^32:
    the two order statistics around the virtual index come from an exact radix select (vqseg_order_stats_f) instead of a
    full sort, and the index is taken in double as numpy does (torch.quantile rounds it to fp32)."""
    x = values.detach().reshape(-1)
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.float().contiguous()
    n = x.numel()
    virtual = percent / 100.0 * (n - 1)
    k = min(max(int(virtual), 0), n - 1)
    ws = torch.empty(lib().vqseg_order_stats_workspace_bytes(), dtype=torch.uint8, device=x.device)
    out = torch.empty(2, dtype=torch.float32, device=x.device)
    _launch("vqseg_order_stats_f", x.device, _f32(x, "values", n), n, k, _T(ws, "workspace", dtype=torch.uint8), ws.numel(),
            _f32(out, "order statistics", 2))
    frac = virtual - k
    if frac <= 0.0:
        return out[0]
    return torch.lerp(out[0], out[1], frac)


def softmax_stats_supported(logits) -> bool:
    return logits.is_cuda and logits.dim() == 4 and 2 <= logits.shape[1] <= 4


# ------------------------------------------------------------------------------------------------
# prediction: resize + mean over views + arg-max (+ top probability, confusion counts) in one pass
# ------------------------------------------------------------------------------------------------
FLIP_DIMS = ((), (3,), (2,), (2, 3))          # flip code -> dims of an (N, C, H, W) tensor: bit 0 columns, bit 1 rows
RESIZE_ARGMAX_CALLS = 0                       # calls that reached the library (for tests, never read by the product)


def _resize_argmax_torch(views, flips, size, want_top, target):
    """resize_argmax with torch ops, for tensors that are not on the GPU"""
    acc = None
    for v, f in zip(views, flips):
        r = F.interpolate(v.flip(FLIP_DIMS[f]) if f else v, size=size, mode="bilinear", align_corners=False)
        acc = r if acc is None else acc + r
    if len(views) > 1:
        acc = acc * (1.0 / len(views))
    b, c = acc.shape[:2]
    label = acc.argmax(dim=1)
    top = torch.softmax(acc, dim=1).max(dim=1).values if want_top else None
    counts = None
    if target is not None:
        t = target.reshape(b, -1)
        cats = c * t + label.reshape(b, -1) + (c * c) * torch.arange(b, device=t.device)[:, None]
        counts = torch.bincount(cats[(t >= 0) & (t < c)], minlength=b * c * c).reshape(b, c, c)
    return label.to(torch.uint8), top, counts


def resize_argmax(logits, size, flips=None, want_top=False, target=None):
    """(label (B, Ho, Wo) u8, top probability (B, Ho, Wo) f32 | None, confusion counts (B, C, C) i64 | None) of the logits resized
    bilinearly (align_corners=False) to `size`, in one HIP pass without the (B, C, Ho, Wo) tensor (vqseg_resize_argmax_f).  `logits`:
    one (B, C, H, W) fp32 tensor or a list of 1, 2 or 4 of them ("views": the networks of an ensemble, flipped test-time views),
    NCHW-contiguous or channels_last; `flips`: one code per view (bit 0 columns, bit 1 rows) that is undone before the resize.  The
    views' resized logits are summed in order and scaled by 1 / V; label is the first maximum, top its softmax probability, counts
    (with `target` (B, Ho, Wo), any integer type; rows = ground truth, targets outside [0, C) skipped) the per-image confusion
    matrix.  With one view it equals softmax_stats / confusion_matrix_device on upsample_bilinear(logits, size) bit for bit.
    Tensors that are not on the GPU are computed with torch ops (F.interpolate, torch.flip).  No gradient flows."""
    global RESIZE_ARGMAX_CALLS
    E = _hip.HipLibraryError
    views = [logits] if torch.is_tensor(logits) else list(logits)
    nv = len(views)
    if nv not in (1, 2, 4):
        raise E(f"resize_argmax: 1, 2 or 4 views (the mean's 1 / V must be exact), got {nv}")
    flips = [0] * nv if flips is None else [int(f) for f in flips]
    if len(flips) != nv:
        raise E(f"resize_argmax: one flip code per view required: {nv} views, {len(flips)} codes")
    if any(f < 0 or f > 3 for f in flips):
        raise E(f"resize_argmax: a flip code is 0..3 (bit 0 columns, bit 1 rows), got {flips}")
    if not all(torch.is_tensor(v) and v.dim() == 4 for v in views):
        raise E("resize_argmax: every view must be a (B, C, H, W) tensor")
    x0 = views[0]
    if any(v.shape != x0.shape or v.device != x0.device for v in views):
        raise E(f"resize_argmax: every view must have view 0's shape and device, got shapes {[tuple(v.shape) for v in views]}")
    b, c, h, w = x0.shape
    if not 2 <= c <= 4:
        raise E(f"resize_argmax: 2..4 classes, got {c}")
    ho, wo = int(size[0]), int(size[1])
    if min(b, h, w, ho, wo) < 1:
        raise E("resize_argmax: empty input or output")
    # one layout for all views: view 0's if it is dense (NCHW-contiguous or channels_last), else NCHW
    fmt = torch.contiguous_format if x0.is_contiguous() or not x0.is_contiguous(memory_format=torch.channels_last) else torch.channels_last
    views = [v.detach() for v in views]
    views = [v if v.is_contiguous(memory_format=fmt) else v.contiguous(memory_format=fmt) for v in views]
    ptrs = [_strided_f32(v, "logits" if nv == 1 else f"logits (view {i})", b * c * h * w) for i, v in enumerate(views)]
    tgt = None
    if target is not None:
        if not torch.is_tensor(target) or target.dtype.is_floating_point or target.dtype.is_complex or target.dtype == torch.bool:
            raise E(f"resize_argmax: target must be an integer tensor, got {getattr(target, 'dtype', type(target).__name__)}")
        if tuple(target.shape) != (b, ho, wo):
            raise E(f"resize_argmax: target must have the output's shape {(b, ho, wo)}, got {tuple(target.shape)}")
        tgt = target.detach().long().contiguous()
    dev = x0.device
    if not x0.is_cuda:
        return _resize_argmax_torch(views, flips, (ho, wo), want_top, tgt)
    label = torch.empty((b, ho, wo), dtype=torch.uint8, device=dev)
    top = torch.empty((b, ho, wo), dtype=torch.float32, device=dev) if want_top else None
    counts = torch.empty((b, c, c), dtype=torch.int64, device=dev) if tgt is not None else None
    varr, farr = (ctypes.c_void_p * 4)(), (ctypes.c_int * 4)(*(flips + [0] * (4 - nv)))
    for i, p in enumerate(ptrs):
        varr[i] = _hip.on_gpu(p)
    # tptr admits two dense layouts; the strides are stated from the layout (a size-1 dimension's own stride is arbitrary)
    strides = (c * h * w, h * w, 1) if fmt == torch.contiguous_format else (c * h * w, 1, c)
    _launch("vqseg_resize_argmax_f", dev, varr, farr, nv, *strides, b, c, h, w, ho, wo, _T(label, "labels", dtype=torch.uint8, numel=b * ho * wo),
            _f32(top, "top probability", b * ho * wo), _T(tgt, "target", dtype=torch.int64, numel=b * ho * wo),
            _T(counts, "confusion counts", dtype=torch.int64, numel=b * c * c))
    RESIZE_ARGMAX_CALLS += 1
    return label, top, counts


# ------------------------------------------------------------------------------------------------
# tiled prediction: windows of the images -> network inputs; window logits -> blended arg-max
# ------------------------------------------------------------------------------------------------
BLENDS = {"uniform": 0, "linear": 1}          # include/vqseg.h: VQSEG_BLEND_*
MAX_WINDOW = 4096
EXTRACT_WINDOWS_CALLS = 0                     # calls that reached the library (for tests, never read by the product)
MERGE_ARGMAX_CALLS = 0

# what extract_windows hands out and merge_argmax takes back: the images' batch and size, the window and stride in image pixels,
# the windows per axis and the size the network sees
WindowGrid = namedtuple("WindowGrid", "batch height width window stride ny nx net_size")


def window_starts(extent, window, stride):
    """the starts of the windows along one axis: n = ceil((extent - window) / stride) + 1, start[k] = min(k * stride, extent - window).
    The last window is clamped to end at the border.  The kernels derive the same starts from (extent, window, stride)."""
    extent, window, stride = int(extent), int(window), int(stride)
    if not 1 <= stride <= window <= extent:
        raise ValueError(f"window_starts: 1 <= stride <= window <= extent required, got stride {stride}, window {window}, extent {extent}")
    n = -((window - extent) // stride) + 1
    return [min(k * stride, extent - window) for k in range(n)]


def _pair(v, what, E):
    try:
        h, w = (int(v), int(v)) if isinstance(v, int) else (int(v[0]), int(v[1]))
    except (TypeError, ValueError, IndexError):
        raise E(f"{what} must be an int or a (h, w) pair, got {v!r}") from None
    return h, w


def _window_grid(batch, height, width, window, stride, net_size, who):
    """the checked WindowGrid of a batch of `height` x `width` images"""
    E = _hip.HipLibraryError
    wh, ww = _pair(window, f"{who}: window", E)
    sy, sx = (max(wh // 2, 1), max(ww // 2, 1)) if stride is None else _pair(stride, f"{who}: stride", E)
    nh, nw = (wh, ww) if net_size is None else _pair(net_size, f"{who}: net_size", E)
    if min(wh, ww, sy, sx, nh, nw) < 1:
        raise E(f"{who}: window, stride and net_size must be positive, got {(wh, ww)}, {(sy, sx)}, {(nh, nw)}")
    if wh > height or ww > width:
        raise E(f"{who}: a window of {(wh, ww)} is larger than the image of {(height, width)} (no padding)")
    if sy > wh or sx > ww:
        raise E(f"{who}: a stride of {(sy, sx)} larger than the window of {(wh, ww)} leaves pixels uncovered")
    if max(wh, ww) > MAX_WINDOW:
        raise E(f"{who}: a window side above {MAX_WINDOW}, got {(wh, ww)}")
    return WindowGrid(int(batch), int(height), int(width), (wh, ww), (sy, sx), len(window_starts(height, wh, sy)),
                      len(window_starts(width, ww, sx)), (nh, nw))


def _extract_windows_torch(images, grid, flips):
    wh, ww = grid.window
    crops = []
    for b in range(grid.batch):
        for y0 in window_starts(grid.height, wh, grid.stride[0]):
            for x0 in window_starts(grid.width, ww, grid.stride[1]):
                crops.append(images[b, :, y0:y0 + wh, x0:x0 + ww])
    rows = torch.stack(crops)
    if grid.net_size != grid.window:
        rows = F.interpolate(rows, size=grid.net_size, mode="bilinear", align_corners=False)
    return torch.stack([rows.flip(FLIP_DIMS[f]) if f else rows for f in flips])


def extract_windows(images, window, stride=None, net_size=None, flips=(0,)):
    """(windows (F, B * T, 3, nh, nw) f32, grid): every window of the window rule (window_starts; `window` and `stride` an int or
    (h, w) in image pixels, stride default window // 2) cropped from `images` (B, 3, H, W) fp32, NCHW-contiguous or channels_last,
    resized bilinearly (align_corners=False, taps clamped inside the window; ATen's un-antialiased rule when it shrinks) to
    `net_size` (default: the window, an exact copy) and flipped by each code of `flips` (1..4 codes 0..3: bit 0 columns, bit 1 rows)
    -- one HIP launch (vqseg_extract_windows_f).  Window rows are image-major, a grid row-major: row = b * T + j * nx + i.  Entry f
    equals nnf.upsample_bilinear(crop, net_size).flip(dims of flips[f]) bit for bit.  `grid` is the WindowGrid merge_argmax takes
    back.  Tensors that are not on the GPU are computed with torch ops.  No gradient flows."""
    global EXTRACT_WINDOWS_CALLS
    E = _hip.HipLibraryError
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[1] != 3:
        raise E(f"extract_windows: images must be a (B, 3, H, W) tensor, got {tuple(getattr(images, 'shape', ()))}")
    flips = [int(f) for f in flips]
    if not 1 <= len(flips) <= 4:
        raise E(f"extract_windows: 1..4 flip codes, got {len(flips)}")
    if any(f < 0 or f > 3 for f in flips):
        raise E(f"extract_windows: a flip code is 0..3 (bit 0 columns, bit 1 rows), got {flips}")
    b, _, h, w = images.shape
    if min(b, h, w) < 1:
        raise E("extract_windows: empty images")
    grid = _window_grid(b, h, w, window, stride, net_size, "extract_windows")
    x = images.detach()
    fmt = torch.contiguous_format if x.is_contiguous() or not x.is_contiguous(memory_format=torch.channels_last) else torch.channels_last
    x = x if x.is_contiguous(memory_format=fmt) else x.contiguous(memory_format=fmt)
    ptr = _strided_f32(x, "images", b * 3 * h * w)
    if not x.is_cuda:
        return _extract_windows_torch(x, grid, flips), grid
    rows, (nh, nw) = b * grid.ny * grid.nx, grid.net_size
    out = torch.empty((len(flips), rows, 3, nh, nw), dtype=torch.float32, device=x.device)
    farr = (ctypes.c_int * 4)(*(flips + [0] * (4 - len(flips))))
    strides = (3 * h * w, h * w, 1) if fmt == torch.contiguous_format else (3 * h * w, 1, 3)
    _launch("vqseg_extract_windows_f", x.device, ptr, *strides, b, h, w, *grid.window, *grid.stride, nh, nw, farr, len(flips),
            _f32(out, "windows", out.numel()))
    EXTRACT_WINDOWS_CALLS += 1
    return out, grid


def _merge_argmax_torch(views, flips, grid, linear, want_top, target):
    """merge_argmax with torch ops, for tensors that are not on the GPU"""
    (wh, ww), (sy, sx), T = grid.window, grid.stride, grid.ny * grid.nx
    c = views[0].shape[1]
    ry, rx = torch.arange(wh, dtype=torch.float32), torch.arange(ww, dtype=torch.float32)
    wgt = (torch.minimum(ry + 1, wh - ry)[:, None] * torch.minimum(rx + 1, ww - rx)[None, :]) if linear else torch.ones(wh, ww)
    wgt = wgt.to(views[0].device)
    ys, xs = window_starts(grid.height, wh, sy), window_starts(grid.width, ww, sx)
    z = None
    for v, f in zip(views, flips):
        s = F.interpolate(v.flip(FLIP_DIMS[f]) if f else v, size=(wh, ww), mode="bilinear", align_corners=False)
        s = s.reshape(grid.batch, T, c, wh, ww)
        acc = torch.zeros((grid.batch, c, grid.height, grid.width), dtype=torch.float32, device=v.device)
        ws = torch.zeros((grid.height, grid.width), dtype=torch.float32, device=v.device)
        for j, y0 in enumerate(ys):
            for i, x0 in enumerate(xs):
                acc[:, :, y0:y0 + wh, x0:x0 + ww] += wgt * s[:, j * grid.nx + i]
                ws[y0:y0 + wh, x0:x0 + ww] += wgt
        m = acc / ws
        z = m if z is None else z + m
    if len(views) > 1:
        z = z * (1.0 / len(views))
    b = grid.batch
    label = z.argmax(dim=1)
    top = torch.softmax(z, dim=1).max(dim=1).values if want_top else None
    counts = None
    if target is not None:
        t = target.reshape(b, -1)
        cats = c * t + label.reshape(b, -1) + (c * c) * torch.arange(b, device=t.device)[:, None]
        counts = torch.bincount(cats[(t >= 0) & (t < c)], minlength=b * c * c).reshape(b, c, c)
    return label.to(torch.uint8), top, counts


def merge_argmax(views, grid, flips=None, blend="linear", want_top=False, target=None):
    """(label (B, H, W) u8, top probability (B, H, W) f32 | None, confusion counts (B, C, C) i64 | None) of the images whose windows
    (`grid`, as extract_windows returned it) went through the network: `views` is one (B * T, C, lh, lw) fp32 logit tensor or a list of
    1, 2 or 4 of them with one flip code each (`flips`: undone as an index map).  Per pixel and view, the windows that hold the pixel
    are summed in grid order, each resized bilinearly (align_corners=False) from (lh, lw) to the window's extent and weighted by
    `blend` -- "uniform": 1, "linear": min(r + 1, window - r) along each axis, so a window counts least at its border -- and divided
    by the weights' sum; the views' means are averaged, label is the first maximum, top its softmax probability, counts (with
    `target` (B, H, W), any integer type) the per-image confusion matrix -- in one HIP pass (vqseg_merge_argmax_f), without the
    (B, C, H, W) logit tensor.  With one window per image and "uniform" it equals resize_argmax bit for bit.  Tensors that are
    not on the GPU are computed with torch ops.  No gradient flows."""
    global MERGE_ARGMAX_CALLS
    E = _hip.HipLibraryError
    views = [views] if torch.is_tensor(views) else list(views)
    nv = len(views)
    if nv not in (1, 2, 4):
        raise E(f"merge_argmax: 1, 2 or 4 views (the mean's 1 / V must be exact), got {nv}")
    flips = [0] * nv if flips is None else [int(f) for f in flips]
    if len(flips) != nv:
        raise E(f"merge_argmax: one flip code per view required: {nv} views, {len(flips)} codes")
    if any(f < 0 or f > 3 for f in flips):
        raise E(f"merge_argmax: a flip code is 0..3 (bit 0 columns, bit 1 rows), got {flips}")
    if blend not in BLENDS:
        raise E(f"merge_argmax: blend is one of {sorted(BLENDS)}, got {blend!r}")
    if not isinstance(grid, WindowGrid):
        raise E(f"merge_argmax: grid must be the WindowGrid extract_windows returned, got {type(grid).__name__}")
    grid = _window_grid(grid.batch, grid.height, grid.width, grid.window, grid.stride, grid.net_size, "merge_argmax")
    if not all(torch.is_tensor(v) and v.dim() == 4 for v in views):
        raise E("merge_argmax: every view must be a (B * T, C, lh, lw) tensor")
    x0 = views[0]
    if any(v.shape != x0.shape or v.device != x0.device for v in views):
        raise E(f"merge_argmax: every view must have view 0's shape and device, got shapes {[tuple(v.shape) for v in views]}")
    n, c, lh, lw = x0.shape
    b, ho, wo = grid.batch, grid.height, grid.width
    if not 2 <= c <= 4:
        raise E(f"merge_argmax: 2..4 classes, got {c}")
    if min(b, lh, lw) < 1:
        raise E("merge_argmax: empty input")
    if n != b * grid.ny * grid.nx:
        raise E(f"merge_argmax: the grid has {b} x {grid.ny} x {grid.nx} = {b * grid.ny * grid.nx} windows, the views have {n} rows")
    fmt = torch.contiguous_format if x0.is_contiguous() or not x0.is_contiguous(memory_format=torch.channels_last) else torch.channels_last
    views = [v.detach() for v in views]
    views = [v if v.is_contiguous(memory_format=fmt) else v.contiguous(memory_format=fmt) for v in views]
    ptrs = [_strided_f32(v, "window logits" if nv == 1 else f"window logits (view {i})", n * c * lh * lw) for i, v in enumerate(views)]
    tgt = None
    if target is not None:
        if not torch.is_tensor(target) or target.dtype.is_floating_point or target.dtype.is_complex or target.dtype == torch.bool:
            raise E(f"merge_argmax: target must be an integer tensor, got {getattr(target, 'dtype', type(target).__name__)}")
        if tuple(target.shape) != (b, ho, wo):
            raise E(f"merge_argmax: target must have the output's shape {(b, ho, wo)}, got {tuple(target.shape)}")
        tgt = target.detach().long().contiguous()
    dev = x0.device
    if not x0.is_cuda:
        return _merge_argmax_torch(views, flips, grid, blend == "linear", want_top, tgt)
    label = torch.empty((b, ho, wo), dtype=torch.uint8, device=dev)
    top = torch.empty((b, ho, wo), dtype=torch.float32, device=dev) if want_top else None
    counts = torch.empty((b, c, c), dtype=torch.int64, device=dev) if tgt is not None else None
    varr, farr = (ctypes.c_void_p * 4)(), (ctypes.c_int * 4)(*(flips + [0] * (4 - nv)))
    for i, p in enumerate(ptrs):
        varr[i] = _hip.on_gpu(p)
    strides = (c * lh * lw, lh * lw, 1) if fmt == torch.contiguous_format else (c * lh * lw, 1, c)
    _launch("vqseg_merge_argmax_f", dev, varr, farr, nv, *strides, b, c, lh, lw, ho, wo, *grid.window, *grid.stride, BLENDS[blend],
            _T(label, "labels", dtype=torch.uint8, numel=b * ho * wo), _f32(top, "top probability", b * ho * wo),
            _T(tgt, "target", dtype=torch.int64, numel=b * ho * wo), _T(counts, "confusion counts", dtype=torch.int64, numel=b * c * c))
    MERGE_ARGMAX_CALLS += 1
    return label, top, counts



# ------------------------------------------------------------------------------------------------
# visualisation: labels, targets and the input image -> the RGB bytes of a panel sheet in one pass
# ------------------------------------------------------------------------------------------------
def sheet_layout(panels, wo):
    """-> ([(kind, x0, width)], sheet width) of panels laid out left to right: a panel is a kind name of _hip.RENDER_KINDS (`wo` wide) or
    ("fill", width)"""
    rows, x = [], 0
    for p in panels:
        kind, width = (p, None) if isinstance(p, str) else (p[0], p[1] if len(p) > 1 else None)
        if kind not in _hip.RENDER_KINDS:
            raise _hip.HipLibraryError(f"render_sheet: panel kinds are {sorted(_hip.RENDER_KINDS)}, got {kind!r}")
        if kind == "fill":
            if width is None or int(width) < 1:
                raise _hip.HipLibraryError("render_sheet: a fill panel is ('fill', width) with a positive width")
            width = int(width)
        elif width is not None and int(width) != wo:
            raise _hip.HipLibraryError(f"render_sheet: every panel but 'fill' is as wide as the display size ({wo}), got {width}")
        else:
            width = wo
        rows.append((kind, x, width))
        x += width
    if not rows:
        raise _hip.HipLibraryError("render_sheet: no panels")
    return rows, x


def render_sheet(panels, size, num_classes, palette, image=None, pred=None, target=None, fill=(1.0, 1.0, 1.0), alpha=0.4, half=False,
                 out=None):
    """The panel sheet of a batch as uint8 RGB, (B * Ho, sheet width, 3) -- with `half` (B * Ho / 2, sheet width / 2, 3), every pixel
    the mean of a 2 x 2 block of the full sheet -- in one HIP pass (vqseg_render_sheet_u8).  `panels`, left to right: "image" (the
    input resized bilinearly, align_corners=False, to `size` = (Ho, Wo)), "target", "pred", "detail" (a wrong pixel takes the
    palette's second block), "mix_pred" / "mix_detail" (clip((1 - alpha) image + alpha colour, 0, 1)), ("fill", width).  `pred`:
    (B, Ho, Wo) uint8 labels as resize_argmax writes them; `target`: (B, Ht, Wt) integer labels at any size (nearest neighbour);
    `image`: (B, 3, h, w) fp32.  `palette`: (2 C + 1, 3) floats.  `out`: a (rows, cols, 3) uint8 tensor to write into, which may be a
    view of a larger canvas (dense pixels, any row pitch); bytes outside the panels are not touched.  Image i takes the rows
    i Ho .. (i + 1) Ho - 1 of every panel.  Tensors must be on the GPU."""
    E = _hip.HipLibraryError
    ho, wo = int(size[0]), int(size[1])
    rows, cols = sheet_layout(panels, wo)
    src = next((t for t in (pred, image, target, out) if torch.is_tensor(t)), None)
    if src is None:
        raise E("render_sheet: at least one of image, pred, target or out must be a tensor (it names the batch and the device)")
    b = int(pred.shape[0] if torch.is_tensor(pred) else image.shape[0] if torch.is_tensor(image) else target.shape[0] if torch.is_tensor(target)
            else (out.shape[0] * (2 if half else 1)) // ho)
    if half and ((b * ho) % 2 or cols % 2):
        raise E(f"render_sheet: half needs a sheet of even height and width, got {b * ho} x {cols}")
    shape = (b * ho // 2, cols // 2, 3) if half else (b * ho, cols, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=src.device)
    elif not torch.is_tensor(out) or tuple(out.shape) != shape:
        raise E(f"render_sheet: out must have the shape {shape}, got {tuple(getattr(out, 'shape', ()))}")
    if torch.is_tensor(image):
        image = image.detach()
        if image.dtype == torch.float32 and image.dim() == 4 and not image.is_contiguous() and not image.is_contiguous(memory_format=torch.channels_last):
            image = image.contiguous()
    if target is not None:
        if not torch.is_tensor(target) or target.dtype.is_floating_point or target.dtype.is_complex or target.dtype == torch.bool:
            raise E(f"render_sheet: target must be an integer tensor, got {getattr(target, 'dtype', type(target).__name__)}")
        target = target.detach().long().contiguous()
    if pred is not None and torch.is_tensor(pred):
        pred = pred.detach().contiguous()
    return _hip.render_sheet(out, rows, (b, ho, wo), num_classes, palette, fill=fill, image=image, pred=pred, target=target, alpha=alpha,
                             box2=half, cols=cols)


# ------------------------------------------------------------------------------------------------
# dense-CRF refinement of class probabilities: exact mean-field on a truncated support (vqseg_crf_prepare_f, vqseg_crf_step_f)
# ------------------------------------------------------------------------------------------------
CRF_MAX_SIDE = 2048                           # include/vqseg.h: squared pixel distances stay exact f32 integers
CRF_DEFAULTS = dict(iter_max=10, bi_w=7.0, bi_xy_std=50.0, bi_rgb_std=4.0, pos_w=3.0, pos_xy_std=3.0, truncate=4.0)     # utils/crf.py:6


def crf_settings(iter_max=10, bi_w=7.0, bi_xy_std=50.0, bi_rgb_std=4.0, pos_w=3.0, pos_xy_std=3.0, truncate=4.0, who="dense_crf"):
    """the checked settings of a dense CRF as (iter_max, bi_w, bi_xy_std, bi_rgb_std, pos_w, pos_xy_std, truncate); truncate None
    (full support) comes back as +inf.  One rule for nnf.dense_crf and utils.crf.DenseCRF."""
    if isinstance(iter_max, bool) or int(iter_max) != iter_max or int(iter_max) < 0:
        raise ValueError(f"{who}: iter_max must be an integer >= 0, got {iter_max!r}")
    vals = [float(bi_w), float(bi_xy_std), float(bi_rgb_std), float(pos_w), float(pos_xy_std)]
    for name, v in zip(("bi_xy_std", "bi_rgb_std", "pos_xy_std"), (vals[1], vals[2], vals[4])):
        if not 0.0 < v <= 1e18:
            raise ValueError(f"{who}: {name} must be positive (and at most 1e18), got {v}")
    for name, v in zip(("bi_w", "pos_w"), (vals[0], vals[3])):
        if not abs(v) <= 1e18:
            raise ValueError(f"{who}: {name} must be finite, got {v}")
    t = float("inf") if truncate is None else float(truncate)
    if not t >= 0.0:
        raise ValueError(f"{who}: truncate must be >= 0 or None (full support), got {truncate!r}")
    return (int(iter_max), *vals, t)


def dense_crf_supported(images, probs) -> bool:
    """what the kernels take: float32 GPU tensors images (B, 3, H, W) and probs (B, C, H, W) of one batch, size and device, 2..4
    classes, sides up to CRF_MAX_SIDE, at most 65535 images"""
    return (torch.is_tensor(images) and torch.is_tensor(probs) and images.is_cuda and probs.device == images.device and images.dim() == 4
            and probs.dim() == 4 and images.dtype == torch.float32 and probs.dtype == torch.float32 and images.shape[1] == 3
            and 2 <= probs.shape[1] <= 4 and images.shape[0] == probs.shape[0] and images.shape[2:] == probs.shape[2:]
            and 1 <= probs.shape[0] <= 65535 and 1 <= probs.shape[2] <= CRF_MAX_SIDE and 1 <= probs.shape[3] <= CRF_MAX_SIDE)


def _crf_dense(v):
    """dense NCHW or channels_last storage and its (batch, channel, pixel) strides, stated from the layout"""
    v = v.detach()
    if not (v.is_contiguous() or v.is_contiguous(memory_format=torch.channels_last)):
        v = v.contiguous()
    b, c, h, w = v.shape
    return v, ((c * h * w, h * w, 1) if v.is_contiguous() else (c * h * w, 1, c))


def dense_crf(images, probs, iter_max=10, bi_w=7.0, bi_xy_std=50.0, bi_rgb_std=4.0, pos_w=3.0, pos_xy_std=3.0, truncate=4.0, out="prob"):
    """Fully connected CRF refinement (utils/crf.py: DenseCRF) of class probabilities `probs` (B, C, H, W) under `images` (B, 3, H, W)
    in [0, 1], both float32 on the GPU, NCHW-contiguous or channels_last: `iter_max` mean-field updates with a Potts compatibility
    and symmetrically normalised kernels, computed exactly over all pixel pairs with |dx|, |dy| <= R = ceil(truncate * xy_std) of
    each kernel (`truncate` None: all pairs) -- the contract of include/vqseg.h, one prepare launch and one step launch per
    iteration.  `out` "prob": Q (B, C, H, W), NCHW-contiguous; "logits": the last update's energies E, softmax(E) = Q (with
    iter_max = 0: -U = log of the clipped probabilities), which resize_argmax takes at equal size for labels, top probability and
    counts.  No gradient flows.  There is no CPU form here (utils.crf.DenseCRF has one)."""
    E = _hip.HipLibraryError
    if out not in ("prob", "logits"):
        raise ValueError(f"dense_crf: out is 'prob' or 'logits', got {out!r}")
    iters, bi_w, bi_xy_std, bi_rgb_std, pos_w, pos_xy_std, trunc = crf_settings(iter_max, bi_w, bi_xy_std, bi_rgb_std, pos_w, pos_xy_std, truncate)
    if not (torch.is_tensor(images) and torch.is_tensor(probs) and images.dim() == 4 and probs.dim() == 4):
        raise E("dense_crf: images must be a (B, 3, H, W) tensor and probs a (B, C, H, W) tensor")
    b, c, h, w = probs.shape
    if images.shape[1] != 3 or images.shape[0] != b or tuple(images.shape[2:]) != (h, w):
        raise E(f"dense_crf: images must be (B, 3, H, W) of the probabilities' batch and size, got {tuple(images.shape)} and {tuple(probs.shape)}")
    if not 2 <= c <= 4:
        raise E(f"dense_crf: 2..4 classes, got {c}")
    if min(b, h, w) < 1 or b > 65535 or max(h, w) > CRF_MAX_SIDE:
        raise E(f"dense_crf: 1..65535 images with sides of 1..{CRF_MAX_SIDE}, got {tuple(probs.shape)}")
    if images.device != probs.device:
        raise E(f"dense_crf: images and probs must be on one device, got {images.device} and {probs.device}")
    state = _crf_prepare(images, probs, iters, bi_xy_std, bi_rgb_std, pos_xy_std, trunc)
    q, unary = state[0], state[2]
    if iters == 0:
        return q[0] if out == "prob" else unary.neg_()
    for it in range(iters):
        _crf_step(state, it & 1, bi_w, bi_xy_std, bi_rgb_std, pos_w, pos_xy_std, trunc, out == "logits" and it == iters - 1)
    return q[iters & 1]


def _crf_prepare(images, probs, iters, bi_xy_std, bi_rgb_std, pos_xy_std, trunc):
    """one vqseg_crf_prepare_f launch -> (q ping-pong pair (q[0] = Q0), colours, unary, positional norm, bilateral norm): the buffers
    the step launches work on, none larger than the probabilities"""
    b, c, h, w = probs.shape
    images, istr = _crf_dense(images)
    probs, pstr = _crf_dense(probs)
    n, dev = h * w, probs.device
    ip, pp = _strided_f32(images, "images", b * 3 * n), _strided_f32(probs, "probabilities", b * c * n)
    if dev.type != "cuda":                       # before any buffer is asked for on a device that has no HIP path
        _launch("vqseg_crf_prepare_f", dev, ip, *istr, pp, *pstr, b, c, h, w, iters, bi_xy_std, bi_rgb_std, pos_xy_std, trunc,
                None, None, None, None, None, None)
    rgb = torch.empty((b, n), dtype=torch.int32, device=dev)
    unary = torch.empty((b, c, h, w), dtype=torch.float32, device=dev)
    q = [torch.empty((b, c, h, w), dtype=torch.float32, device=dev) for _ in range(2 if iters else 1)]          # ping-pong
    npos = torch.empty(n, dtype=torch.float32, device=dev) if iters else None
    nbi = torch.empty((b, n), dtype=torch.float32, device=dev) if iters else None
    table = torch.empty(h + w, dtype=torch.float32, device=dev) if iters else None
    _launch("vqseg_crf_prepare_f", dev, ip, *istr, pp, *pstr, b, c, h, w, iters, bi_xy_std, bi_rgb_std, pos_xy_std, trunc,
            _T(rgb, "colours", dtype=torch.int32, numel=b * n), _f32(unary, "unary", b * c * n), _f32(q[0], "q", b * c * n),
            _f32(npos, "positional norm", n), _f32(nbi, "bilateral norm", b * n), _f32(table, "positional table", h + w))
    return q, rgb, unary, npos, nbi


def _crf_step(state, at, bi_w, bi_xy_std, bi_rgb_std, pos_w, pos_xy_std, trunc, energies):
    """one vqseg_crf_step_f launch: q[at] -> q[1 - at] (E instead of Q with `energies`)"""
    q, rgb, unary, npos, nbi = state
    b, c, h, w = unary.shape
    n = h * w
    _launch("vqseg_crf_step_f", unary.device, _T(rgb, "colours", dtype=torch.int32, numel=b * n), _f32(unary, "unary", b * c * n),
            _f32(npos, "positional norm", n), _f32(nbi, "bilateral norm", b * n), _f32(q[at], "q in", b * c * n),
            _f32(q[1 - at], "q out", b * c * n), b, c, h, w, bi_w, bi_xy_std, bi_rgb_std, pos_w, pos_xy_std, trunc, int(bool(energies)))


# ------------------------------------------------------------------------------------------------
# SLIC superpixels and the mean over the segments of a label map (vqseg_slic_*_f, vqseg_segment_*_f; include/vqseg.h states the algorithm)
# ------------------------------------------------------------------------------------------------
SLIC_MAX_SIDE = 4096
SEGMENT_MAX_CHANNELS = 1024


def slic_grid(h: int, w: int, num_components: int):
    """(gy, gx) of `num_components` superpixels on an h x w image: S = sqrt(h w / K), gy = max(1, round(h / S)), gx likewise
    (Python's round; K_eff = gy * gx need not be K).  1 <= K <= h w, so a cell is at least one pixel."""
    h, w = int(h), int(w)
    if isinstance(num_components, bool) or int(num_components) != num_components or not 1 <= int(num_components) <= h * w:
        raise ValueError(f"num_components must be an integer in 1..h * w = {h * w}, got {num_components!r}")
    s = (h * w / int(num_components)) ** 0.5
    return max(1, int(round(h / s))), max(1, int(round(w / s)))


def slic_settings(h, w, num_components, compactness=10.0, iters=10, who="slic"):
    """the checked settings of a slic call as (gy, gx, spatial weight (compactness / S)^2, iters)"""
    gy, gx = slic_grid(h, w, num_components)
    if isinstance(iters, bool) or int(iters) != iters or int(iters) < 0:
        raise ValueError(f"{who}: iters must be an integer >= 0, got {iters!r}")
    m = float(compactness)
    if not 0.0 <= m <= 1e9:
        raise ValueError(f"{who}: compactness must lie in [0, 1e9], got {compactness!r}")
    return gy, gx, m * m * int(num_components) / (int(h) * int(w)), int(iters)


def slic_supported(images) -> bool:
    """what the kernels take: a float32 GPU tensor (B, 3, H, W), 1..65535 images, sides up to SLIC_MAX_SIDE"""
    return (torch.is_tensor(images) and images.is_cuda and images.dim() == 4 and images.dtype == torch.float32 and images.shape[1] == 3
            and 1 <= images.shape[0] <= 65535 and 1 <= images.shape[2] <= SLIC_MAX_SIDE and 1 <= images.shape[3] <= SLIC_MAX_SIDE)


def _slic_lab(images, gy, gx):
    """one vqseg_slic_lab_f launch -> (lab (B, 3, H, W) planar, the grid's initial centres (B, gy * gx, 5))"""
    images, istr = _crf_dense(images)
    b, _, h, w = images.shape
    dev, n, k = images.device, h * w, gy * gx
    ip = _strided_f32(images, "images", b * 3 * n)
    if dev.type != "cuda":                       # before any buffer is asked for on a device that has no HIP path
        _launch("vqseg_slic_lab_f", dev, ip, *istr, b, h, w, gy, gx, None, None)
    lab = torch.empty((b, 3, h, w), dtype=torch.float32, device=dev)
    centers = torch.empty((b, k, 5), dtype=torch.float32, device=dev)
    _launch("vqseg_slic_lab_f", dev, ip, *istr, b, h, w, gy, gx, _f32(lab, "lab", b * 3 * n), _f32(centers, "centers", b * k * 5))
    return lab, centers


def _slic_assign(lab, centers, gy, gx, weight, labels=None):
    """one vqseg_slic_assign_f launch -> labels (B, H, W) int32 (`labels`: written in place)"""
    b, _, h, w = lab.shape
    if labels is None:
        labels = torch.empty((b, h, w), dtype=torch.int32, device=lab.device)
    _launch("vqseg_slic_assign_f", lab.device, _f32(lab, "lab", b * 3 * h * w), _f32(centers, "centers", b * gy * gx * 5), b, h, w, gy, gx,
            float(weight), _T(labels, "labels", dtype=torch.int32, numel=b * h * w))
    return labels


def _slic_update(lab, labels, centers, gy, gx):
    """one vqseg_slic_update_f launch: `centers` (B, gy * gx, 5) become the means of their pixels, in place"""
    b, _, h, w = lab.shape
    _launch("vqseg_slic_update_f", lab.device, _f32(lab, "lab", b * 3 * h * w), _T(labels, "labels", dtype=torch.int32, numel=b * h * w),
            b, h, w, gy, gx, _f32(centers, "centers", b * gy * gx * 5))
    return centers


def _slic_loop(lab, centers, gy, gx, weight, iters):
    """`iters` times {assign; update} on `centers` (in place), then the final assign -> labels (slic and saliency_rbd share it)"""
    labels = None
    for _ in range(iters):
        labels = _slic_assign(lab, centers, gy, gx, weight, labels)
        _slic_update(lab, labels, centers, gy, gx)
    return _slic_assign(lab, centers, gy, gx, weight, labels)


def slic(images, num_components, compactness=10.0, iters=10):
    """SLIC superpixels of `images` (B, 3, H, W) float32 in [0, 1] on the GPU, NCHW-contiguous or channels_last -> (labels int32
    (B, H, W), centers float32 (B, K_eff, 5) = (L, a, b, y, x), (gy, gx)): the algorithm of include/vqseg.h -- CIELAB, a gy x gx
    grid of slic_grid, `iters` times {assign among the 3 x 3 cells around the home cell; update}, one final assign, so the labels
    are the assignment against the returned centres.  No connectivity enforcement.  One Lab launch, 2 iters + 1 others; bit-identical
    from call to call.  No gradient flows.  There is no CPU form here (utils.superpixel.slic has one)."""
    E = _hip.HipLibraryError
    if not (torch.is_tensor(images) and images.dim() == 4 and images.shape[1] == 3):
        raise E(f"slic: images must be a (B, 3, H, W) tensor, got {tuple(getattr(images, 'shape', ()))}")
    b, _, h, w = images.shape
    gy, gx, weight, iters = slic_settings(h, w, num_components, compactness, iters)
    if min(b, h, w) < 1 or b > 65535 or max(h, w) > SLIC_MAX_SIDE:
        raise E(f"slic: 1..65535 images with sides of 1..{SLIC_MAX_SIDE}, got {tuple(images.shape)}")
    lab, centers = _slic_lab(images, gy, gx)
    return _slic_loop(lab, centers, gy, gx, weight, iters), centers, (gy, gx)


def segment_mean_supported(x, labels) -> bool:
    """what the kernels take: x float32 (B, C, H, W) on the GPU with up to SEGMENT_MAX_CHANNELS channels, labels an integer tensor
    (B, H, W) on the same device"""
    return (torch.is_tensor(x) and torch.is_tensor(labels) and x.is_cuda and labels.device == x.device and x.dim() == 4 and labels.dim() == 3
            and x.dtype == torch.float32 and labels.dtype in (torch.int32, torch.int64) and x.numel() > 0
            and 1 <= x.shape[1] <= SEGMENT_MAX_CHANNELS and labels.shape[0] == x.shape[0] and labels.shape[1:] == x.shape[2:])


def _segment_mean(x, labels, k):
    """the two launches: sums and counts of x over the segments, then their quotient at every pixel, with x's strides"""
    x, xs = _crf_dense(x)
    b, c, h, w = x.shape
    n, dev = h * w, x.device
    xp, lp = _strided_f32(x, "x", b * c * n), _T(labels, "labels", dtype=torch.int32, numel=b * n)
    if dev.type != "cuda":
        _launch("vqseg_segment_sums_f", dev, xp, *xs, lp, b, c, n, k, None, None)
    sums = torch.empty((b, k, c), dtype=torch.float32, device=dev)
    counts = torch.empty((b, k), dtype=torch.int32, device=dev)
    y = torch.empty_strided(x.shape, x.stride(), dtype=torch.float32, device=dev)
    sp, cp = _f32(sums, "segment sums", b * k * c), _T(counts, "segment counts", dtype=torch.int32, numel=b * k)
    _launch("vqseg_segment_sums_f", dev, xp, *xs, lp, b, c, n, k, sp, cp)
    _launch("vqseg_segment_broadcast_f", dev, xp, *xs, lp, sp, cp, b, c, n, k, _strided_f32(y, "y", b * c * n), *xs)
    return y


class _SegmentMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, labels, k):
        ctx.save_for_backward(labels)
        ctx.k = k
        return _segment_mean(x, labels, k)

    @staticmethod
    def backward(ctx, g):
        (labels,) = ctx.saved_tensors
        return _segment_mean(g.float(), labels, ctx.k), None, None       # a symmetric projection: its own adjoint


def segment_mean(x, labels, num_segments):
    """y[b, :, p] = the mean of x[b, :, q] over the pixels q of image b with labels[b, q] == labels[b, p], for ANY label map; a pixel
    whose label lies outside [0, num_segments) passes through unchanged.  x float32 (B, C, H, W) on the GPU, NCHW-contiguous or
    channels_last (y has x's strides), labels (B, H, W) int32 (int64 is converted).  Two launches (vqseg_segment_sums_f,
    vqseg_segment_broadcast_f); the backward pass is the same two on the incoming gradient.  Within a segment y is exactly constant."""
    E = _hip.HipLibraryError
    if not (torch.is_tensor(x) and torch.is_tensor(labels) and x.dim() == 4 and labels.dim() == 3):
        raise E("segment_mean: x must be a (B, C, H, W) tensor and labels a (B, H, W) tensor")
    if labels.shape[0] != x.shape[0] or labels.shape[1:] != x.shape[2:]:
        raise E(f"segment_mean: labels must be (B, H, W) of x's batch and size, got {tuple(labels.shape)} and {tuple(x.shape)}")
    if labels.dtype not in (torch.int32, torch.int64):
        raise E(f"segment_mean: labels must be int32 (or int64), got {labels.dtype}")
    if isinstance(num_segments, bool) or int(num_segments) != num_segments or int(num_segments) < 1:
        raise ValueError(f"segment_mean: num_segments must be a positive integer, got {num_segments!r}")
    if x.numel() == 0 or x.shape[1] > SEGMENT_MAX_CHANNELS:
        raise E(f"segment_mean: a non-empty x with at most {SEGMENT_MAX_CHANNELS} channels, got {tuple(x.shape)}")
    if labels.device != x.device:
        raise E(f"segment_mean: x and labels must be on one device, got {x.device} and {labels.device}")
    labels = labels.detach().to(torch.int32).contiguous()
    return _SegmentMean.apply(x, labels, int(num_segments))


# ------------------------------------------------------------------------------------------------
# RBD saliency over SLIC superpixels (vqseg_region_graph_f, vqseg_rbd_*_f; include/vqseg.h states the definition)
# ------------------------------------------------------------------------------------------------
RBD_MAX_SEGMENTS = 1024


def rbd_settings(sigma_clr=10.0, sigma_bndcon=1.0, sigma_spa=0.25, mu=0.1, who="saliency_rbd"):
    """the checked parameters of an RBD call as floats"""
    out = []
    for name, v in (("sigma_clr", sigma_clr), ("sigma_bndcon", sigma_bndcon), ("sigma_spa", sigma_spa)):
        v = float(v)
        if not 0.0 < v <= 1e18:
            raise ValueError(f"{who}: {name} must lie in (0, 1e18], got {v!r}")
        out.append(v)
    mu = float(mu)
    if not 0.0 <= mu <= 1e18:
        raise ValueError(f"{who}: mu must lie in [0, 1e18], got {mu!r}")
    return (*out, mu)


def rbd_supported(images, n_segments=250) -> bool:
    """what the kernels take: what slic takes, with a grid of at most RBD_MAX_SEGMENTS cells"""
    if not slic_supported(images):
        return False
    try:
        gy, gx = slic_grid(images.shape[2], images.shape[3], n_segments)
    except (ValueError, TypeError):
        return False
    return gy * gx <= RBD_MAX_SEGMENTS


def _rbd_check(who, b, h, w, gy, gx):
    E = _hip.HipLibraryError
    if min(b, h, w) < 1 or b > 65535 or max(h, w) > SLIC_MAX_SIDE:
        raise E(f"{who}: 1..65535 images with sides of 1..{SLIC_MAX_SIDE}, got {b} of {h} x {w}")
    if not (1 <= gy <= h and 1 <= gx <= w):
        raise E(f"{who}: the grid must have 1..h rows and 1..w columns of cells, got {gy} x {gx} on {h} x {w}")
    if gy * gx > RBD_MAX_SEGMENTS:
        raise E(f"{who}: at most {RBD_MAX_SEGMENTS} superpixels, got a {gy} x {gx} grid ({gy * gx})")


def _rbd_region_graph(lab, labels, gy, gx):
    """one vqseg_region_graph_f launch -> (stats (B, K, 8) = (L, a, b, y, x, n, bnd, 0), adj uint8 (B, K, K))"""
    b, _, h, w = lab.shape
    k, dev = gy * gx, lab.device
    _rbd_check("region_graph", b, h, w, gy, gx)
    lp, bp = _f32(lab, "lab", b * 3 * h * w), _T(labels, "labels", dtype=torch.int32, numel=b * h * w)
    if dev.type != "cuda":
        _launch("vqseg_region_graph_f", dev, lp, bp, b, h, w, gy, gx, None, None)
    stats = torch.empty((b, k, 8), dtype=torch.float32, device=dev)
    adj = torch.empty((b, k, k), dtype=torch.uint8, device=dev)
    _launch("vqseg_region_graph_f", dev, lp, bp, b, h, w, gy, gx, _f32(stats, "stats", b * k * 8), _T(adj, "adj", dtype=torch.uint8, numel=b * k * k))
    return stats, adj


def _rbd_tables(who, stats, *tables):
    """(b, k) of stats (B, K, 8), after checking that every table is (B, K, K) or (B, K) of it"""
    E = _hip.HipLibraryError
    if not (torch.is_tensor(stats) and stats.dim() == 3 and stats.shape[2] == 8 and 1 <= stats.shape[1] <= RBD_MAX_SEGMENTS
            and 1 <= stats.shape[0] <= 65535):
        raise E(f"{who}: stats must be (B, K, 8) with 1..65535 images and K <= {RBD_MAX_SEGMENTS}, got {tuple(getattr(stats, 'shape', ()))}")
    b, k = stats.shape[:2]
    for t in tables:
        if not (torch.is_tensor(t) and tuple(t.shape) in ((b, k, k), (b, k))):
            raise E(f"{who}: a table of shape {tuple(getattr(t, 'shape', ()))} beside stats {tuple(stats.shape)}")
    return b, k


def _rbd_weights(stats, adj):
    """one vqseg_rbd_weights_f launch -> W (B, K, K): the colour distance along an edge, 0 on the diagonal, +inf elsewhere"""
    b, k = _rbd_tables("rbd_weights", stats, adj)
    sp, ap = _f32(stats, "stats", b * k * 8), _T(adj, "adj", dtype=torch.uint8, numel=b * k * k)
    if stats.device.type != "cuda":
        _launch("vqseg_rbd_weights_f", stats.device, sp, ap, b, k, None)
    wgt = torch.empty((b, k, k), dtype=torch.float32, device=stats.device)
    _launch("vqseg_rbd_weights_f", stats.device, sp, ap, b, k, _f32(wgt, "weights", b * k * k))
    return wgt


def _rbd_geodesic(wgt, inplace=False):
    """vqseg_rbd_geodesic_f: all-pairs shortest path lengths over W (B, K, K) (a copy unless `inplace`)"""
    E = _hip.HipLibraryError
    if not (torch.is_tensor(wgt) and wgt.dim() == 3 and wgt.shape[1] == wgt.shape[2] and 1 <= wgt.shape[1] <= RBD_MAX_SEGMENTS
            and 1 <= wgt.shape[0] <= 65535):
        raise E(f"rbd_geodesic: W must be (B, K, K) with 1..65535 images and K <= {RBD_MAX_SEGMENTS}, got {tuple(getattr(wgt, 'shape', ()))}")
    b, k = wgt.shape[:2]
    wp = _f32(wgt, "weights", b * k * k)
    if wgt.device.type != "cuda":
        _launch("vqseg_rbd_geodesic_f", wgt.device, wp, b, k)
    g = wgt if inplace else wgt.clone()
    _launch("vqseg_rbd_geodesic_f", g.device, _f32(g, "geodesic", b * k * k), b, k)
    return g


def _rbd_background(g, stats, sigma_clr=10.0, sigma_bndcon=1.0):
    """one vqseg_rbd_background_f launch -> w_bg (B, K)"""
    b, k = _rbd_tables("rbd_background", stats, g)
    gp, sp = _f32(g, "geodesic", b * k * k), _f32(stats, "stats", b * k * 8)
    if g.device.type != "cuda":
        _launch("vqseg_rbd_background_f", g.device, gp, sp, b, k, float(sigma_clr), float(sigma_bndcon), None)
    w_bg = torch.empty((b, k), dtype=torch.float32, device=g.device)
    _launch("vqseg_rbd_background_f", g.device, gp, sp, b, k, float(sigma_clr), float(sigma_bndcon), _f32(w_bg, "w_bg", b * k))
    return w_bg


def _rbd_contrast(g, stats, w_bg, h, w, sigma_spa=0.25):
    """one vqseg_rbd_contrast_f launch -> wCtr (B, K), not yet normalised"""
    b, k = _rbd_tables("rbd_contrast", stats, g, w_bg)
    gp, sp, wp = _f32(g, "geodesic", b * k * k), _f32(stats, "stats", b * k * 8), _f32(w_bg, "w_bg", b * k)
    if g.device.type != "cuda":
        _launch("vqseg_rbd_contrast_f", g.device, gp, sp, wp, b, k, int(h), int(w), float(sigma_spa), None)
    wctr = torch.empty((b, k), dtype=torch.float32, device=g.device)
    _launch("vqseg_rbd_contrast_f", g.device, gp, sp, wp, b, k, int(h), int(w), float(sigma_spa), _f32(wctr, "wctr", b * k))
    return wctr


def _rbd_solve(g, stats, adj, w_bg, wctr, sigma_clr=10.0, mu=0.1):
    """one vqseg_rbd_solve_f launch -> (wCtr normalised, x, x normalised), each (B, K)"""
    b, k = _rbd_tables("rbd_solve", stats, g, adj, w_bg, wctr)
    dev = g.device
    ins = (_f32(g, "geodesic", b * k * k), _f32(stats, "stats", b * k * 8), _T(adj, "adj", dtype=torch.uint8, numel=b * k * k),
           _f32(w_bg, "w_bg", b * k), _f32(wctr, "wctr", b * k))
    if dev.type != "cuda":
        _launch("vqseg_rbd_solve_f", dev, *ins, b, k, float(sigma_clr), float(mu), None, None, None, None)
    work = torch.empty((b, k, k), dtype=torch.float32, device=dev)
    outs = torch.empty((3, b, k), dtype=torch.float32, device=dev)
    _launch("vqseg_rbd_solve_f", dev, *ins, b, k, float(sigma_clr), float(mu), _f32(work, "workspace", b * k * k),
            *(_f32(o, "solve output", b * k) for o in outs))
    return outs[0], outs[1], outs[2]


def _rbd_paint(xnorm, labels, gy, gx):
    """one vqseg_rbd_paint_f launch -> sal (B, H, W) = xnorm[b, label]"""
    b, h, w = labels.shape
    _rbd_check("rbd_paint", b, h, w, gy, gx)
    k = gy * gx
    xp, lp = _f32(xnorm, "xnorm", b * k), _T(labels, "labels", dtype=torch.int32, numel=b * h * w)
    if labels.device.type != "cuda":
        _launch("vqseg_rbd_paint_f", labels.device, xp, lp, b, h, w, gy, gx, None)
    sal = torch.empty((b, h, w), dtype=torch.float32, device=labels.device)
    _launch("vqseg_rbd_paint_f", labels.device, xp, lp, b, h, w, gy, gx, _f32(sal, "saliency", b * h * w))
    return sal


def rbd_from_labels(lab, labels, grid, sigma_clr=10.0, sigma_bndcon=1.0, sigma_spa=0.25, mu=0.1, return_parts=False):
    """RBD saliency (include/vqseg.h) of planar Lab images (B, 3, H, W) float32 under a SLIC label map (B, H, W) int32 of the grid
    (gy, gx), both on the GPU -> (B, H, W) float32 in [0, 1], exactly constant within a superpixel.  6 + 3 ceil(K / 64) launches,
    bit-identical from call to call and independent of the batch.  `return_parts`: (map, dict of every stage's output)."""
    E = _hip.HipLibraryError
    if not (torch.is_tensor(lab) and torch.is_tensor(labels) and lab.dim() == 4 and lab.shape[1] == 3 and labels.dim() == 3
            and labels.shape[0] == lab.shape[0] and labels.shape[1:] == lab.shape[2:]):
        raise E(f"saliency_rbd: lab must be (B, 3, H, W) and labels (B, H, W) of one batch and size, got "
                f"{tuple(getattr(lab, 'shape', ()))} and {tuple(getattr(labels, 'shape', ()))}")
    if lab.dtype != torch.float32 or labels.dtype != torch.int32:
        raise E(f"saliency_rbd: lab must be float32 and labels int32, got {lab.dtype} and {labels.dtype}")
    if labels.device != lab.device:
        raise E(f"saliency_rbd: lab and labels must be on one device, got {lab.device} and {labels.device}")
    gy, gx = int(grid[0]), int(grid[1])
    sigma_clr, sigma_bndcon, sigma_spa, mu = rbd_settings(sigma_clr, sigma_bndcon, sigma_spa, mu)
    b, _, h, w = lab.shape
    _rbd_check("saliency_rbd", b, h, w, gy, gx)
    lab, labels = lab.detach().contiguous(), labels.detach().contiguous()
    stats, adj = _rbd_region_graph(lab, labels, gy, gx)
    g = _rbd_geodesic(_rbd_weights(stats, adj), inplace=True)
    w_bg = _rbd_background(g, stats, sigma_clr, sigma_bndcon)
    wctr = _rbd_contrast(g, stats, w_bg, h, w, sigma_spa)
    wctr_norm, x, xnorm = _rbd_solve(g, stats, adj, w_bg, wctr, sigma_clr, mu)
    sal = _rbd_paint(xnorm, labels, gy, gx)
    if return_parts:
        return sal, dict(stats=stats, adj=adj, geodesic=g, w_bg=w_bg, wctr=wctr, wctr_norm=wctr_norm, x=x, xnorm=xnorm)
    return sal


def saliency_rbd(images, n_segments=250, compactness=10.0, iters=10, sigma_clr=10.0, sigma_bndcon=1.0, sigma_spa=0.25, mu=0.1,
                 return_parts=False):
    """RBD saliency maps of `images` (B, 3, H, W) float32 in [0, 1] on the GPU, NCHW-contiguous or channels_last -> (B, H, W) float32
    in [0, 1]: slic's superpixels (ONE Lab launch serves the assign / update loop and the region pass), then rbd_from_labels.  The
    labels are nnf.slic's, bit for bit.  No gradient flows.  `return_parts`: (map, dict with labels, centers, grid and every stage).
    There is no CPU form here (utils.saliency.saliency_rbd has one)."""
    E = _hip.HipLibraryError
    if not (torch.is_tensor(images) and images.dim() == 4 and images.shape[1] == 3):
        raise E(f"saliency_rbd: images must be a (B, 3, H, W) tensor, got {tuple(getattr(images, 'shape', ()))}")
    b, _, h, w = images.shape
    gy, gx, weight, iters = slic_settings(h, w, n_segments, compactness, iters, who="saliency_rbd")
    rbd_settings(sigma_clr, sigma_bndcon, sigma_spa, mu)
    _rbd_check("saliency_rbd", b, h, w, gy, gx)
    if images.dtype != torch.float32:
        raise E(f"saliency_rbd: images must be float32, got {images.dtype}")
    lab, centers = _slic_lab(images, gy, gx)
    labels = _slic_loop(lab, centers, gy, gx, weight, iters)
    out = rbd_from_labels(lab, labels, (gy, gx), sigma_clr, sigma_bndcon, sigma_spa, mu, return_parts)
    if return_parts:
        out[1].update(labels=labels, centers=centers, grid=(gy, gx), lab=lab)
    return out


# ------------------------------------------------------------------------------------------------
# Connected regions of an integer map (vqseg_region_*; include/vqseg.h states the definition, tests/region_cases.py restates it)
# ------------------------------------------------------------------------------------------------
REGION_MAX_SIDE = 4096
REGION_VALUE_DTYPES = (torch.uint8, torch.int32)              # what the kernels read; int64 is converted here and the result converted back
REGION_CALLS = 0              # calls of filter_regions that reached the library (as _hip.BOX_MIX_CALLS: for tests, never read by the product)


def region_settings(connectivity=4, ignore=(), who="regions"):
    """the checked (connectivity, ignore tuple) of a region call: 4 or 8; 0 to 4 integers that fit int32"""
    if isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError(f"{who}: connectivity must be 4 or 8, got {connectivity!r}")
    if isinstance(ignore, (int, np.integer)) and not isinstance(ignore, bool):
        ignore = (ignore,)
    try:
        ignore = tuple(ignore)
    except TypeError:
        raise ValueError(f"{who}: ignore must be a sequence of 0 to 4 integers, got {ignore!r}") from None
    if len(ignore) > 4 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -2 ** 31 <= int(v) < 2 ** 31 for v in ignore):
        raise ValueError(f"{who}: ignore must be a sequence of 0 to 4 integers that fit int32, got {ignore!r}")
    return int(connectivity), tuple(int(v) for v in ignore)


def _region_shape(t, name, who, dtypes):
    E = _hip.HipLibraryError
    if not (torch.is_tensor(t) and t.dim() == 3):
        raise E(f"{who}: {name} must be a (B, H, W) tensor, got {tuple(getattr(t, 'shape', ()))}")
    if t.dtype not in dtypes:
        raise E(f"{who}: {name} must be {' or '.join(str(d).removeprefix('torch.') for d in dtypes)}, got {t.dtype}")
    b, h, w = t.shape
    if not (1 <= b <= 65535 and 1 <= h <= REGION_MAX_SIDE and 1 <= w <= REGION_MAX_SIDE):
        raise E(f"{who}: 1..65535 images with sides of 1..{REGION_MAX_SIDE}, got {tuple(t.shape)}")
    return b, h, w


def _region_same(who, first, **others):
    E = _hip.HipLibraryError
    for name, t in others.items():
        if tuple(t.shape) != tuple(first.shape):
            raise E(f"{who}: {name} must have the values' shape {tuple(first.shape)}, got {tuple(t.shape)}")
        if t.device != first.device:
            raise E(f"{who}: all tensors must be on one device, got {first.device} and {t.device} ({name})")


def regions_supported(values) -> bool:
    """what the kernels take: an integer GPU tensor (B, H, W) of uint8, int32 or int64, 1..65535 images, sides up to REGION_MAX_SIDE"""
    return (torch.is_tensor(values) and values.is_cuda and values.dim() == 3 and values.dtype in REGION_VALUE_DTYPES + (torch.int64,)
            and 1 <= values.shape[0] <= 65535 and 1 <= values.shape[1] <= REGION_MAX_SIDE and 1 <= values.shape[2] <= REGION_MAX_SIDE)


def _region_values(values, who):
    """(the map as the kernels read it, its entry-point suffix).  An int64 map is narrowed to int32 without a look at its values (that
    would be a host round trip): class ids, superpixel labels and 255 fit; a value outside int32 wraps, in the result too."""
    _region_shape(values, "values", who, REGION_VALUE_DTYPES + (torch.int64,))
    v = values.detach()
    v = (v.to(torch.int32) if v.dtype == torch.int64 else v).contiguous()
    return v, "u8" if v.dtype == torch.uint8 else "i32"


def _i32(t, name, numel):
    return _T(t, name, dtype=torch.int32, numel=numel)


def _region_roots(v, kind, conn, ign):
    b, h, w = v.shape
    dev, n = v.device, b * h * w
    name = f"vqseg_region_roots_{kind}"
    vp = _T(v, "values", dtype=v.dtype, numel=n)
    ig = list(ign) + [0] * (4 - len(ign))
    if dev.type != "cuda":
        _launch(name, dev, vp, b, h, w, conn, len(ign), *ig, None, None)
    parent = torch.empty((b, h, w), dtype=torch.int32, device=dev)
    roots = torch.empty((b, h, w), dtype=torch.int32, device=dev)
    _launch(name, dev, vp, b, h, w, conn, len(ign), *ig, _i32(parent, "parent", n), _i32(roots, "roots", n))
    return roots


def region_roots(values, connectivity=4, ignore=()):
    """roots int32 (B, H, W) of the connected regions of `values` (B, H, W) uint8 / int32 (int64 is converted) on the GPU: the smallest
    row-major index y * W + x of the pixel's region -- equal value, 4- or 8-connected, per image -- and -1 where the value is one of
    `ignore` (0 to 4 integers).  Three launches (vqseg_region_roots_u8 / _i32); exact, bit-identical from call to call.  There is no
    CPU form here (utils.regions has one)."""
    conn, ign = region_settings(connectivity, ignore, "region_roots")
    v, kind = _region_values(values, "region_roots")
    return _region_roots(v, kind, conn, ign)


def _region_ids(roots):
    b, h, w = roots.shape
    dev, n = roots.device, b * h * w
    rp = _i32(roots, "roots", n)
    if dev.type != "cuda":
        _launch("vqseg_region_ids_i32", dev, rp, b, h, w, None, None, None)
    nblk = int(lib().vqseg_region_ids_partials(h, w))
    partial = torch.empty((b, nblk), dtype=torch.int32, device=dev)
    ids = torch.empty((b, h, w), dtype=torch.int32, device=dev)
    counts = torch.empty((b,), dtype=torch.int32, device=dev)
    _launch("vqseg_region_ids_i32", dev, rp, b, h, w, _i32(partial, "partial", b * nblk), _i32(ids, "ids", n), _i32(counts, "counts", b))
    return ids, counts


def region_ids(roots):
    """(ids int32 (B, H, W), counts int32 (B,)) of a root map as region_roots makes it: a region's id is its 0-based rank among the
    image's regions by rising root (scipy.ndimage.label's order, minus one), -1 where root is -1; counts the regions per image.  An
    entry of `roots` outside [0, H W), or one that does not point at a root, is a pixel of no region.  Four launches."""
    _region_shape(roots, "roots", "region_ids", (torch.int32,))
    return _region_ids(roots.detach().contiguous())


def _region_areas(roots):
    b, h, w = roots.shape
    dev, n = roots.device, b * h * w
    rp = _i32(roots, "roots", n)
    if dev.type != "cuda":
        _launch("vqseg_region_areas_i32", dev, rp, b, h, w, None)
    areas = torch.empty((b, h, w), dtype=torch.int32, device=dev)
    _launch("vqseg_region_areas_i32", dev, rp, b, h, w, _i32(areas, "areas", n))
    return areas


def region_areas(roots):
    """areas int32 (B, H, W): every region's area at its root index, 0 elsewhere (one memset and one launch: the runs of equal
    roots of a workgroup's 256 pixels are gathered in LDS, then one atomic per root)"""
    _region_shape(roots, "roots", "region_areas", (torch.int32,))
    return _region_areas(roots.detach().contiguous())


def region_table(values, roots, ids, counts, capacity):
    """(table int32 (B, capacity, 8) = (value, area, ymin, xmin, ymax, xmax, root, 0), moments int64 (B, capacity, 2) = (sum y, sum x)):
    row `id` of every region of region_roots / region_ids' maps; rows from min(count, capacity) on are zero, and a region whose id is
    >= capacity writes no row.  ids outside [0, capacity) and roots outside [0, H W) are never used as indices.  `counts` (B,) int32
    is what region_ids returned (its shape is checked; the kernels do not read it)."""
    E = _hip.HipLibraryError
    v, _kind = _region_values(values, "region_table")
    b, h, w = _region_shape(roots, "roots", "region_table", (torch.int32,))
    _region_shape(ids, "ids", "region_table", (torch.int32,))
    _region_same("region_table", v, roots=roots, ids=ids)
    if not (torch.is_tensor(counts) and counts.dtype == torch.int32 and tuple(counts.shape) == (b,)):
        raise E(f"region_table: counts must be an int32 tensor ({b},), got {getattr(counts, 'dtype', None)} {tuple(getattr(counts, 'shape', ()))}")
    if isinstance(capacity, bool) or int(capacity) != capacity or not 1 <= int(capacity) or b * int(capacity) > 1 << 26:
        raise ValueError(f"region_table: capacity must be a positive integer with B * capacity <= 2^26, got {capacity!r}")
    capacity = int(capacity)
    roots, ids = roots.detach().contiguous(), ids.detach().contiguous()
    dev, n = v.device, b * h * w
    vp, rp, ip = _T(v, "values", dtype=v.dtype, numel=n), _i32(roots, "roots", n), _i32(ids, "ids", n)
    if dev.type != "cuda":
        _launch("vqseg_region_table_i32", dev, vp, v.element_size(), rp, ip, b, h, w, capacity, None, None)
    table = torch.empty((b, capacity, 8), dtype=torch.int32, device=dev)
    moments = torch.empty((b, capacity, 2), dtype=torch.int64, device=dev)
    _launch("vqseg_region_table_i32", dev, vp, v.element_size(), rp, ip, b, h, w, capacity, _i32(table, "table", b * capacity * 8),
            _T(moments, "moments", dtype=torch.int64, numel=b * capacity * 2))
    return table, moments


def region_fill(fill, dtype, who="filter_regions"):
    """the checked fill of a filter call as (neighbour flag, constant): "neighbour", or an integer the element type holds"""
    if isinstance(fill, str):
        if fill != "neighbour":
            raise ValueError(f"{who}: fill must be 'neighbour' or an integer, got {fill!r}")
        return 1, 0
    info = torch.iinfo(torch.int32 if dtype == torch.int64 else dtype)
    if isinstance(fill, bool) or not isinstance(fill, (int, np.integer)) or not info.min <= int(fill) <= info.max:
        raise ValueError(f"{who}: fill must be 'neighbour' or an integer in {info.min}..{info.max} for {dtype}, got {fill!r}")
    return 0, int(fill)


def region_min_area(min_area, who="filter_regions"):
    if isinstance(min_area, bool) or not isinstance(min_area, (int, np.integer)) or not 0 <= int(min_area) < 2 ** 31:
        raise ValueError(f"{who}: min_area must be an integer >= 0, got {min_area!r}")
    return int(min_area)


def filter_regions_from(values, roots, areas, min_area, fill=0):
    """the filter launch alone, from maps already made (region_roots, region_areas): see filter_regions"""
    global REGION_CALLS
    min_area = region_min_area(min_area)
    v, kind = _region_values(values, "filter_regions")
    neighbour, const = region_fill(fill, values.dtype)
    b, h, w = v.shape
    _region_shape(roots, "roots", "filter_regions", (torch.int32,))
    _region_shape(areas, "areas", "filter_regions", (torch.int32,))
    _region_same("filter_regions", v, roots=roots, areas=areas)
    roots, areas = roots.detach().contiguous(), areas.detach().contiguous()
    dev, n = v.device, b * h * w
    name = f"vqseg_region_filter_{kind}"
    vp, rp, ap = _T(v, "values", dtype=v.dtype, numel=n), _i32(roots, "roots", n), _i32(areas, "areas", n)
    if dev.type != "cuda":
        _launch(name, dev, vp, rp, ap, b, h, w, min_area, neighbour, const, None)
    out = torch.empty_like(v)
    _launch(name, dev, vp, rp, ap, b, h, w, min_area, neighbour, const, _T(out, "out", dtype=v.dtype, numel=n))
    REGION_CALLS += 1
    return out.to(values.dtype)


def filter_regions(values, min_area, connectivity=4, ignore=(), fill=0):
    """`values` (B, H, W) uint8 / int32 / int64 on the GPU with every region (region_roots' definition) of fewer than `min_area` pixels
    replaced: by the constant `fill`, or with fill="neighbour" by the input value of the pixel before the region's root -- (y, x - 1),
    else (y - 1, x), else the region stays.  Ignored pixels keep their value.  Read from the input: single shot, no cascade.  Roots
    (three launches), areas (a memset and one) and the gather; exact and bit-identical from call to call."""
    conn, ign = region_settings(connectivity, ignore, "filter_regions")
    region_min_area(min_area)
    v, kind = _region_values(values, "filter_regions")
    region_fill(fill, values.dtype)
    roots = _region_roots(v, kind, conn, ign)
    out = filter_regions_from(v, roots, _region_areas(roots), min_area, fill)
    return out.to(values.dtype)


# ------------------------------------------------------------------------------------------------
# Panoptic quality: region overlap, matching, counts (vqseg_instance_*; include/vqseg.h states the definition, tests/instance_cases.py
# restates it)
# ------------------------------------------------------------------------------------------------
INSTANCE_MAX_CAPACITY = 65535
INSTANCE_MAX_CLASSES = 255
INSTANCE_CALLS = 0            # calls of instance_overlap that reached the library (as REGION_CALLS: for tests, never read by the product)

InstanceTally = namedtuple("InstanceTally", "match inter union matched tally iou_sum overflow")


def instance_settings(num_classes, things=None, void=(255,), connectivity=4, capacity=1024, who="instances"):
    """the checked (num_classes, things, void, connectivity, capacity) of an instance call: 1..255 classes; things a sorted tuple of
    distinct classes (default 1..C-1); void 0 to 4 integers that fit int32, none of them a thing; 4 or 8; capacity in 1..65535"""
    if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or not 1 <= int(num_classes) <= INSTANCE_MAX_CLASSES:
        raise ValueError(f"{who}: num_classes must be an integer in 1..{INSTANCE_MAX_CLASSES}, got {num_classes!r}")
    c = int(num_classes)
    if things is None:
        things = range(1, c)
    if isinstance(things, (int, np.integer)) and not isinstance(things, bool):
        things = (things,)
    try:
        things = tuple(things)
    except TypeError:
        raise ValueError(f"{who}: things must be a sequence of classes in 0..{c - 1}, got {things!r}") from None
    if any(isinstance(t, bool) or not isinstance(t, (int, np.integer)) or not 0 <= int(t) < c for t in things) or len(set(things)) != len(things):
        raise ValueError(f"{who}: things must be distinct classes in 0..{c - 1}, got {things!r}")
    things = tuple(sorted(int(t) for t in things))
    connectivity, void = region_settings(connectivity, void, who)
    if set(void) & set(things):
        raise ValueError(f"{who}: a void value cannot be a thing class, got void {void!r} and things {things!r}")
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or not 1 <= int(capacity) <= INSTANCE_MAX_CAPACITY:
        raise ValueError(f"{who}: capacity must be an integer in 1..{INSTANCE_MAX_CAPACITY}, got {capacity!r}")
    return c, things, void, connectivity, int(capacity)


def instance_supported(pred, target) -> bool:
    """what the instance kernels take: two maps regions_supported takes, of one shape, on one device"""
    return regions_supported(pred) and regions_supported(target) and tuple(pred.shape) == tuple(target.shape) and pred.device == target.device


def _instance_rows(t, name, who, b, capacity, cols=None, dtype=torch.int32):
    shape = (b, capacity) if cols is None else (b, capacity, cols)
    if not (torch.is_tensor(t) and t.dtype == dtype and tuple(t.shape) == shape):
        raise _hip.HipLibraryError(f"{who}: {name} must be a {str(dtype).removeprefix('torch.')} tensor {shape}, got "
                                   f"{getattr(t, 'dtype', None)} {tuple(getattr(t, 'shape', ()))}")
    return t.detach().contiguous()


def _instance_counts(t, name, who, b):
    if not (torch.is_tensor(t) and t.dtype == torch.int32 and tuple(t.shape) == (b,)):
        raise _hip.HipLibraryError(f"{who}: {name} must be an int32 tensor ({b},), got {getattr(t, 'dtype', None)} {tuple(getattr(t, 'shape', ()))}")
    return t.detach().contiguous()


def _instance_capacity(capacity, table, who):
    if capacity is None:
        capacity = table.shape[1] if torch.is_tensor(table) and table.dim() == 3 else None
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or not 1 <= int(capacity) <= INSTANCE_MAX_CAPACITY:
        raise ValueError(f"{who}: capacity must be an integer in 1..{INSTANCE_MAX_CAPACITY}, got {capacity!r}")
    return int(capacity)


def instance_overlap(pred_ids, gt_ids, target, pred_table, gt_table, void=(255,), capacity=None):
    """(cand, inter, void_count), int32 (B, capacity) each, of two id maps int32 (B, H, W) as region_ids makes them, the target class map
    (uint8 / int32; int64 is converted) and both region tables (B, capacity, 8): cand[b][g] the prediction id that holds more than
    half of ground-truth region g (or -1; garbage that is a valid id where no region does -- instance_tally's test sorts that out),
    inter[b][g] the pixels g shares with it, void_count[b][p] the pixels of prediction region p that have no ground-truth id and a
    target value in `void`.  vqseg_instance_vote_i32 (two memsets, one pass) and vqseg_instance_overlap_i32 (a memset, a small launch,
    one pass).  Ids outside [0, capacity) are pixels of no region.  Exact, bit-identical from call to call."""
    global INSTANCE_CALLS
    who = "instance_overlap"
    _conn, vd = region_settings(4, void, who)
    b, h, w = _region_shape(pred_ids, "pred_ids", who, (torch.int32,))
    _region_shape(gt_ids, "gt_ids", who, (torch.int32,))
    t, _kind = _region_values(target, who)
    _region_same(who, pred_ids, gt_ids=gt_ids, target=t)
    capacity = _instance_capacity(capacity, gt_table, who)
    pred_table = _instance_rows(pred_table, "pred_table", who, b, capacity, 8)
    gt_table = _instance_rows(gt_table, "gt_table", who, b, capacity, 8)
    pred_ids, gt_ids = pred_ids.detach().contiguous(), gt_ids.detach().contiguous()
    dev, n = pred_ids.device, b * h * w
    nb = int(lib().vqseg_instance_vote_bits(capacity))
    pp, gp, tp = _i32(pred_ids, "pred_ids", n), _i32(gt_ids, "gt_ids", n), _T(t, "target", dtype=t.dtype, numel=n)
    _i32(pred_table, "pred_table", b * capacity * 8)
    gtp = _i32(gt_table, "gt_table", b * capacity * 8)
    vv = list(vd) + [0] * (4 - len(vd))
    if dev.type != "cuda":
        _launch("vqseg_instance_vote_i32", dev, pp, gp, tp, t.element_size(), b, h, w, capacity, len(vd), *vv, None, None)
    votes = torch.empty((b, capacity, nb), dtype=torch.int32, device=dev)
    void_count = torch.empty((b, capacity), dtype=torch.int32, device=dev)
    cand, inter = torch.empty_like(void_count), torch.empty_like(void_count)
    vp = _i32(votes, "votes", b * capacity * nb)
    _launch("vqseg_instance_vote_i32", dev, pp, gp, tp, t.element_size(), b, h, w, capacity, len(vd), *vv, vp, _i32(void_count, "void_count", b * capacity))
    _launch("vqseg_instance_overlap_i32", dev, pp, gp, vp, gtp, b, h, w, capacity, _i32(cand, "cand", b * capacity), _i32(inter, "inter", b * capacity))
    INSTANCE_CALLS += 1
    return cand, inter, void_count


def instance_tally(cand, inter, void_count, pred_table, gt_table, pred_counts, gt_counts, num_classes):
    """InstanceTally(match, inter, union, matched, tally, iou_sum, overflow) from instance_overlap's three tables, both region tables
    (B, capacity, 8) and both region counts (B,): match[b][g] the partner of ground-truth row g (equal value, 2 * inter > union) or
    -1, inter / union of the match (0 without one), matched[b][p] 1 for a prediction row with a partner; tally int32 (B, C, 5) = (tp,
    fp, fn, n_pred, n_gt) per class, iou_sum float64 (B, C) in rising ground-truth id, overflow int32 (B,) = a count exceeds the
    capacity (such an image matches nothing and counts nothing).  vqseg_instance_match_i32 and vqseg_instance_tally_i32: a memset
    and two small launches."""
    who = "instance_tally"
    if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or not 1 <= int(num_classes) <= INSTANCE_MAX_CLASSES:
        raise ValueError(f"{who}: num_classes must be an integer in 1..{INSTANCE_MAX_CLASSES}, got {num_classes!r}")
    c = int(num_classes)
    if not (torch.is_tensor(cand) and cand.dim() == 2 and 1 <= cand.shape[0] <= 65535 and 1 <= cand.shape[1] <= INSTANCE_MAX_CAPACITY):
        raise _hip.HipLibraryError(f"{who}: cand must be an int32 tensor (B, capacity) with 1..65535 images and 1..{INSTANCE_MAX_CAPACITY} rows, got "
                                   f"{tuple(getattr(cand, 'shape', ()))}")
    b, capacity = cand.shape
    cand = _instance_rows(cand, "cand", who, b, capacity)
    inter = _instance_rows(inter, "inter", who, b, capacity).clone()         # the match launch rewrites it
    void_count = _instance_rows(void_count, "void_count", who, b, capacity)
    pred_table = _instance_rows(pred_table, "pred_table", who, b, capacity, 8)
    gt_table = _instance_rows(gt_table, "gt_table", who, b, capacity, 8)
    pred_counts, gt_counts = _instance_counts(pred_counts, "pred_counts", who, b), _instance_counts(gt_counts, "gt_counts", who, b)
    dev, rows = cand.device, b * capacity
    _region_same(who, cand, inter=inter, void_count=void_count)
    for name, x in (("pred_table", pred_table), ("gt_table", gt_table), ("pred_counts", pred_counts), ("gt_counts", gt_counts)):
        if x.device != dev:
            raise _hip.HipLibraryError(f"{who}: all tensors must be on one device, got {dev} and {x.device} ({name})")
    cp, ip, vp = _i32(cand, "cand", rows), _i32(inter, "inter", rows), _i32(void_count, "void_count", rows)
    ptp, gtp = _i32(pred_table, "pred_table", rows * 8), _i32(gt_table, "gt_table", rows * 8)
    pcp, gcp = _i32(pred_counts, "pred_counts", b), _i32(gt_counts, "gt_counts", b)
    if dev.type != "cuda":
        _launch("vqseg_instance_match_i32", dev, cp, vp, ptp, gtp, pcp, gcp, b, capacity, ip, None, None, None)
    match, union, matched = torch.empty_like(cand), torch.empty_like(cand), torch.empty_like(cand)
    tally = torch.empty((b, c, 5), dtype=torch.int32, device=dev)
    iou_sum = torch.empty((b, c), dtype=torch.float64, device=dev)
    overflow = torch.empty((b,), dtype=torch.int32, device=dev)
    mp, up, dp = _i32(match, "match", rows), _i32(union, "union", rows), _i32(matched, "matched", rows)
    _launch("vqseg_instance_match_i32", dev, cp, vp, ptp, gtp, pcp, gcp, b, capacity, ip, mp, up, dp)
    _launch("vqseg_instance_tally_i32", dev, mp, dp, ip, up, vp, ptp, gtp, pcp, gcp, b, capacity, c, _i32(tally, "tally", b * c * 5),
            _T(iou_sum, "iou_sum", dtype=torch.float64, numel=b * c), _i32(overflow, "overflow", b))
    return InstanceTally(match, inter, union, matched, tally, iou_sum, overflow)


# ------------------------------------------------------------------------------------------------
# Boundary metrics (vqseg_boundary_*; include/vqseg.h states the definition, tests/boundary_cases.py restates it)
# ------------------------------------------------------------------------------------------------
EDT_NONE = 2 ** 31 - 1        # the squared distance on a plane without a seed
EDT_MAX_SIDE = 2048           # sides of a distance transform (the row pass keeps distances in 16 bits); REGION_MAX_SIDE is 4096
EDT_MAX_PLANES = 1 << 19      # planes per launch
BOUNDARY_MAX_CLASSES = 32
BOUNDARY_WORKSPACE_BYTES = 512 << 20          # boundary_counts: the int32 distance planes of one chunk of images stay under this
BOUNDARY_CALLS = 0            # calls of boundary_counts that reached the library (as REGION_CALLS: for tests, never read by the product)


def boundary_classes(num_classes, who="boundary"):
    if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or not 1 <= int(num_classes) <= BOUNDARY_MAX_CLASSES:
        raise ValueError(f"{who}: num_classes must be an integer in 1..{BOUNDARY_MAX_CLASSES}, got {num_classes!r}")
    return int(num_classes)


def boundary_threshold(value, name, who="boundary_counts"):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 0 <= int(value) <= EDT_NONE - 1:
        raise ValueError(f"{who}: {name} must be an integer in 0..2^31 - 2 (a squared distance), got {value!r}")
    return int(value)


def _boundary_labels(labels, name, who):
    """(the map as the kernels read it: uint8 or int32, int64 narrowed as _region_values does; b, h, w)"""
    E = _hip.HipLibraryError
    _region_shape(labels, name, who, REGION_VALUE_DTYPES + (torch.int64,))
    b, h, w = labels.shape
    if h > EDT_MAX_SIDE or w > EDT_MAX_SIDE:
        raise E(f"{who}: sides of 1..{EDT_MAX_SIDE}, got {tuple(labels.shape)}")
    v = labels.detach()
    v = (v.to(torch.int32) if v.dtype == torch.int64 else v).contiguous()
    return v, b, h, w


def boundaries_supported(labels) -> bool:
    """what the boundary kernels take: regions_supported with sides up to EDT_MAX_SIDE"""
    return regions_supported(labels) and labels.shape[1] <= EDT_MAX_SIDE and labels.shape[2] <= EDT_MAX_SIDE


def _boundary_seeds(v, c, ign):
    b, h, w = v.shape
    dev, n = v.device, b * h * w
    name = "vqseg_boundary_seeds_" + ("u8" if v.dtype == torch.uint8 else "i32")
    vp = _T(v, "labels", dtype=v.dtype, numel=n)
    ig = list(ign) + [0] * (4 - len(ign))
    if dev.type != "cuda":
        _launch(name, dev, vp, b, h, w, c, len(ign), *ig, None)
    seeds = torch.empty((b, c, h, w), dtype=torch.uint8, device=dev)
    _launch(name, dev, vp, b, h, w, c, len(ign), *ig, _T(seeds, "seeds", dtype=torch.uint8, numel=n * c))
    return seeds


def class_boundaries(labels, num_classes, ignore=()):
    """seeds uint8 (B, C, H, W) of 0 / 1 from `labels` (B, H, W) uint8 / int32 (int64 is converted) on the GPU: pixel p is a boundary
    pixel of class c when labels[p] == c and one of its 4-neighbours inside the image is neither c nor one of `ignore` (0 to 4
    integers).  The image border makes no boundary.  One launch (vqseg_boundary_seeds_u8 / _i32); sides up to 2048, B * C <= 2^19.
    There is no CPU form here (utils.boundary has one)."""
    c = boundary_classes(num_classes, "class_boundaries")
    _conn, ign = region_settings(4, ignore, "class_boundaries")
    v, b, _h, _w = _boundary_labels(labels, "labels", "class_boundaries")
    if b * c > EDT_MAX_PLANES:
        raise _hip.HipLibraryError(f"class_boundaries: at most 2^19 planes (B * num_classes), got {b} x {c}")
    return _boundary_seeds(v, c, ign)


def _edt_planes(seeds):
    """(planes, h, w) uint8 contiguous -> int32 squared distances: the row launch and the column launch"""
    planes, h, w = seeds.shape
    dev, n = seeds.device, planes * h * w
    sp = _T(seeds, "seeds", dtype=torch.uint8, numel=n)
    if dev.type != "cuda":
        _launch("vqseg_boundary_edt_rows_u8", dev, sp, planes, h, w, None, None)
    g = torch.empty((planes, h, w), dtype=torch.int16, device=dev)          # u16 on the device: torch has no arithmetic for it, none is needed
    row_has = torch.empty((planes, h), dtype=torch.uint8, device=dev)
    d2 = torch.empty((planes, h, w), dtype=torch.int32, device=dev)
    gp, rp = _T(g, "g", dtype=torch.int16, numel=n), _T(row_has, "row_has", dtype=torch.uint8, numel=planes * h)
    _launch("vqseg_boundary_edt_rows_u8", dev, sp, planes, h, w, gp, rp)
    _launch("vqseg_boundary_edt_cols_i32", dev, gp, rp, planes, h, w, _i32(d2, "d2", n))
    return d2


def edt_sq(seeds):
    """int32 squared Euclidean distances to the nearest non-zero pixel of `seeds` (..., H, W) uint8 or bool on the GPU, every leading
    dimension a batch of independent planes; EDT_NONE on a plane without a seed.  Exact: rint(scipy's distance_transform_edt(seeds ==
    0) ** 2) where the plane has a seed.  Two launches per 2^19 planes (vqseg_boundary_edt_rows_u8, vqseg_boundary_edt_cols_i32);
    sides up to 2048."""
    E = _hip.HipLibraryError
    if not (torch.is_tensor(seeds) and seeds.dim() >= 2):
        raise E(f"edt_sq: seeds must be a (..., H, W) tensor, got {tuple(getattr(seeds, 'shape', ()))}")
    if seeds.dtype not in (torch.uint8, torch.bool):
        raise E(f"edt_sq: seeds must be uint8 or bool, got {seeds.dtype}")
    h, w = seeds.shape[-2:]
    if not (1 <= h <= EDT_MAX_SIDE and 1 <= w <= EDT_MAX_SIDE) or seeds.numel() == 0:
        raise E(f"edt_sq: at least one plane with sides of 1..{EDT_MAX_SIDE}, got {tuple(seeds.shape)}")
    s = seeds.detach()
    s = (s.to(torch.uint8) if s.dtype == torch.bool else s).contiguous().view(-1, h, w)
    parts = [_edt_planes(s[k:k + EDT_MAX_PLANES]) for k in range(0, s.shape[0], EDT_MAX_PLANES)]
    return (parts[0] if len(parts) == 1 else torch.cat(parts)).view(seeds.shape)


def boundary_chunk(num_classes, h, w):
    """images per chunk of boundary_counts: 2 C int32 distance planes per image stay under BOUNDARY_WORKSPACE_BYTES, C B under 2^19"""
    per_image = 2 * num_classes * h * w * 4
    return max(1, min((BOUNDARY_WORKSPACE_BYTES - 1) // per_image, EDT_MAX_PLANES // num_classes))


def boundary_counts(pred, target, num_classes, tol_sq, width_sq, ignore=()):
    """table int32 (B, C, 8) = (n_pred, hit_pred, n_gt, hit_gt, band_inter, band_union, hd_pred_sq, hd_gt_sq) per image and class from
    the class maps `pred` and `target` (B, H, W) uint8 / int32 / int64 on the GPU -- include/vqseg.h states every column.  tol_sq =
    floor(tolerance^2), width_sq = floor(width^2); a pixel counts when its target is not one of `ignore`.  Per chunk of images (whose
    distance planes stay under 512 MiB): two boundary launches, two row and two column launches, the table preset and the counts."""
    global BOUNDARY_CALLS
    c = boundary_classes(num_classes, "boundary_counts")
    tol_sq, width_sq = boundary_threshold(tol_sq, "tol_sq"), boundary_threshold(width_sq, "width_sq")
    _conn, ign = region_settings(4, ignore, "boundary_counts")
    p, b, h, w = _boundary_labels(pred, "pred", "boundary_counts")
    t, _b, _h, _w = _boundary_labels(target, "target", "boundary_counts")
    _region_same("boundary_counts", p, target=t)
    dev = p.device
    ig = list(ign) + [0] * (4 - len(ign))
    if dev.type != "cuda":                                     # everything else is right: the device error, before anything is made
        n = b * h * w
        _launch("vqseg_boundary_counts_i32", dev, _T(p, "pred", dtype=p.dtype, numel=n), p.element_size(), _T(t, "target", dtype=t.dtype, numel=n),
                t.element_size(), None, None, None, None, b, h, w, c, tol_sq, width_sq, len(ign), *ig, None)
    table = torch.empty((b, c, 8), dtype=torch.int32, device=dev)
    step = boundary_chunk(c, h, w)
    for k in range(0, b, step):
        pk, tk = p[k:k + step], t[k:k + step]
        nb = pk.shape[0]
        n = nb * h * w
        bp, bg = _boundary_seeds(pk, c, ign), _boundary_seeds(tk, c, ign)
        dp, dg = _edt_planes(bp.view(nb * c, h, w)), _edt_planes(bg.view(nb * c, h, w))
        _launch("vqseg_boundary_counts_i32", dev, _T(pk, "pred", dtype=pk.dtype, numel=n), pk.element_size(),
                _T(tk, "target", dtype=tk.dtype, numel=n), tk.element_size(), _T(bp, "bp", dtype=torch.uint8, numel=n * c),
                _T(bg, "bg", dtype=torch.uint8, numel=n * c), _i32(dp, "dp", n * c), _i32(dg, "dg", n * c), nb, h, w, c, tol_sq, width_sq,
                len(ign), *ig, _i32(table[k:k + step], "table", nb * c * 8))
    BOUNDARY_CALLS += 1
    return table


# ------------------------------------------------------------------------------------------------
# Feature perturbation: channel dropout of the decoder's inputs, fused with the concatenation that doubles the batch
# (vqseg_channel_keep_f, vqseg_channel_dropout_cat_f, vqseg_channel_dropout_fold_f; include/vqseg.h states the definition).
# The reference's UniMatch stream is decoder(torch.cat((f, nn.Dropout2d(0.5)(f)))) (deprecated/train_UNIMatch.py:172,183-185).
# CPU tensors, and anything the kernels do not take, use the torch-op form of the SAME definition -- the Philox draw in int64
# tensor ops, the product and the sum as separate float32 operators -- so a result is the same bits wherever it is computed;
# VQSEG_OPTS=py_feature_perturb=0 forces that form on the device (A/B runs).
# ------------------------------------------------------------------------------------------------
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57             # the round multipliers of Philox4x32
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85             # the key's Weyl increments
_U32 = 0xffffffff
CHANNEL_DROPOUT_DTYPES = (torch.float32, torch.bfloat16)


def _mulhilo32(m: int, v: torch.Tensor):
    """(hi, lo) words of the 64-bit product m * v for a 32-bit constant m and an int64 tensor v of 32-bit values: 16-bit halves keep
    every intermediate below 2^49"""
    low = m * (v & 0xffff)
    mid = m * (v >> 16) + (low >> 16)
    return mid >> 16, ((mid & 0xffff) << 16) | (low & 0xffff)


def philox4x32(counter, key, rounds: int = 10, device=None):
    """Philox4x32 (ten rounds by default) with torch integer ops: `counter` four and `key` two 32-bit words, each an int or an int64
    tensor (broadcast against each other) -> the block's four words as int64 tensors.  What channel_keep_kernel computes."""
    c = [torch.as_tensor(v, dtype=torch.int64, device=device) & _U32 for v in counter]
    k0, k1 = (torch.as_tensor(v, dtype=torch.int64, device=device) & _U32 for v in key)
    c0, c1, c2, c3 = torch.broadcast_tensors(*c)
    for _ in range(rounds):
        hi0, lo0 = _mulhilo32(PHILOX_M0, c0)
        hi1, lo1 = _mulhilo32(PHILOX_M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + PHILOX_W0) & _U32, (k1 + PHILOX_W1) & _U32
    return c0, c1, c2, c3


def channel_keep_params(p):
    """-> (threshold, inv_keep) of a drop probability 0 <= p < 1: clamp(round(p 2^32), 0, 2^32 - 1), and 1 / (1 - p) rounded to float32
    (returned as the Python float of that value)"""
    if isinstance(p, bool) or not isinstance(p, (int, float, np.floating, np.integer)) or not 0.0 <= float(p) < 1.0:
        raise ValueError(f"channel_keep: the drop probability must lie in [0, 1), got {p!r}")
    p = float(p)
    return min(max(int(np.floor(p * 4294967296.0 + 0.5)), 0), _U32), float(np.float32(1.0 / (1.0 - p)))


def _u_int(v, bits, name):
    if isinstance(v, bool) or int(v) != v or not 0 <= int(v) < (1 << bits):
        raise ValueError(f"channel_keep: {name} must be an integer in [0, 2^{bits}), got {v!r}")
    return int(v)


def channel_keep(sizes, p, seed, stream, step, device):
    """The keep / scale table of one perturbed forward -> (flat float32 table, [one (B, C_l) view per level]).  `sizes`: the levels'
    (B, C_l), one B.  Element e of the flat table (level-major: level l at offset B * sum_{j<l} C_j) is 1 / (1 - p) where word 0 of
    Philox4x32-10(counter (e, stream, step_lo, step_hi), key (seed_lo, seed_hi)) >= round(p 2^32), else 0: a pure function of its
    arguments -- no generator state, no host-to-device copy, one launch (vqseg_channel_keep_f) for all levels."""
    sizes = [(int(b), int(c)) for b, c in sizes]
    if not sizes or any(b < 1 or c < 1 for b, c in sizes) or len({b for b, _c in sizes}) != 1:
        raise ValueError(f"channel_keep: sizes must be (B, C_l) pairs of one positive B and positive C_l, got {sizes!r}")
    threshold, inv_keep = channel_keep_params(p)
    seed, stream, step = _u_int(seed, 64, "seed"), _u_int(stream, 32, "stream"), _u_int(step, 64, "step")
    total = sum(b * c for b, c in sizes)
    if total > _U32:
        raise ValueError(f"channel_keep: {total} table elements, above 2^32 - 1 (the element index is one counter word)")
    dev = torch.device(device)
    if dev.type == "cuda" and py_opt("py_feature_perturb", 1) == 1:
        flat = torch.empty(total, dtype=torch.float32, device=dev)
        _launch("vqseg_channel_keep_f", dev, _f32(flat, "scale", total), total, seed, stream, step, threshold, inv_keep)
    else:
        e = torch.arange(total, dtype=torch.int64, device=dev)
        word0 = philox4x32((e, stream, step & _U32, step >> 32), (seed & _U32, seed >> 32), device=dev)[0]
        flat = torch.where(word0 >= threshold, inv_keep, 0.0).to(torch.float32)
    views, at = [], 0
    for b, c in sizes:
        views.append(flat[at:at + b * c].view(b, c))
        at += b * c
    return flat, views


def _cl_format(x):
    """the memory format channel_dropout_cat's output takes: x's when x is dense in one of the two, else contiguous"""
    if x.is_contiguous() or not x.is_contiguous(memory_format=torch.channels_last):
        return torch.contiguous_format
    return torch.channels_last


def channel_dropout_supported(x) -> bool:
    """what the kernels take: a non-empty float32 / bfloat16 (B, C, H, W) tensor on the GPU, NCHW-contiguous or channels_last"""
    return (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.dtype in CHANNEL_DROPOUT_DTYPES and x.numel() > 0
            and (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last))
            and x.shape[1] * x.shape[2] * x.shape[3] <= 1 << 40 and x.shape[0] * x.shape[1] <= 1 << 31)


def _compute_dtype(t):
    return torch.float64 if t.dtype == torch.float64 else torch.float32


def _dropout_cat_torch(x, scale):
    n = x.shape[0]
    s = scale[:, :, None, None]
    ct = _compute_dtype(x)
    out = torch.empty((2 * n,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device, memory_format=_cl_format(x))
    out[:n].copy_(x)
    out[n:].copy_(torch.where(s == 0, torch.zeros((), dtype=x.dtype, device=x.device), (x.to(ct) * s.to(ct)).to(x.dtype)))
    return out


def _dropout_fold_torch(g, scale):
    n = g.shape[0] // 2
    s = scale[:, :, None, None]
    ct = _compute_dtype(g)
    return torch.where(s == 0, g[:n], (g[:n].to(ct) + g[n:].to(ct) * s.to(ct)).to(g.dtype))


def _dropout_launch(name, src, scale, dst, n, c, h, w):
    bf = _is_bf16(src)
    _launch(name, src.device, bf, _T(src, "x" if dst.shape[0] > src.shape[0] else "g", bf=bf, numel=src.numel()),
            _f32(scale, "scale", n * c), _T(dst, "out", bf=bf, numel=dst.numel()), n, c, h, w, int(not src.is_contiguous()))


class _ChannelDropoutCat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale, hip):
        n, c, h, w = x.shape
        ctx.save_for_backward(scale)
        ctx.hip, ctx.fmt = hip, _cl_format(x)
        if not hip:
            return _dropout_cat_torch(x, scale)
        out = torch.empty((2 * n, c, h, w), dtype=x.dtype, device=x.device, memory_format=ctx.fmt)
        _dropout_launch("vqseg_channel_dropout_cat_f", x, scale, out, n, c, h, w)
        return out

    @staticmethod
    def backward(ctx, g):
        (scale,) = ctx.saved_tensors
        if not ctx.hip:
            return _dropout_fold_torch(g, scale), None, None
        n, c, h, w = g.shape[0] // 2, g.shape[1], g.shape[2], g.shape[3]
        g = g.contiguous(memory_format=ctx.fmt)              # (the forward's layout; the decoder's gradients arrive in it)
        gx = torch.empty((n, c, h, w), dtype=g.dtype, device=g.device, memory_format=ctx.fmt)
        _dropout_launch("vqseg_channel_dropout_fold_f", g, scale, gx, n, c, h, w)
        return gx, None, None


def channel_dropout_cat(x, scale):
    """torch.cat((x, dropout(x))) in one pass: x (B, C, H, W), scale float32 (B, C) (a level's view of channel_keep's table) ->
    (2B, C, H, W) of x's dtype and layout with out[:B] = x by bits and out[B + n, c] = +0.0 where scale[n, c] == 0 (a selection: an
    Inf or NaN activation of a dropped channel does not leak), else x[n, c] * scale[n, c] (the float32 product, rounded once more
    for bfloat16).  Backward: gx = g[:B] + g[B:] * scale with the product rounded to float32 before the add, and g[:B] alone where
    the channel was dropped; no gradient flows to `scale`.  float32 / bfloat16 tensors on the GPU run the HIP kernels; everything
    else (and everything under VQSEG_OPTS=py_feature_perturb=0) the torch-op form of the same definition."""
    E = _hip.HipLibraryError
    if not (torch.is_tensor(x) and x.dim() == 4 and x.is_floating_point()):
        raise E("channel_dropout_cat: x must be a floating-point (B, C, H, W) tensor")
    if not (torch.is_tensor(scale) and scale.dtype == torch.float32 and tuple(scale.shape) == tuple(x.shape[:2])):
        raise E(f"channel_dropout_cat: scale must be a float32 (B, C) = {tuple(x.shape[:2])} tensor, got "
                f"{tuple(scale.shape) if torch.is_tensor(scale) else type(scale).__name__}"
                f"{' of ' + str(scale.dtype) if torch.is_tensor(scale) else ''}")
    if scale.device != x.device:
        raise E(f"channel_dropout_cat: x and scale must be on one device, got {x.device} and {scale.device}")
    if x.numel() == 0:
        raise E("channel_dropout_cat: empty tensor")
    scale = scale.detach().contiguous()
    return _ChannelDropoutCat.apply(x, scale, channel_dropout_supported(x) and py_opt("py_feature_perturb", 1) == 1)
