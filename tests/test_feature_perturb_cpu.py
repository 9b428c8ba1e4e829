"""The feature-perturbation stream without a GPU: the torch-op form of the definition in include/vqseg.h (the Philox draw, the keep
table's layout, channel_dropout_cat forward and backward), the configuration's checks, and the model's `need_fp` plumbing on a CPU
model whose convolutional parts are stood in for by plain torch modules (the accelerated layers take no CPU tensors)."""
import numpy as np
import pytest
import torch
from torch import nn

from vq_seg_amd import _hip, nnf


def _words(counter, key):
    return [int(w) for w in nnf.philox4x32(counter, key)]


# Known answers of Philox4x32-10 (the Random123 distribution's kat_vectors: counter / key -> the block's four words)
KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    assert tuple(_words(counter, key)) == want
    # ... and as tensors of several counters at once (what channel_keep does)
    e = torch.tensor([counter[0], counter[0]], dtype=torch.int64)
    got = nnf.philox4x32((e, counter[1], counter[2], counter[3]), key)
    assert all(w.dtype == torch.int64 and w.tolist() == [v, v] for w, v in zip(got, want))


def test_threshold_and_scale_of_a_probability():
    assert nnf.channel_keep_params(0) == (0, 1.0)
    assert nnf.channel_keep_params(0.5) == (1 << 31, 2.0)
    t, inv = nnf.channel_keep_params(0.25)
    assert t == 1 << 30 and inv == float(np.float32(4.0 / 3.0)) and np.float32(inv) == inv
    assert nnf.channel_keep_params(1.0 - 2.0 ** -40)[0] == 0xffffffff               # clamped: round(p 2^32) would be 2^32
    for bad in (1.0, -0.25, 1.5, float("nan"), True, "0.5", None):
        with pytest.raises(ValueError, match="drop probability"):
            nnf.channel_keep_params(bad)


def test_p_zero_keeps_everything():
    flat, views = nnf.channel_keep([(3, 5), (3, 2)], 0.0, 1, 2, 3, "cpu")
    assert flat.dtype == torch.float32 and torch.equal(flat, torch.ones(21))


def test_table_layout_is_level_major():
    sizes = [(3, 64), (3, 257), (3, 8)]
    flat, views = nnf.channel_keep(sizes, 0.5, 42, 1, 9, "cpu")
    assert flat.shape == (3 * (64 + 257 + 8),) and [tuple(v.shape) for v in views] == sizes
    at = 0
    for (b, c), v in zip(sizes, views):
        assert v.data_ptr() == flat.data_ptr() + 4 * at and v.is_contiguous()       # a view of the one table, at B * sum of the C before
        assert torch.equal(v.reshape(-1), flat[at:at + b * c])
        at += b * c
    # element e depends on e alone: the same draw as one level
    one, _ = nnf.channel_keep([(1, flat.numel())], 0.5, 42, 1, 9, "cpu")
    assert torch.equal(one, flat)
    assert set(flat.tolist()) == {0.0, 2.0}
    # ... and is the documented word of the documented block
    for e in (0, 1, 200, flat.numel() - 1):
        w0 = _words((e, 1, 9, 0), (42, 0))[0]
        assert float(flat[e]) == (2.0 if w0 >= 1 << 31 else 0.0)
    big, _ = nnf.channel_keep([(1, 4)], 0.5, (7 << 32) | 5, 3, (2 << 32) | 11, "cpu")   # the high words of seed and step are key / counter words
    assert big.tolist() == [2.0 if _words((e, 3, 11, 2), (5, 7))[0] >= 1 << 31 else 0.0 for e in range(4)]
    for bad in ([], [(2, 3), (3, 3)], [(0, 3)], [(2, 0)]):
        with pytest.raises(ValueError, match="sizes"):
            nnf.channel_keep(bad, 0.5, 0, 0, 0, "cpu")
    for kw in (dict(seed=-1), dict(stream=1 << 32), dict(step=1 << 64), dict(seed=0.5)):
        with pytest.raises(ValueError, match="must be an integer"):
            nnf.channel_keep([(1, 4)], 0.5, **{**dict(seed=0, stream=0, step=0), **kw}, device="cpu")


def test_kept_share_of_a_large_draw():
    """65 536 independent keeps at p = 0.5: the count is binomial with sigma = 128, so within 4 sigma = 512 of one half"""
    flat, _ = nnf.channel_keep([(1, 65536)], 0.5, 42, 0, 0, "cpu")
    kept = int((flat != 0).sum())
    print("kept", kept, "of 65536")
    assert abs(kept - 32768) <= 512


def test_draws_change_with_seed_stream_and_step():
    base = dict(seed=42, stream=0, step=0)
    ref, _ = nnf.channel_keep([(4, 256)], 0.5, device="cpu", **base)
    again, _ = nnf.channel_keep([(4, 256)], 0.5, device="cpu", **base)
    assert torch.equal(ref, again)
    for key in base:
        other, _ = nnf.channel_keep([(4, 256)], 0.5, device="cpu", **{**base, key: base[key] + 1})
        differ = int((other != ref).sum())
        assert 1024 // 2 - 4 * 16 <= differ <= 1024 // 2 + 4 * 16, (key, differ)       # independent halves: binomial(1024, 1/2), sigma 16


def _scale(b, c, p=0.5, seed=3):
    return nnf.channel_keep([(b, c)], p, seed, 0, 0, "cpu")[1][0]


def test_gradcheck_of_the_torch_op_form():
    scale = _scale(2, 5, 0.25)
    assert 0 < int((scale == 0).sum()) < scale.numel()
    for fmt in (torch.contiguous_format, torch.channels_last):
        x = torch.randn(2, 5, 3, 4, dtype=torch.float64).contiguous(memory_format=fmt).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda t: nnf.channel_dropout_cat(t, scale), (x,))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_a_dropped_channel_is_a_selection_forward_and_backward(dtype):
    scale = torch.tensor([[0.0, 2.0, 0.0], [2.0, 0.0, 2.0]])
    x = torch.randn(2, 3, 2, 2).to(dtype)
    for n, c, v in ((0, 0, float("inf")), (0, 2, float("nan")), (1, 1, float("-inf")), (0, 1, float("inf")), (1, 0, -0.0)):
        x[n, c, 0, 0] = v
    x.requires_grad_(True)
    out = nnf.channel_dropout_cat(x, scale)
    assert out.shape == (4, 3, 2, 2) and out.dtype == dtype
    bits = lambda t: t.detach().contiguous().view(torch.int16 if dtype == torch.bfloat16 else torch.int32)
    assert torch.equal(bits(out[:2]), bits(x))                                      # the clean half: by bits
    dropped = (scale == 0)[:, :, None, None].expand(2, 3, 2, 2)
    assert int(bits(out[2:])[dropped].abs().sum()) == 0                             # +0.0, whatever the activation was
    assert float(out.detach()[2, 1, 0, 0]) == float("inf") and torch.equal(out.detach()[2:][~dropped], (2 * x.detach())[~dropped])
    assert bits(out[3, 0, 0, 0]) == bits(torch.tensor(-0.0, dtype=dtype))           # a kept -0.0 stays -0.0
    g = torch.randn(4, 3, 2, 2).to(dtype)
    g[2, 0, 1, 1], g[2, 2, 0, 1], g[3, 1, 0, 0] = float("nan"), float("inf"), float("-inf")      # second-half gradients of dropped channels
    (gx,) = torch.autograd.grad(out, x, g)
    assert torch.equal(bits(gx)[dropped], bits(g[:2])[dropped])                     # the first half alone, by bits: nothing leaked
    want = (g[:2].float() + g[2:].float() * 2.0).to(dtype)
    assert torch.equal(bits(gx)[~dropped], bits(want)[~dropped])
    assert not scale.requires_grad


def test_argument_checks():
    E = _hip.HipLibraryError
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(E, match="scale must be a float32"):
        nnf.channel_dropout_cat(x, torch.ones(2, 4))
    with pytest.raises(E, match="scale must be a float32"):
        nnf.channel_dropout_cat(x, torch.ones(2, 3, dtype=torch.float64))
    with pytest.raises(E, match=r"\(B, C, H, W\)"):
        nnf.channel_dropout_cat(torch.zeros(2, 3, 4), torch.ones(2, 3))
    assert not nnf.channel_dropout_supported(x) and not nnf.channel_dropout_supported(None)      # a CPU tensor: the torch-op form
    L = _hip.lib()
    for name in ("vqseg_channel_keep_f", "vqseg_channel_dropout_cat_f", "vqseg_channel_dropout_fold_f"):
        assert name in _hip.SYMBOLS and hasattr(L, name)
    assert L.vqseg_channel_keep_f(None, 4, 0, 0, 0, 0, 1.0, None) == -1 and b"null" in L.vqseg_last_error()
    assert L.vqseg_channel_dropout_cat_f(0, None, None, None, 1, 1, 1, 1, 0, None) == -1 and b"null" in L.vqseg_last_error()
    assert L.vqseg_channel_dropout_fold_f(2, None, None, None, 1, 1, 1, 1, 0, None) == -1 and b"bf16 must be" in L.vqseg_last_error()


def test_config_validation():
    from vq_seg_amd.trainer import CPSConfig
    cfg = CPSConfig(model={})
    assert cfg.feature_perturb is None and cfg.feature_perturb_weight == 0.5
    cfg = CPSConfig(model={}, feature_perturb=0, feature_perturb_weight=0)
    assert cfg.feature_perturb == 0.0 and isinstance(cfg.feature_perturb, float)
    assert CPSConfig(model={}, recipe="v2", feature_perturb=0.5).feature_perturb == 0.5
    for bad in (1.0, -0.1, 2, float("nan"), "0.5", True):
        with pytest.raises(ValueError, match=r"feature_perturb must be None or a drop probability in \[0, 1\)"):
            CPSConfig(model={}, feature_perturb=bad)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="feature_perturb_weight"):
            CPSConfig(model={}, feature_perturb=0.5, feature_perturb_weight=bad)
    with pytest.raises(ValueError, match="does not combine with unsup_criterion='conf_ce'"):
        CPSConfig(model={}, feature_perturb=0.5, unsup_criterion="conf_ce")
    assert CPSConfig(model={}, unsup_criterion="conf_ce").feature_perturb is None   # each alone is fine


# ---- the model's plumbing on the CPU ---------------------------------------------------------------------------------------------------
class _Encoder(nn.Module):
    """six feature maps of a (B, 3, 16, 16) image from plain convolutions: index 0 is dropped by the model, as the real encoder's"""
    CH = (3, 4, 6, 8, 10, 12)

    def __init__(self):
        super().__init__()
        self.convs = nn.ModuleList(nn.Conv2d(3, c, 1) for c in self.CH[1:])

    def out_channels(self):
        return self.CH

    def forward(self, x):
        return [x] + [conv(x[:, :, ::2 ** i, ::2 ** i]) for i, conv in enumerate(self.convs)]


class _Decoder(nn.Module):
    def __init__(self):
        super().__init__()
        self.mix = nn.ModuleList(nn.Conv2d(c, 5, 1) for c in _Encoder.CH[1:])
        self.bn = nn.BatchNorm2d(5)
        self.batches = []

    def forward(self, *feats):
        self.batches.append([f.shape[0] for f in feats])
        size = feats[0].shape[-2:]
        return self.bn(sum(nn.functional.interpolate(m(f), size=size) for m, f in zip(self.mix, feats)))


class _Proto(nn.Module):
    def forward(self, decoder_out, gt, *a, **k):
        self.seen = decoder_out.shape
        return decoder_out.float().mean()


def _cpu_model(name):
    from vq_seg_amd.models.networks import make_model
    m = make_model({"name": name, "params": {"encoder_name": "resnet50", "num_classes": 3, "depth": 5, "encoder_weights": None,
                                             "vq_cfg": {"num_embeddings": [0, 0, 0, 0, 0]}}})
    m.encoder, m.decoder, m.prototype_loss = _Encoder(), _Decoder(), _Proto()
    m.segmentation_head = nn.Conv2d(5, 3, 1, bias=False)
    m.upsampling = nn.Upsample(scale_factor=2)
    return m


@pytest.mark.parametrize("name", ["vqreptunet1x1", "vqreptunet1x1v2"])
def test_need_fp_appends_the_perturbed_prediction_and_is_refused_in_eval_mode(name, monkeypatch):
    from vq_seg_amd.models.networks.modified_vqunet import net
    monkeypatch.setattr(net, "_to_device_layout", lambda x: x)
    m = _cpu_model(name)
    x, gt = torch.randn(2, 3, 16, 16), torch.randint(0, 3, (2, 16, 16))
    m.train()
    plain = m(x, gt)
    assert len(plain) == 4 and m.decoder.batches[-1] == [2] * 5
    off = m(x, gt, need_fp=False)
    assert len(off) == 4 and torch.equal(off[0], plain[0])
    out = m(x, gt, need_fp=True)
    assert len(out) == 5 and out[4].shape == out[0].shape == (2, 3, 32, 32)
    assert m.decoder.batches[-1] == [4] * 5 and m.prototype_loss.seen[0] == 2         # 2B through the decoder, the clean half to the loss
    assert not torch.equal(out[4], out[0])
    spec = dict(p=0.0, seed=1, stream=2, step=3)
    same = m(x, gt, need_fp=spec)                                                  # p = 0: the perturbed half is a duplicate
    assert torch.allclose(same[4], same[0], atol=1e-6) and torch.equal(spec["scale"], torch.ones(2 * sum(_Encoder.CH[1:])))
    spec = dict(p=0.5, seed=1, stream=2, step=3)
    a, b = m(x, gt, need_fp=spec)[4], m(x, gt, need_fp=dict(spec))[4]
    assert torch.equal(a, b)                                                        # the draw is a function of the spec
    assert torch.equal(spec["scale"], nnf.channel_keep([(2, c) for c in _Encoder.CH[1:]], 0.5, 1, 2, 3, "cpu")[0])
    side = dict(perturb=dict(spec))
    c = m.finish(*m.quantize(m.encode(x)), gt=gt, side=side)
    assert len(c) == 5 and torch.equal(c[4], a) and "scale" in side["perturb"]
    out[4].sum().backward()
    g = m.encoder.convs[0].weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and bool(g.any())
    m.eval()
    assert len(m(x)) == 4
    with pytest.raises(RuntimeError, match="training-mode option"):
        m(x, need_fp=True)
    with pytest.raises(RuntimeError, match="training-mode option"):
        m.finish(*m.quantize(m.encode(x)), side=dict(perturb=dict(spec)))
