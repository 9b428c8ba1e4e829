"""`forward(need_fp=...)` of the VQ-UNet on the GPU (the 64 x 64, batch 2, 64-code model of tests/test_conf_ce_trainer_gpu.py): the
perturbed stream's prediction with the HIP op and with its torch-op form is the same bits (the op is bit-exact, everything around it
is the same kernels on the same inputs); with p = 0 the two halves of the 2B decoder batch are duplicates, so `output_fp` stays
within the logit bar (1e-3 of the tensor's scale) of the clean output -- only the order of the BatchNorm reductions over 2B images
differs; the gradient of `output_fp` reaches the first encoder convolution; need_fp=False is the call without the keyword."""
import pytest
import torch

from tests import extent as E
from vq_seg_amd import _hip, nnf

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _cfg(name):
    return {"name": name, "params": {"encoder_name": "resnet50", "num_classes": 3, "depth": 5,
                                     "vq_cfg": {"num_embeddings": [0, 0, 64, 64, 64], "distance": "euclidean", "kmeans_init": True},
                                     "margin": 0.0, "scale": 1.0, "use_feature": False, "encoder_weights": None}}


def _model(name="vqreptunet1x1"):
    from vq_seg_amd.models.networks import make_model
    from vq_seg_amd.trainer import SyntheticCropWeed
    torch.manual_seed(3)
    m = make_model(_cfg(name)).to(DEV).train()
    x, gt = SyntheticCropWeed(64, 2, DEV, seed=5).labelled()
    kw = dict(percent=80.0) if name == "vqreptunet1x1" else dict(th=0.7)
    m(x, gt, **kw)                                              # the first training forward initialises the codebooks (k-means)
    return m, x, gt, kw


def _same(a, b):
    return E.same_bits(a.detach(), b.detach())


@pytest.mark.parametrize("amp", [None, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", ["vqreptunet1x1", "vqreptunet1x1v2"])
def test_hip_op_and_torch_op_form_give_the_same_bits(name, amp, monkeypatch):
    m, x, gt, kw = _model(name)
    names, real = [], nnf._launch
    monkeypatch.setattr(nnf, "_launch", lambda n_, *a, **k: (names.append(n_), real(n_, *a, **k))[1])
    spec = dict(p=0.5, seed=42, stream=1, step=7)

    def run():
        s = dict(spec)
        with torch.autocast("cuda", dtype=amp, enabled=amp is not None), torch.no_grad():
            return m(x, gt, need_fp=s, **kw), s["scale"]

    out_hip, scale_hip = run()
    count = lambda pre: sum(n_.startswith(pre) for n_ in names)
    assert count("vqseg_channel_keep_f") == 1 and count("vqseg_channel_dropout_cat_f") == 5
    monkeypatch.setitem(_hip.PY_OPTS, "py_feature_perturb", 0)
    names.clear()
    out_py, scale_py = run()
    assert count("vqseg_channel_") == 0
    assert len(out_hip) == len(out_py) == 5 and out_hip[4].shape == out_hip[0].shape == (2, 3, 64, 64)
    assert _same(scale_hip, scale_py) and 0 < int((scale_hip == 0).sum()) < scale_hip.numel()
    for i in (0, 1, 3, 4):
        assert _same(out_hip[i], out_py[i]), i
    assert not _same(out_hip[4], out_hip[0])


def test_p_zero_reproduces_the_clean_output_within_the_logit_bar():
    m, x, gt, kw = _model()
    out = m(x, gt, need_fp=dict(p=0.0, seed=1, stream=0, step=0), **kw)
    torch.cuda.synchronize()
    clean, fp = out[0].detach().float(), out[4].detach().float()
    err, scale = float((fp - clean).abs().max()), float(clean.abs().max())
    print(f"p = 0: max |output_fp - output| = {err:.3e}, max |output| = {scale:.3e}, bar {1e-3 * scale:.3e}")
    assert err <= 1e-3 * scale


def test_gradient_of_the_perturbed_prediction_reaches_the_first_encoder_convolution():
    m, x, gt, kw = _model()
    m.zero_grad(set_to_none=True)
    out = m(x, gt, need_fp=True, **kw)
    out[4].float().sum().backward()
    nnf.flush_pending_wgrads()
    torch.cuda.synchronize()
    g = m.encoder.conv1.weight.grad
    assert g is not None and bool(torch.isfinite(g).all()) and bool(g.any())
    for p in m.decoder.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())


def test_need_fp_false_is_the_call_without_the_keyword_and_eval_mode_refuses():
    m, x, gt, kw = _model()
    with torch.no_grad():
        a, b = m(x, gt, **kw), m(x, gt, need_fp=False, **kw)
    assert len(a) == len(b) == 4
    for i in (0, 1, 3):
        assert _same(a[i], b[i]), i
    m.eval()
    with torch.no_grad():
        assert len(m(x)) == 4
        with pytest.raises(RuntimeError, match="training-mode option"):
            m(x, need_fp=True)
