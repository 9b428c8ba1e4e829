"""The dense-CRF kernels (vqseg_crf_prepare_f, vqseg_crf_step_f through nnf.dense_crf) against the float64 restatement of
tests/crf_cases.py.

The bar follows the project's rule (tests/test_conf_ce_kernel_gpu.py): per case and iteration count the float32 torch-op form of the
same contract (utils.crf.mean_field_torch, dtype=float32, on the CPU) is measured against float64, and the kernel is allowed 4x
that error plus one float32 ulp of 1.0 on Q.  Labels must equal float64's at every pixel -- the case maker keeps every pixel's
top-two gap above 1e-4, so none is excluded.  The measured errors are printed (pytest -s) and recorded in profiles/crf.md."""
import functools

import numpy as np
import pytest
import torch

from tests import crf_cases
from vq_seg_amd import nnf
from vq_seg_amd.utils.crf import mean_field_torch

pytestmark = pytest.mark.gpu

ULP = float(np.finfo(np.float32).eps)
LAYOUTS = {"nchw": torch.contiguous_format, "nhwc": torch.channels_last}


@functools.lru_cache(maxsize=None)
def f32_error(shape, setting):
    """{t: max |float32 torch-op form - float64| over the batch}: the error float32 arithmetic itself makes on this case"""
    images, probs, ref = crf_cases.case(shape, setting)
    err = {t: 0.0 for t in crf_cases.ITERS}
    for n in range(shape[0]):
        keep = {}
        mean_field_torch(torch.from_numpy(images[n].copy()), torch.from_numpy(probs[n].copy()), iter_max=max(crf_cases.ITERS), dtype=torch.float32,
                         keep=keep, **crf_cases.SETTINGS[setting])
        for t in crf_cases.ITERS:
            err[t] = max(err[t], float(np.abs(keep[t].double().numpy() - ref[t][n]).max()))
    return err


def on_gpu(shape, setting, layout):
    images, probs, ref = crf_cases.case(shape, setting)
    x = torch.from_numpy(images.copy()).cuda().contiguous(memory_format=LAYOUTS[layout])
    p = torch.from_numpy(probs.copy()).cuda().contiguous(memory_format=LAYOUTS[layout])
    return x, p, ref


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("setting", sorted(crf_cases.SETTINGS))
@pytest.mark.parametrize("shape", crf_cases.SHAPES, ids=str)
def test_kernels_meet_the_float32_bar_and_the_float64_labels(shape, setting, layout):
    x, p, ref = on_gpu(shape, setting, layout)
    assert nnf.dense_crf_supported(x, p)
    assert shape[0] == 1 or not np.array_equal(crf_cases.case(shape, setting)[0][0], crf_cases.case(shape, setting)[0][1])
    base = f32_error(shape, setting)
    changed = 0.0
    for t in crf_cases.ITERS:
        kw = dict(crf_cases.SETTINGS[setting], iter_max=t)
        q = nnf.dense_crf(x, p, **kw)
        e = nnf.dense_crf(x, p, out="logits", **kw)
        assert q.dtype == torch.float32 and tuple(q.shape) == shape and q.is_contiguous()
        got = q.double().cpu().numpy()
        err = float(np.abs(got - ref[t]).max())
        bar = 4.0 * base[t] + ULP
        soft = torch.softmax(e.double(), dim=1)
        err_logits = float((soft - q.double()).abs().max())
        print(f"crf {shape} {setting} {layout} iters={t}: kernel {err:.3g}  float32 form {base[t]:.3g}  bar {bar:.3g}  softmax(logits)-prob {err_logits:.3g}")
        assert err <= bar
        assert err_logits <= bar
        assert float(np.abs(soft.cpu().numpy() - ref[t]).max()) <= bar
        assert np.array_equal(got.argmax(axis=1), ref[t].argmax(axis=1))
        assert np.array_equal(e.cpu().numpy().argmax(axis=1), ref[t].argmax(axis=1))
        changed = float((ref[t].argmax(axis=1) != crf_cases.case(shape, setting)[1].argmax(axis=1)).mean())
    assert changed > 0.03                                        # the refinement moves labels: a kernel that does nothing fails


def test_no_iterations_give_the_clipped_renormalised_input():
    x, p, _ = on_gpu(crf_cases.SHAPES[2], "cut", "nchw")
    p = p.clone()
    p[:, :, 0, 0] = torch.tensor([0.0, 1.0, 0.0, 0.0], device=p.device)
    clipped = p.double().clamp(1e-5, 1.0)
    want = clipped / clipped.sum(dim=1, keepdim=True)
    assert (nnf.dense_crf(x, p, iter_max=0).double() - want).abs().max() <= 2 * ULP      # a float32 sum and a division
    # -U = log(clip p) down to log(1e-5) = -11.5, where a float32 ulp is 2^-20 = 9.5e-7: the 3 ulp OpenCL allows a float log, plus
    # 2.5e-8 for the clip threshold 1e-5 rounded to float32
    assert (nnf.dense_crf(x, p, iter_max=0, out="logits").double() - clipped.log()).abs().max() <= 3 * 2.0 ** -20 + 2.5e-8
    # E = -U with |U| <= 11.6 carries half an ulp of 16 (4.8e-7) into the exponent, the softmax a few ulp more
    assert (nnf.dense_crf(x, p, iter_max=3, bi_w=0.0, pos_w=0.0).double() - want).abs().max() <= 1e-6


@pytest.mark.parametrize("setting", sorted(crf_cases.SETTINGS))
def test_two_calls_are_bit_identical(setting):
    x, p, _ = on_gpu(crf_cases.SHAPES[0], setting, "nhwc")
    kw = dict(crf_cases.SETTINGS[setting], iter_max=3)
    a, b = nnf.dense_crf(x, p, **kw), nnf.dense_crf(x, p, **kw)
    assert torch.equal(a, b)
    assert torch.equal(nnf.dense_crf(x, p, out="logits", **kw), nnf.dense_crf(x, p, out="logits", **kw))
    # ... and the storage layout does not change a bit of the result
    assert torch.equal(a, nnf.dense_crf(x.contiguous(), p.contiguous(), **kw))


@pytest.mark.parametrize("iters", [0, 1, 2, 5])
def test_one_prepare_and_exactly_iter_max_step_launches(monkeypatch, iters):
    x, p, _ = on_gpu(crf_cases.SHAPES[1], "cut", "nchw")
    names, real = [], nnf._launch
    monkeypatch.setattr(nnf, "_launch", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    nnf.dense_crf(x, p, iter_max=iters, **crf_cases.SETTINGS["cut"])
    assert names == ["vqseg_crf_prepare_f"] + ["vqseg_crf_step_f"] * iters


def test_densecrf_on_device_tensors_takes_the_kernels(monkeypatch):
    from vq_seg_amd.utils.crf import DenseCRF
    x, p, ref = on_gpu(crf_cases.SHAPES[0], "cut", "nchw")
    names, real = [], nnf._launch
    monkeypatch.setattr(nnf, "_launch", lambda name, *a, **k: (names.append(name), real(name, *a, **k))[1])
    crf = DenseCRF(iter_max=2, **crf_cases.SETTINGS["cut"])
    q = crf(x[1], p[1])
    assert torch.is_tensor(q) and q.is_cuda and tuple(q.shape) == tuple(p[1].shape)
    assert names == ["vqseg_crf_prepare_f", "vqseg_crf_step_f", "vqseg_crf_step_f"]
    assert float(np.abs(q.double().cpu().numpy() - ref[2][1]).max()) <= 4.0 * f32_error(crf_cases.SHAPES[0], "cut")[2] + ULP
    assert torch.equal(crf.batch(x, p)[1], q)                    # an image's result does not depend on its batch
