"""Dense-CRF refinement off the GPU: utils.crf.DenseCRF's torch-op form against the float64 restatement of tests/crf_cases.py, the
properties of the contract, argument checks, the compat import, and the library's host-side refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import crf_cases
from vq_seg_amd import _hip, nnf
from vq_seg_amd.utils.crf import DenseCRF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUT = crf_cases.SETTINGS["cut"]


def small(seed=5, c=3, h=17, w=23):
    images, probs = crf_cases.make_inputs(seed, 1, c, h, w)
    return images[0], probs[0]


@pytest.mark.parametrize("setting", sorted(crf_cases.SETTINGS))
@pytest.mark.parametrize("shape", crf_cases.SHAPES[:3], ids=str)
def test_densecrf_cpu_equals_the_restatement(shape, setting):
    """the reference's call, image (3, H, W) and prob_map (C, H, W), on CPU tensors and on numpy: a float32 numpy (C, H, W)"""
    images, probs, ref = crf_cases.case(shape, setting)
    for iters in crf_cases.ITERS:
        crf = DenseCRF(iters, 7, 50, 4, 3, 3) if setting == "defaults" else DenseCRF(iter_max=iters, **crf_cases.SETTINGS[setting])
        got_t = crf(torch.from_numpy(images[0].copy()), torch.from_numpy(probs[0].copy()))
        got_n = crf(images[0].copy(), probs[0].copy())
        for got in (got_t, got_n):
            assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == probs[0].shape
            assert np.abs(got - ref[iters][0]).max() <= 1e-6
        assert np.array_equal(got_t, got_n)


def test_constructor_takes_the_references_argument_order():
    crf = DenseCRF(5, 1.0, 20, 3, 2.0, 1.5)
    assert (crf.iter_max, crf.bi_w, crf.bi_xy_std, crf.bi_rgb_std, crf.pos_w, crf.pos_xy_std, crf.truncate) == (5, 1.0, 20, 3, 2.0, 1.5, 4.0)
    d = DenseCRF()
    assert (d.iter_max, d.bi_w, d.bi_xy_std, d.bi_rgb_std, d.pos_w, d.pos_xy_std, d.truncate) == (10, 7, 50, 4, 3, 3, 4.0)


def test_no_iterations_and_no_weights_give_the_clipped_renormalised_input():
    image, prob = small()
    prob = prob.copy()
    prob[:, 0, 0] = (0.0, 1.0, 0.0)                              # clipped to 1e-5, then renormalised
    clipped = np.clip(prob.astype(np.float64), 1e-5, 1.0)
    want = clipped / clipped.sum(axis=0, keepdims=True)
    assert np.abs(DenseCRF(iter_max=0)(image, prob) - want).max() <= 1e-6
    for iters in (1, 4):
        assert np.abs(DenseCRF(iter_max=iters, bi_w=0, pos_w=0)(image, prob) - want).max() <= 1e-6


def test_rows_sum_to_one_and_a_flip_of_the_inputs_flips_q():
    image, prob = small(seed=6, c=4)
    crf = DenseCRF(iter_max=3, **CUT)
    q = crf(image, prob)
    assert np.abs(q.sum(axis=0) - 1.0).max() <= 1e-6
    assert (q.argmax(axis=0) != prob.argmax(axis=0)).mean() > 0.03          # it does something
    for axes in ((2,), (1,), (1, 2)):
        flipped = crf(np.flip(image, axes).copy(), np.flip(prob, axes).copy())
        assert np.abs(np.flip(flipped, axes) - q).max() <= 1e-6


def test_truncate_none_is_a_truncate_that_covers_the_image():
    image, prob = small(seed=7)
    kw = dict(iter_max=2, bi_xy_std=4.0, pos_xy_std=1.5)
    full = DenseCRF(truncate=None, **kw)(image, prob)
    wide = DenseCRF(truncate=40.0, **kw)(image, prob)            # R = 60 and 160 on a 17 x 23 image
    cut = DenseCRF(truncate=2.0, **kw)(image, prob)
    assert np.array_equal(full, wide)
    assert np.abs(full - cut).max() > 1e-4


def test_batch_on_cpu_tensors_and_logits():
    images, probs, ref = crf_cases.case(crf_cases.SHAPES[1], "cut")
    crf = DenseCRF(iter_max=2, **CUT)
    x, p = torch.from_numpy(images.copy()), torch.from_numpy(probs.copy())
    q = crf.batch(x, p)
    e = crf.batch(x, p, out="logits")
    assert q.dtype == torch.float32 and tuple(q.shape) == probs.shape
    assert np.abs(q.numpy() - ref[2]).max() <= 1e-6
    assert (torch.softmax(e.double(), dim=1) - q.double()).abs().max() <= 1e-6
    with pytest.raises(ValueError, match="out is"):
        crf.batch(x, p, out="labels")


def test_argument_validation():
    for kw in (dict(iter_max=-1), dict(iter_max=1.5), dict(bi_xy_std=0), dict(bi_rgb_std=-1.0), dict(pos_xy_std=0.0), dict(truncate=-1.0),
               dict(truncate=float("nan")), dict(bi_w=float("inf")), dict(pos_w=float("nan"))):
        with pytest.raises(ValueError, match="DenseCRF"):
            DenseCRF(**kw)
    image, prob = small()
    with pytest.raises(ValueError, match="one size"):
        DenseCRF()(image[:, :-1], prob)
    with pytest.raises(ValueError, match="one size"):
        DenseCRF()(image[:2], prob)
    with pytest.raises(ValueError, match="at least 2 classes"):
        DenseCRF()(image, prob[:1])
    with pytest.raises(ValueError, match="out is"):
        nnf.dense_crf(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), out="labels")
    with pytest.raises(ValueError, match="iter_max"):
        nnf.dense_crf(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), iter_max=-2)
    E = _hip.HipLibraryError
    with pytest.raises(E, match="2..4 classes"):
        nnf.dense_crf(torch.zeros(1, 3, 4, 4), torch.zeros(1, 5, 4, 4))
    with pytest.raises(E, match="batch and size"):
        nnf.dense_crf(torch.zeros(1, 3, 4, 5), torch.zeros(1, 3, 4, 4))
    with pytest.raises(E, match="expected a float32"):
        nnf.dense_crf(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4, dtype=torch.float64))
    assert not nnf.dense_crf_supported(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4))       # not on the GPU


def test_nnf_dense_crf_has_no_cpu_fallback():
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        nnf.dense_crf(torch.rand(2, 3, 8, 8), torch.softmax(torch.rand(2, 3, 8, 8), dim=1))
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        nnf.dense_crf(torch.rand(1, 3, 8, 8), torch.softmax(torch.rand(1, 2, 8, 8), dim=1), iter_max=0, out="logits")


def test_predictor_and_test_loop_refuse_what_is_not_built():
    from vq_seg_amd.evaluate import test_loop
    from vq_seg_amd.predict import Predictor
    model = torch.nn.Conv2d(3, 3, 1)
    with pytest.raises(ValueError, match="not built"):
        Predictor(model, 3, window=8, crf=True)
    with pytest.raises(TypeError, match="DenseCRF"):
        Predictor(model, 3, crf="yes")
    assert Predictor(model, 3).crf is None and isinstance(Predictor(model, 3, crf=True).crf, DenseCRF)
    with pytest.raises(ValueError, match="crf needs fused=True"):
        test_loop(model, [], 3, crf=True)
    with pytest.raises(ValueError, match="not built"):
        test_loop(model, [], 3, fused=True, crf=True, window=8)


def test_reference_import_of_densecrf_binds_in_a_fresh_interpreter(tmp_path):
    """`from utils.crf import DenseCRF` of deprecated/test _crf.py with <repo>/compat in front of sys.path, from a foreign directory"""
    script = tmp_path / "crf_head.py"
    script.write_text("import sys\nsys.path.insert(0, sys.argv[1])\nimport torch\nfrom utils.crf import DenseCRF\nimport vq_seg_amd.utils.crf as mine\n"
                      "crf = DenseCRF(iter_max=1)\nq = crf(torch.rand(3, 6, 7), torch.softmax(torch.rand(2, 6, 7), dim=0))\n"
                      "print(DenseCRF is mine.DenseCRF, type(q).__name__, q.dtype, q.shape)\n")
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    res = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "compat")], cwd=str(tmp_path), env=env, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stdout.strip().splitlines()[-1] == "True ndarray float32 (2, 6, 7)"


def test_the_library_refuses_bad_arguments_without_a_device():
    L = _hip.lib()
    one = torch.zeros(64)
    p = one.data_ptr()                                           # any non-null address: every refusal comes before it is touched

    def prepare(image=p, prob=p, b=1, c=3, h=4, w=4, iter_max=1, stds=(50.0, 4.0, 3.0), truncate=4.0, bufs=(p,) * 6):
        return L.vqseg_crf_prepare_f(image, 3 * h * w, h * w, 1, prob, c * h * w, h * w, 1, b, c, h, w, iter_max, *stds, truncate, *bufs, None)

    def step(ptrs=(p, p, p, p, p, p + 4), b=1, c=3, h=4, w=4, bi_w=7.0, stds=(50.0, 4.0), pos_w=3.0, pos_xy_std=3.0, truncate=4.0):
        return L.vqseg_crf_step_f(*ptrs, b, c, h, w, bi_w, *stds, pos_w, pos_xy_std, truncate, 0, None)

    def refused(rc, text):
        assert rc == -1 and text in L.vqseg_last_error(), (rc, L.vqseg_last_error())

    refused(prepare(image=None), b"null")
    refused(prepare(bufs=(p, p, None, p, p, p)), b"null")
    refused(prepare(bufs=(p, p, p, None, p, p)), b"null norm_pos")
    refused(prepare(iter_max=-1), b"iter_max")
    for c in (1, 5):
        refused(prepare(c=c), b"2..4 classes")
        refused(step(c=c), b"2..4 classes")
    refused(prepare(h=0), b"positive")
    refused(prepare(w=4096), b"2048")
    for stds in ((0.0, 4.0, 3.0), (50.0, -1.0, 3.0), (50.0, 4.0, 0.0), (float("nan"), 4.0, 3.0)):
        refused(prepare(stds=stds), b"must be positive")
    refused(step(stds=(0.0, 4.0)), b"must be positive")
    refused(step(pos_xy_std=-3.0), b"must be positive")
    for t in (-1.0, float("nan")):
        refused(prepare(truncate=t), b"truncate")
        refused(step(truncate=t), b"truncate")
    refused(step(ptrs=(p, p, p, p, None, p)), b"null")
    refused(step(ptrs=(p, p, p, p, p, p)), b"ping-pong")
    refused(step(bi_w=float("inf")), b"finite")
    refused(L.vqseg_crf_prepare_f(p, 48, 16, 2, p, 48, 16, 1, 1, 3, 4, 4, 1, 50.0, 4.0, 3.0, 4.0, p, p, p, p, p, p, None), b"layout")
