"""The supervised contrastive loss without a GPU: the torch-op form of the stabilised arithmetic against what the reference module
computed (tests/golden/supcon_ref.npz) and, where the reference overflows, against a float64 restatement; the package surface."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import supcon_cases as sc
from tests.test_abi_cpu import header_symbols
from vq_seg_amd import _hip, loss, nnf
from vq_seg_amd.loss import SupConLoss
from vq_seg_amd.loss.contrastive_loss import supcon_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "supcon_ref.npz"))
# |loss * HW^2 - golden * HW^2|, absolute.  The reference's own float32 value (a plain exp, a float32 sum over HW^2 terms, a float32 log)
# was measured 9e-7 .. 2.7e-6 away from a float64 log-sum-exp on inputs of this kind; the two float32 forms must agree to 2e-6.
VALUE_BAR = 2e-6
GRAD_BAR = 1e-5           # relative L2 of the gradient against the reference's autograd.grad


@pytest.mark.parametrize("k", range(len(sc.GOLDEN_CASES)))
def test_torch_form_matches_the_reference(k):
    x, target = sc.golden_inputs(k)
    hw2 = float(x.shape[2] * x.shape[3]) ** 2
    xg = x.clone().requires_grad_(True)
    y = SupConLoss(sc.TEMPERATURE)(xg, target)              # CPU tensors: the torch-op form
    (g,) = torch.autograd.grad(y, xg)
    ref, ref_g = float(GOLDEN[f"loss_{k}"]), torch.from_numpy(GOLDEN[f"grad_{k}"])
    err = abs(float(y.detach()) * hw2 - ref * hw2)
    rel = float((g - ref_g).norm() / ref_g.norm())
    print(f"case {k}: |d loss| * HW^2 = {err:.3e}, gradient rel L2 = {rel:.3e}")
    assert err <= VALUE_BAR
    assert rel <= GRAD_BAR
    assert float(g[2:].abs().max()) == 0.0                  # only images 0 and 1 enter


@pytest.mark.parametrize("kind", ["three", "block255"])
def test_finite_where_the_reference_overflows(kind):
    """scale 3: max z is in the thousands, exp(z) is inf in float32 and the reference returns NaN; the stabilised form stays finite and
    equal to float64.  Bar: the float32 z of either side carries C 2^-24 |x||y| / T from the dot product and a few 2^-24 |z| from the
    division and the log-sum-exp's subtraction; logA and logP each move by at most the largest z error (log-sum-exp is 1-Lipschitz in
    the sup norm), so |d (logA - logP)| <= 2 (C 2^-24 |x||y| / T + 4 * 2^-24 zmax)."""
    b, c, h, w = 3, 32, 16, 16
    x, target = sc.features(950, (b, c, h, w), 3.0), sc.targets(951, b, h, w, kind)
    ref = sc.restate64(x, target)
    assert ref["zmax"] > 1000.0
    xg = x.clone().requires_grad_(True)
    y = supcon_torch(xg, target, sc.TEMPERATURE)
    (g,) = torch.autograd.grad(y, xg)
    t = float(np.float32(sc.TEMPERATURE))
    bar = 2 * (c * 2.0 ** -24 * ref["norm"] / t + 4 * 2.0 ** -24 * ref["zmax"])
    err = abs(float(y.detach().double()) * (h * w) ** 2 - ref["diff"])
    print(f"{kind}: zmax {ref['zmax']:.0f}, |d (logA - logP)| = {err:.3e} (bar {bar:.3e})")
    assert np.isfinite(float(y.detach())) and bool(torch.isfinite(g).all())
    assert err <= bar
    for k_, key in ((0, "g1"), (1, "g2")):
        rel = float((sc.rows_of(g, k_) - ref[key]).norm() / ref[key].norm())
        # exp(z - logA) with z and logA in float32 below 8192: four roundings of 2^-24 * 8192 in the exponent -> 2e-3 relative per pair
        assert rel <= 2e-3, rel


def test_no_positive_pair_is_inf_with_a_finite_gradient():
    b, c, h, w = 3, 16, 6, 5
    x, target = sc.features(952, (b, c, h, w), 0.3), sc.targets(953, b, h, w, "disjoint")
    ref = sc.restate64(x, target)
    xg = x.clone().requires_grad_(True)
    y = supcon_torch(xg, target, sc.TEMPERATURE)
    (g,) = torch.autograd.grad(y, xg)
    assert float(y) == float("inf") and ref["diff"] == float("inf")
    assert float((sc.rows_of(g, 0) - ref["g1_all"]).norm() / ref["g1_all"].norm()) <= 1e-5      # the positive term is absent (deliberate: the reference gives NaN)
    assert float((sc.rows_of(g, 1) - ref["g2_all"]).norm() / ref["g2_all"].norm()) <= 1e-5


def test_chunks_without_a_positive_pair_and_autocast(monkeypatch):
    """row chunks of 8: image 0's first rows carry a class image 1 does not have, so whole chunks have no positive pair -- they add nothing
    and leave no NaN in the gradient; inside an autocast region the product stays float32 (the same bits as outside it)"""
    from vq_seg_amd.loss import contrastive_loss
    monkeypatch.setattr(contrastive_loss, "_CHUNK_ROWS", 8)
    b, c, h, w = 3, 16, 6, 8
    x, target = sc.features(954, (b, c, h, w), 0.3), sc.targets(955, b, h, w, "three")
    target[0, :2] = 7                                       # 16 rows = two chunks of image 0 without a partner in image 1
    ref = sc.restate64(x, target)
    xg = x.clone().requires_grad_(True)
    y = supcon_torch(xg, target, sc.TEMPERATURE)
    (g,) = torch.autograd.grad(y, xg)
    assert abs(float(y.detach()) * (h * w) ** 2 - ref["diff"]) <= 1e-5 and bool(torch.isfinite(g).all())
    assert float((sc.rows_of(g, 0) - ref["g1"]).norm() / ref["g1"].norm()) <= 1e-5
    with torch.autocast("cpu", dtype=torch.bfloat16):
        y_amp = supcon_torch(x, target, sc.TEMPERATURE)
    assert y_amp.dtype == torch.float32 and float(y_amp) == float(y.detach())


def test_nearest_targets_and_four_dim_labels():
    x, target = sc.golden_inputs(1)                          # targets at twice the feature size
    a = supcon_torch(x, target, sc.TEMPERATURE)
    assert float(a) == float(supcon_torch(x, target.unsqueeze(1), sc.TEMPERATURE))
    assert abs(float(a) * 35.0 ** 2 - sc.restate64(x, target)["diff"]) <= VALUE_BAR


def test_batch_of_two_is_refused():
    x, target = sc.golden_inputs(0)
    with pytest.raises(AssertionError, match="batch size is larger than 2"):
        SupConLoss()(x[:2], target[:2])
    assert SupConLoss().temperature == 0.04


def test_symbols_are_declared():
    names = {"vqseg_supcon_workspace_bytes", "vqseg_supcon_forward_f", "vqseg_supcon_backward_f"}
    assert names <= set(header_symbols()) and names <= set(_hip.SYMBOLS)
    L = _hip.lib()
    assert L.vqseg_supcon_workspace_bytes(0) == 0
    assert L.vqseg_supcon_workspace_bytes(35) == 4 * 35 * 4                                   # one column split
    assert L.vqseg_supcon_workspace_bytes(96 * 96) < (2 << 20)                                # O(HW): the dense matrix would be 340 MB
    # bad shapes and null pointers are refused before anything touches a device
    assert L.vqseg_supcon_forward_f(0, None, None, 24, 4, 4, 24, None, None, 4, 4, 0.04, None, 0, None, None) == -1
    assert b"multiple of 16" in L.vqseg_last_error()
    assert L.vqseg_supcon_forward_f(0, None, None, 32, 4, 4, 32, None, None, 4, 4, 0.04, None, 0, None, None) == -1
    assert b"null" in L.vqseg_last_error()
    assert L.vqseg_supcon_backward_f(1, None, None, 32, 4, 4, 32, None, None, 4, 4, 0.0, None, None, None, None, 32, None) == -1
    assert b"temperature" in L.vqseg_last_error()


def test_wrapper_refuses_wrong_inputs_before_a_device():
    x, target = sc.golden_inputs(0)
    assert not nnf.supcon_supported(x, target)               # CPU tensors take SupConLoss's torch-op form
    with pytest.raises(_hip.HipLibraryError, match="float32 .* or bfloat16"):
        nnf.supcon(x.double(), target)
    with pytest.raises(_hip.HipLibraryError, match="multiple of 16"):
        nnf.supcon(x[:, :24], target)
    with pytest.raises(_hip.HipLibraryError, match="integer class labels"):
        nnf.supcon(x, target.float())
    with pytest.raises(_hip.HipLibraryError, match="one target per image"):
        nnf.supcon(x, target[:2])
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        nnf.supcon(x, target)


def test_factory_keys_are_the_references():
    assert sorted(loss.loss_func_dict) == sorted(loss.loss_dict) == ["cross_entropy", "dice_loss", "focal_loss", "nll_loss"]
    assert loss.SupConLoss is SupConLoss


def test_compat_binds_the_reference_names(tmp_path):
    script = ("import sys; sys.path.insert(0, sys.argv[1])\n"
              "from loss import SupConLoss\n"
              "from loss.contrastive_loss import SupConLoss as S2\n"
              "import vq_seg_amd.loss as real\n"
              "assert SupConLoss is real.SupConLoss is S2\n"
              "print('bound')\n")
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    res = subprocess.run([sys.executable, "-c", script, os.path.join(ROOT, "compat")], cwd=str(tmp_path), env=env, capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0 and res.stdout.strip().endswith("bound"), res.stderr[-2000:]
