"""The float64 pieces that tests/test_loss_kernels_gpu.py writes out (per-image Dice sums, per-row prototype terms, the closed-form
feature gradient, the CPS combination) reassemble to oracle/torch_ref.py's scalars on the golden inputs (cases.proto_inputs(),
cases.loss_inputs()).  tests/test_oracle_golden.py pins torch_ref to tests/golden/prototype.npz and losses_metrics.npz, so the GPU
suite's references hang on what the reference recorded.  Also here, because it needs no GPU: the seeds of the prototype cases leave
at most 1 % of a case's rows near a branch point of phi_of."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import torch_ref as R
from tests import cases, golden_io
from tests import test_loss_kernels_gpu as K

TIGHT = 1e-12                                                   # float64 against float64, the sums in another order


def close(a, b, tol=TIGHT):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), (a, b)


@pytest.mark.parametrize("ignored", [False, True])
def test_dice_pieces_reassemble_to_torch_ref(ignored):
    pred, pred2, tgt = cases.loss_inputs()
    if ignored:
        tgt = tgt.clone()
        tgt[:, ::5, ::3] = 255
        tgt[1] = 255
    for p in (pred, pred2):
        pd = p.double()
        inter, sets, ce = K.dice_pieces(pd.reshape(3, 3, -1), tgt.reshape(3, -1), 255)
        close(K.dice_from_pieces(inter, sets), R.dice_loss(pd, tgt))
        close(ce[:, 0].sum(), F.cross_entropy(pd, tgt, ignore_index=255, reduction="sum"))
        assert ce[:, 1].sum().item() == float((tgt != 255).sum())
        # the gradient the GPU suite uses (autograd through the pieces) is the gradient of torch_ref's loss
        x = pd.clone().requires_grad_(True)
        (g_ref,) = torch.autograd.grad(R.dice_loss(x, tgt) + 0.5 * F.cross_entropy(x, tgt, ignore_index=255, reduction="sum"), x)
        i0, s0 = inter.clone().requires_grad_(True), sets.clone().requires_grad_(True)
        gi, gs = torch.autograd.grad(K.dice_from_pieces(i0, s0), (i0, s0))
        g = K.dice_grad_ref(pd.reshape(3, 3, -1), tgt.reshape(3, -1), 255, gi, gs, torch.full((3,), 0.5, dtype=torch.float64))
        close(g.reshape(p.shape), g_ref)
    if not ignored:                                             # and torch_ref's sum is the golden file's
        fx = golden_io.load("losses_metrics")
        inter, sets, ce = K.dice_pieces(pred.double().reshape(3, 3, -1), tgt.reshape(3, -1), 255)
        sup = 0.5 * ce[:, 0].sum() / ce[:, 1].sum() + K.dice_from_pieces(inter, sets)
        assert abs(sup.item() - float(fx["sup_loss"])) <= 1e-6 * abs(float(fx["sup_loss"]))


def _proto_rows():
    feat, gt, scores, protos, entropy = cases.proto_inputs()
    fd = feat.double()
    labels = F.interpolate(gt[:, None].float(), feat.shape[-2:], mode="nearest").long().permute(0, 2, 3, 1).reshape(-1)
    return feat, fd, cases.rows_of(fd), gt, labels, scores, protos.double(), entropy


@pytest.mark.parametrize("margin,scale", [(0.0, 1.0), (0.5, 30.0), (0.3, 8.0)])
def test_proto_rows_reassemble_to_torch_ref(margin, scale):
    fx = golden_io.load("prototype")
    feat, fd, rows, gt, labels, scores, pd, entropy = _proto_rows()
    pn = F.normalize(pd, dim=-1)
    # variant 1: the keep mask as the reference derives it from the entropies
    percent = fx.meta["percent"]
    keep = (entropy <= float(np.percentile(entropy.numpy().flatten(), percent))).double()
    l1 = -torch.mean(K.proto_ll(rows, pn, labels, 1, margin, scale, True) * keep)
    close(l1, R.prototype_loss_v1(fd, gt, pd, percent, entropy, margin, scale))
    # variant 2, ground truth and pseudo scores (confidence mask)
    l2 = -torch.mean(K.proto_ll(rows, pn, labels, 2, margin, scale, True))
    close(l2, R.prototype_loss_v2(fd, gt, pd, fx.meta["th"], margin, scale)[0])
    sc = F.interpolate(scores.double(), feat.shape[-2:], mode="bilinear")
    prob = torch.softmax(sc.permute(0, 2, 3, 1).reshape(-1, 3), dim=-1)
    conf = (prob.max(dim=1)[0] > fx.meta["th"]).double()
    pseudo = torch.argmax(sc, dim=1).reshape(-1)
    l2s = -torch.mean(K.proto_ll(rows, pn, pseudo, 2, margin, scale, True) * conf)
    close(l2s, R.prototype_loss_v2(fd, scores.double(), pd, fx.meta["th"], margin, scale)[0])
    if (margin, scale) in ((0.0, 1.0), (0.5, 30.0)):            # and those are the golden file's numbers
        tag = "m0" if margin == 0 else "m05"
        assert abs(l1.item() - float(fx[f"v1_{tag}_loss"])) <= 1e-5 * abs(float(fx[f"v1_{tag}_loss"]))
        assert abs(l2.item() - float(fx[f"v2_{tag}_gt_loss"])) <= 1e-5 * abs(float(fx[f"v2_{tag}_gt_loss"]))


@pytest.mark.parametrize("easy", [True, False])
@pytest.mark.parametrize("variant", [1, 2])
@pytest.mark.parametrize("margin,scale", [(0.0, 1.0), (0.5, 30.0), (1.5, 1.0)])
def test_proto_closed_form_is_the_gradient_of_the_restatement(margin, scale, variant, easy):
    """the closed form whose terms make the GPU suite's bound is autograd's gradient of proto_ll, the non-easy margin included (its
    restatement is torch_ref._margin_terms); a zero row gets (sum_c gcos_c p_c) / 1e-12"""
    _, _, rows, _, labels, _, pd, entropy = _proto_rows()
    rows = rows[:300].clone()
    rows[0] = 0.0
    labels, w = labels[:300], entropy[:300].double()
    pn = F.normalize(pd, dim=-1)
    loss, gx, _ = K.proto_ref(rows, pn, labels, w, 3.0, variant, margin, scale, easy)
    gx_c, S, _, cos, Sd = K.proto_closed(rows, pn, labels, w, 3.0, variant, margin, scale, easy)
    assert float((gx - gx_c).abs().max()) <= 1e-10 * float(gx.abs().max())
    assert bool((gx_c.abs() <= S * (1 + 1e-12)).all()) and bool((S <= Sd * (1 + 1e-12)).all())      # the sums of absolute values bound the element
    assert bool(torch.isfinite(gx[0]).all()) and float(gx[0].abs().max()) > 1e6 * float(gx[1:].abs().max())
    assert bool((cos[0] == 0).all())


def test_combine_reassembles_to_the_training_step_scalars():
    """combine_ref with one supervised and two CPS terms is 0.5 CE + Dice per term, as tests/test_oracle_golden.py forms the golden's
    sup_loss and cps_loss from torch_ref.dice_loss"""
    fx = golden_io.load("losses_metrics")
    pred, pred2, tgt = cases.loss_inputs()
    fa = R.score_mask(pred, torch.argmax(pred, 1).long(), fx.meta["th"])
    fb = R.score_mask(pred2, torch.argmax(pred2, 1).long(), fx.meta["th"])
    pieces = lambda p, t: list(K.dice_pieces(p.double().reshape(3, 3, -1), t.reshape(3, -1), 255))
    terms = [pieces(pred, tgt), pieces(pred, fb), pieces(pred2, fa)]
    total, stats = K.combine_ref(terms, 1, 1.0, 0.5, 1e-6, [], 0.0, [], 0.0)
    assert abs(stats[4].item() - float(fx["sup_loss"])) <= 1e-6 * abs(float(fx["sup_loss"]))
    assert abs(stats[3].item() - float(fx["cps_loss"])) <= 1e-6 * abs(float(fx["cps_loss"]))
    close(total, stats[4] + stats[3])
    commits = [torch.tensor([0.1, 0.2], dtype=torch.float64), torch.tensor([0.3, 0.4], dtype=torch.float64)]
    protos = [torch.tensor(2.0, dtype=torch.float64)]
    total2, stats2 = K.combine_ref(terms, 1, 1.5, 0.5, 1e-6, commits, 0.25, protos, 0.01)
    close(stats2[1], 0.25)
    close(stats2[2], 0.02)
    close(total2, stats[4] + 1.5 * stats[3] + 0.25 + 0.02)


@pytest.mark.parametrize("i", range(len(K.PROTO_CASES)), ids=K.PROTO_IDS)
def test_proto_case_seeds_leave_at_most_one_percent_near_a_branch_point(i):
    out = K.proto_switch_cap(i)                                 # asserts the cap
    variant, k, c, m = K.PROTO_CASES[i][:4]
    x, proto, labels, w = K.proto_inputs(i)
    assert x.shape == (m, c) and proto.shape == (k, c) and int(labels.max()) < k and out.shape == (m,)
    if m >= 255:                                                # the four special rows are what the docstring says
        cos = F.normalize(x.double(), dim=1) @ proto.double().t()
        assert bool((x[0] == 0).all()) and abs(float(x[3].norm()) - 1e-3) < 1e-8
        assert abs(cos[1, labels[1]].item() - (1 - 1e-3)) < 2e-5 and abs(cos[2, labels[2]].item() + (1 - 1e-3)) < 2e-5
        assert abs(float(x[1].norm()) - 3.0) < 0.01 and abs(float(x[2].norm()) - 2.0) < 0.01
