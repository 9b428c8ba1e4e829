"""The averaged ("teacher") networks above the kernel: optim.HipAdam.attach_average on a small net, and CPSConfig.ema_decay /
teacher_pseudo_labels in the CPS step (recipe v1, 64 x 64, batch 2 + 2, 64 codes, bf16: the model of tests/test_balanced_trainer_gpu.py).

Every comparison is a bit-equality: between the teacher and the float32 emulation chained on the host from the recorded student
values (tests/ema_cases.py::ema_emulate), between two runs of the same float32 code, or between the teacher's forward through the
images its launch wrote and a freshly built module's through lazily packed ones."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch
from torch import nn

from tests import ema_cases as E
from tests import optim_cases as C

pytestmark = pytest.mark.gpu

DECAY = 0.99


def dev():
    return torch.device("cuda:0")


def _np(t):
    return t.detach().float().cpu().numpy().copy()


# ------------------------------------------------------------------------------------------------ HipAdam with an average, small net
class _SmallNet(nn.Module):
    """conv 3 x 3 24 -> 40, conv 1 x 1 40 -> 33, their BatchNorms and a flat parameter.  The weight-gradient kernels take channel
    counts that are multiples of 8, so the 33-channel layer TRAINS through ATen and only eval forwards (the teacher's) run it on the HIP
    kernels: its student record has no images and the teacher's record has, the 3 x 3 layer's records both have."""

    def __init__(self):
        super().__init__()
        self.c3, self.b3 = nn.Conv2d(24, 40, 3, padding=1, bias=False), nn.BatchNorm2d(40)
        self.c1, self.b1 = nn.Conv2d(40, 33, 1, bias=False), nn.BatchNorm2d(33)
        self.scale = nn.Parameter(torch.linspace(0.5, 1.5, 33))

    def forward(self, x):
        from vq_seg_amd import nnf
        y = nnf.conv_bn_act(x, self.c3, self.b3)
        y = self.b1(self.c1(y.float())) if self.training else nnf.conv_bn_act(y, self.c1, self.b1, relu=False)
        return y.float() * self.scale.view(1, -1, 1, 1)


def _fresh_small(state):
    m = _SmallNet().to(dev())
    m.load_state_dict(state)
    return m.eval()


def test_hip_adam_keeps_the_average_and_the_teachers_images_in_its_launch():
    from vq_seg_amd.averaging import AveragedNetwork
    from vq_seg_amd.optim import HipAdam
    torch.manual_seed(3)
    net = _SmallNet().to(dev())
    opt = HipAdam(net.parameters(), lr=0.02)
    avg = AveragedNetwork(net, _SmallNet, DECAY)
    opt.attach_average(avg)
    assert not avg.module.training and not any(p.requires_grad for p in avg.module.parameters())
    xs = [torch.rand(2, 24, 16, 16, device=dev()).contiguous(memory_format=torch.channels_last).to(torch.bfloat16) for _ in range(3)]
    chain = None
    for step, x in enumerate(xs, start=1):
        with torch.no_grad():
            avg.module(xs[0])                                            # the teacher runs forwards: its image kinds are learnt like any weight's
        net(x).square().mean().backward()
        opt.step()
        opt.zero_grad(set_to_none=False)
        torch.cuda.synchronize()
        assert avg.updates == step
        student, teacher = net.state_dict(), avg.state_dict()["module"]
        assert list(student) == list(teacher)
        if step == 1:
            for name in student:
                assert torch.equal(student[name], teacher[name]), f"after the first update {name} is not the student's"
            chain = {name: _np(t) for name, t in student.items() if t.is_floating_point()}
        else:
            for name, e_old in chain.items():
                chain[name] = E.check_ema(_np(teacher[name]), e_old, _np(student[name]), DECAY, False, f"step {step} {name}")
            assert torch.equal(student["b3.num_batches_tracked"], teacher["b3.num_batches_tracked"])
            assert not torch.equal(student["c3.weight"], teacher["c3.weight"])
        if step >= 2:                                                     # the launch wrote the teacher's forward images and installed them
            for conv in (avg.module.c3, avg.module.c1):
                pack = conv.weight._vq_pack
                assert pack is not None and "fwd" in pack["all"] and pack["all"]["fwd"] is conv.weight._vq_img_bufs["fwd"]
            assert getattr(net.c3.weight, "_vq_kinds", None) and not getattr(net.c1.weight, "_vq_kinds", None)
        with torch.no_grad():
            got, want = avg.module(xs[0]), _fresh_small(teacher)(xs[0])
        assert torch.equal(got, want), f"step {step}: the teacher's forward differs from a freshly built module with its state"
    # nothing of the average in the optimiser's state
    assert set(opt.state_dict()) == {"state", "param_groups"}
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in opt.state_dict()["state"].values())


# ------------------------------------------------------------------------------------------------ the CPS trainer
SUBSET = ("encoder.conv1.weight", "decoder.blocks.4.0.0.weight", "encoder.layer1.0.conv1.weight", "decoder.blocks.4.0.1.weight",
          "decoder.blocks.4.0.1.running_mean", "codebook.4.codebook.embedding.weight", "segmentation_head.weight")
COPIED = ("codebook.4.codebook.embedding.weight",)


def _model():
    return {"name": "vqreptunet1x1", "params": {"encoder_name": "resnet50", "num_classes": 3, "depth": 5,
                                                "vq_cfg": {"num_embeddings": [0, 0, 64, 64, 64], "distance": "euclidean", "kmeans_init": True},
                                                "margin": 0.0, "scale": 1.0, "use_feature": False, "encoder_weights": None}}


def _trainer(**kw):
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer
    return CPSTrainer(CPSConfig(model=_model(), recipe="v1", total_iters=8, amp_dtype=torch.bfloat16, keep_aux=True, **kw), dev())


@functools.lru_cache(maxsize=None)
def _batches():
    from vq_seg_amd.trainer import SyntheticCropWeed
    lab, ul = SyntheticCropWeed(64, 2, dev(), seed=5), SyntheticCropWeed(64, 2, dev(), seed=6)
    return [(lab.labelled(), ul.unlabelled()) for _ in range(3)]


@functools.lru_cache(maxsize=None)
def _tmpdir():
    return tempfile.mkdtemp(prefix="ema_teacher_")


def _states(modules):
    torch.cuda.synchronize()
    return [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in modules]


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def _pair_scores(tr, modules, ul):
    """the no-grad eval forwards that open the step, for `modules`, as the step runs them"""
    with torch.no_grad():
        for m in tr.models:
            m.eval()
        o1, o2 = tr._fwd_pair((ul,), (ul,), use_amp=tr.cfg.eval_amp, models=modules)
        tr._join()
        for m in tr.models:
            m.train()
    torch.cuda.synchronize()
    return o1[0].float().clone(), o2[0].float().clone()


@functools.lru_cache(maxsize=None)
def _run(kind):
    """three steps of one trainer; everything the tests below compare, recorded once"""
    kw = {"plain": {}, "observe": dict(ema_decay=DECAY), "pseudo": dict(ema_decay=DECAY, teacher_pseudo_labels=True)}[kind]
    tr = _trainer(**kw)
    rec = dict(tr=tr, outs=[], aux=[], subset=[], after_first=None, forwards=None)
    for i, ((l_in, l_tg), ul) in enumerate(_batches()):
        if i == 2 and kind == "pseudo":
            tr.save_checkpoint(os.path.join(_tmpdir(), "pseudo_2.pt"))
            ul_cl = ul.contiguous(memory_format=torch.channels_last)
            rec["forwards"] = dict(teacher=_pair_scores(tr, tr.teachers, ul_cl), student=_pair_scores(tr, tr.models, ul_cl))
        out = tr.step(l_in, l_tg, ul)
        torch.cuda.synchronize()
        rec["outs"].append({k: v.detach().clone() for k, v in out.items()})
        rec["aux"].append({k: v.detach().clone() for k, v in tr.aux.items() if torch.is_tensor(v)})
        if tr.teachers:
            rec["subset"].append([{n: _np(m.state_dict()[n]) for n in SUBSET} for m in tr.models])
            if i == 0:
                rec["after_first"] = (_states(tr.models), [{k: v.detach().clone() for k, v in a.state_dict()["module"].items()} for a in tr.averages],
                                      [a.updates for a in tr.averages])
    rec["students"] = _states(tr.models)
    if kind == "plain":
        tr.save_checkpoint(os.path.join(_tmpdir(), "plain_3.pt"))
    return rec


def test_observation_only_leaves_the_step_bit_identical():
    """ema_decay set, teacher_pseudo_labels off: outputs and student state of three steps are those of a trainer built without the field"""
    plain, obs = _run("plain"), _run("observe")
    assert not plain["tr"].teachers and not plain["tr"].averages and len(obs["tr"].teachers) == 2
    for x, y in zip(plain["outs"], obs["outs"]):
        assert all(torch.equal(x[k], y[k]) for k in x)
    for a, b in zip(plain["students"], obs["students"]):
        assert _same(a, b)


def test_teacher_contents_follow_the_host_chain():
    obs = _run("observe")
    tr = obs["tr"]
    students, teachers, updates = obs["after_first"]
    assert updates == [1, 1] and [a.updates for a in tr.averages] == [3, 3]
    for s, t in zip(students, teachers):
        assert _same(s, t), "after step 1 the teacher is not the student"
    for k, (avg, model) in enumerate(zip(tr.averages, tr.models)):
        teacher, student = avg.state_dict()["module"], model.state_dict()
        assert not avg.module.training
        differ = [n for n in teacher if teacher[n].is_floating_point() and not torch.equal(teacher[n], student[n])]
        assert len(differ) > 0.8 * sum(t.is_floating_point() for t in teacher.values()), "after step 3 the teachers must differ from the students"
        for n in SUBSET:
            p1, p2, p3 = (obs["subset"][i][k][n] for i in range(3))
            if n in COPIED:
                C.check_bits(_np(teacher[n]), p3, f"network {k + 1} {n}: a copy record")
                continue
            e2 = E.ema_emulate(p1, p2, DECAY, False)
            E.check_ema(_np(teacher[n]), e2, p3, DECAY, False, f"network {k + 1} {n}")
            assert not np.array_equal(_np(teacher[n]), p3), n


def test_teacher_pseudo_labels_are_the_teachers_scores():
    plain, ps = _run("plain"), _run("pseudo")
    for i in (0, 1):                                                      # the teacher has the student's bits: the plain trainer's steps
        assert all(torch.equal(plain["outs"][i][k], ps["outs"][i][k]) for k in plain["outs"][i]), i
        assert all(torch.equal(plain["aux"][i][k], ps["aux"][i][k]) for k in plain["aux"][i]), i
    for k in (0, 1):
        used = ps["aux"][2][f"score_{k + 1}"]
        assert torch.equal(used, ps["forwards"]["teacher"][k]), f"step 2 score_{k + 1} is not the teacher's forward"
        assert not torch.equal(used, ps["forwards"]["student"][k]), f"step 2 score_{k + 1} is the student's forward"
    assert not all(torch.equal(plain["outs"][2][k], ps["outs"][2][k]) for k in ("loss", "cps_loss"))


def test_checkpoints_round_trip_the_teachers():
    ps, plain = _run("pseudo"), _run("plain")
    a = ps["tr"]
    b = _trainer(ema_decay=DECAY, teacher_pseudo_labels=True)
    b.load_checkpoint(os.path.join(_tmpdir(), "pseudo_2.pt"))
    assert [x.updates for x in b.averages] == [2, 2] and b.iter == 2
    (l_in, l_tg), ul = _batches()[2]
    out = b.step(l_in, l_tg, ul)
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], ps["outs"][2][k]) for k in out)
    for x, y in zip(_states(a.models), _states(b.models)):
        assert _same(x, y), "students differ after the resumed step"
    for x, y in zip(a.averages, b.averages):
        assert _same(x.state_dict()["module"], y.state_dict()["module"]) and x.updates == y.updates == 3, "teachers differ after the resumed step"
    # a file written with the feature off: teachers = the loaded students, updates = 0
    b.load_checkpoint(os.path.join(_tmpdir(), "plain_3.pt"))
    assert [x.updates for x in b.averages] == [0, 0]
    for m, avg, want in zip(b.models, b.averages, plain["students"]):
        assert _same(m.state_dict(), want) and _same(avg.state_dict()["module"], m.state_dict())
        assert all(getattr(tm, "initted") == getattr(sm, "initted") for (_, tm), (_, sm) in zip(avg.module.named_modules(), m.named_modules()) if hasattr(sm, "initted"))


def test_evaluate_scores_the_teacher():
    from vq_seg_amd.evaluate import test_loop
    from vq_seg_amd.models.networks import make_model
    from vq_seg_amd.trainer import SyntheticCropWeed
    tr = _run("observe")["tr"]
    data = SyntheticCropWeed(64, 2, dev(), seed=7, cell=8)                # 64 cells per image: every class in every image, so that
    batches = [data.labelled() for _ in range(2)]                         # Measurement.recall (hits / ground-truth pixels per image) is finite
    assert all(len(torch.unique(lab[i])) == 3 for _, lab in batches for i in range(lab.shape[0]))
    got = tr.evaluate(batches, which="teacher", index=1)
    fresh = make_model(_model()).to(dev())
    fresh.load_state_dict(tr.averages[1].state_dict()["module"])
    want = test_loop(fresh, batches, 3, device=dev(), amp_dtype=torch.bfloat16)
    assert got == want and all(np.isfinite(v).all() for v in got.values()), (got, want)
    assert tr.evaluate(batches, which="student", index=1) == test_loop(tr.models[1], batches, 3, device=dev(), amp_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        _run("plain")["tr"].evaluate(batches, which="teacher")
