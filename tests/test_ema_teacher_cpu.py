"""The averaged ("teacher") networks without a GPU: the emulation the GPU tests compare against is itself checked (exact rational
arithmetic; a counted float64 bar), the assertion function the GPU tests use catches emulations that carry one defect each, the
second struct and the entry point's refusals, and the host classes (averaging.AveragedNetwork, CPSConfig, optim.HipAdam's layout)."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch
from torch import nn

from tests import ema_cases as E
from tests import optim_cases as C


# ------------------------------------------------------------------------------------------------ the emulation
def _special_pairs():
    """(e, p') of about 2k elements: +-0, subnormals, opposite signs near cancellation, ordinary values; then +-inf and NaN"""
    f = np.float32
    rs = np.random.RandomState(11)
    base = [f(0.0), f(-0.0), f(1e-45), f(-1e-45), f(3e-42), f(-7e-40), f(1.1754942e-38), f(-1.1754944e-38), f(1e-30), f(0.1), f(-0.1), f(0.25),
            f(3.3e38), f(-3.3e38), f(1.0), f(np.nextafter(f(1.0), f(2.0))), f(-np.nextafter(f(1.0), f(0.0)))]
    grid = [(a, b) for a in base for b in base]                                           # 289
    near = rs.uniform(-1, 1, 600).astype(f)
    cancel = [(a, f(-a * f(1 + k * 2.0 ** -23))) for a, k in zip(near, rs.randint(-3, 4, 600))]   # opposite signs, |p'| within 3 ulp of |e|
    close = [(a, np.nextafter(a, f(np.inf) if k else f(-np.inf))) for a, k in zip(near[:300], rs.randint(0, 2, 300))]
    ordinary = list(zip(E.ema_data(12, 800), C.adam_data(13, 800)[0]))
    finite = np.array(grid + cancel + close + ordinary, dtype=f)
    nonfinite = np.array([(a, b) for a in (f(np.inf), f(-np.inf), f(np.nan)) for b in base] + [(a, b) for b in (f(np.inf), f(-np.inf), f(np.nan)) for a in base]
                         + [(f(np.inf), f(np.inf)), (f(np.inf), f(-np.inf)), (f(np.nan), f(np.inf))], dtype=f)
    return finite, nonfinite


@pytest.mark.parametrize("decay", [E.DECAY, 0.999, 0.0, 0.5])
def test_emulation_against_exact_rational_arithmetic(decay):
    finite, nonfinite = _special_pairs()
    assert finite.shape[0] >= 1900
    e, p = finite[:, 0], finite[:, 1]
    got = E.ema_emulate(e, p, decay, False)
    w = E.ema_weight(decay)
    want = np.empty_like(got)
    for i, (a, b) in enumerate(zip(e, p)):
        d = C.round_fraction_f32(Fraction(float(b)) - Fraction(float(a)))                 # the difference, rounded once
        if np.isinf(d):                                                                   # 3.3e38 - (-3.3e38): the fma of an infinity
            want[i] = d
        elif a == 0 and b == 0:                                                           # signed zeros follow IEEE rules, not rationals:
            with np.errstate(all="ignore"):                                               # every operation on them is exact
                want[i] = w * (b - a) + a
        else:
            want[i] = C.fma32_fraction(w, d, a)                                           # the fma, rounded once
    C.check_bits(got, want, f"ema_emulate against rational arithmetic, decay {decay}")
    # infinities and NaN: the float64 evaluation has the same special results; NaN compared by position
    e, p = nonfinite[:, 0], nonfinite[:, 1]
    with np.errstate(all="ignore"):
        want = (e.astype(np.float64) + float(E.ema_weight(decay)) * (p - e).astype(np.float64)).astype(np.float32)
    got = E.ema_emulate(e, p, decay, False)
    assert (np.isnan(got) == np.isnan(want)).all() and np.isnan(want).sum() >= 30
    C.check_bits(got, want, f"ema_emulate on infinities and NaN, decay {decay}")
    # copy: the bits, NaN included by position
    C.check_bits(E.ema_emulate(e, p, decay, True), p, "copy")
    assert (C.f32_bits(E.ema_emulate(finite[:, 0], finite[:, 1], decay, True)) == C.f32_bits(finite[:, 1])).all()


@pytest.mark.parametrize("decay", [E.DECAY, 0.999, 0.9])
def test_emulation_within_the_counted_bar_of_float64(decay):
    n = 20000
    e, p = E.ema_data(21, n), C.adam_data(22, n)[0]
    got = E.ema_emulate(e, p, decay, False).astype(np.float64)
    ref, bar = E.ema_fp64(e, p, decay)
    ratio = np.abs(got - ref) / bar
    C.note("ema fp64", f"decay {decay}: worst share of the counted bar h(e') + w h(p' - e)", float(ratio.max()), 1.0)
    assert ratio.max() <= 1.0, f"off by {ratio.max():.3g} of the counted bar at {int(ratio.argmax())}"
    assert ratio.max() > 0.2, "a bar five times too wide would prove little"


# ------------------------------------------------------------------------------------------------ defects
@pytest.mark.parametrize("defect", E.DEFECTS)
def test_the_gpu_tests_assertion_catches_each_defect(defect):
    n = 4099
    p_old, g, m, v = C.adam_data(31, n)
    p_new = C.adam_emulate(p_old, g, m, v, *C.HYPER)[0]
    e = E.ema_data(32, n)
    copy = defect == "copy_ignored"
    good = E.ema_emulate(e, p_new, E.DECAY, copy)
    E.check_ema(good, e, p_new, E.DECAY, copy, "the emulation itself")
    bad = E.ema_emulate(e, p_new, E.DECAY, copy, defect=defect, p_old=p_old)
    with pytest.raises(AssertionError):
        E.check_ema(bad, e, p_new, E.DECAY, copy, defect)
    E.check_ema(bad, e, p_new, E.DECAY, copy, defect, defect=defect, p_old=p_old)         # and the defect is what was asked for


# ------------------------------------------------------------------------------------------------ ABI
def test_struct_is_forty_bytes_and_matches_the_header():
    from vq_seg_amd.optim import _EMA_REC, _REC
    assert _EMA_REC.itemsize == 40 and _REC.itemsize == 80
    assert [(_EMA_REC.fields[n][1], n) for n in _EMA_REC.names] == [(0, "e"), (8, "copy"), (12, "reserved"), (16, "fwd"), (24, "tr"), (32, "s3")]


def test_entry_point_refuses_bad_arguments_on_the_host():
    from vq_seg_amd import _hip
    L = _hip.lib()
    buf = ctypes.create_string_buffer(256)                                # never read: every call below is refused before a launch
    ptr = ctypes.addressof(buf)
    ok = dict(params=ptr, ema=ptr, items=ptr, n=1, step=3, decay=0.99)
    cases = [dict(params=None), dict(ema=None), dict(items=None), dict(n=0), dict(n=-1), dict(step=0), dict(decay=-0.1), dict(decay=1.0),
             dict(decay=float("nan"))]
    for case in cases:
        a = dict(ok, **case)
        rc = L.vqseg_adam_ema_step_f32(a["params"], a["ema"], a["items"], a["n"], 1e-3, 0.9, 0.999, 1e-8, a["step"], a["decay"], 0, None)
        assert rc == -1, case
        msg = L.vqseg_last_error().decode()
        assert "adam_ema_step" in msg, (case, msg)
        if "decay" in case:
            assert "ema_decay" in msg, msg


# ------------------------------------------------------------------------------------------------ host classes
class _Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        from vq_seg_amd.vector_quantizer.vq_img import VectorQuantizer
        self.conv, self.bn = nn.Conv2d(4, 8, 3, bias=False), nn.BatchNorm2d(8)
        self.vq = VectorQuantizer(8, 16, ema_update=True, threshold_ema_dead_code=1.0)
        self.scale = nn.Parameter(torch.ones(8))


def _tiny_pair():
    from vq_seg_amd.averaging import AveragedNetwork
    torch.manual_seed(1)
    student = _Tiny()
    student.conv.weight._vq_kinds = {"fwd"}                               # kernel-side attributes a deepcopy would drag along
    student.bn.running_mean.uniform_(-1, 1)
    student.bn.num_batches_tracked.fill_(7)
    student.vq.codebook.initted = True
    return student, AveragedNetwork(student, _Tiny, 0.99)


def test_averaged_network_starts_as_the_student_and_pairs_by_name():
    student, avg = _tiny_pair()
    assert avg.decay == 0.99 and avg.updates == 0 and isinstance(avg.updates, int)
    teacher = avg.module
    assert teacher is not student and not teacher.training and not any(p.requires_grad for p in teacher.parameters())
    assert student.training and all(p.requires_grad for p in student.parameters())
    assert not hasattr(teacher.conv.weight, "_vq_kinds") and teacher.vq.codebook.initted is True
    a, b = student.state_dict(), teacher.state_dict()
    assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert all(x.data_ptr() != y.data_ptr() for x, y in zip(a.values(), b.values()))
    pairs = {p.name: p for p in avg.pairs}
    floating = [n for n, t in list(student.named_parameters()) + list(student.named_buffers()) if t.is_floating_point()]
    assert sorted(pairs) == sorted(floating)
    assert sorted(n for n, p in pairs.items() if p.copy) == ["vq.codebook.cluster_size", "vq.codebook.embed_avg", "vq.codebook.embedding.weight"]
    assert sorted(n for n, p in pairs.items() if p.average_only) == sorted(n for n, t in student.named_buffers() if t.is_floating_point())
    assert "bn.running_mean" in pairs and pairs["bn.running_mean"].average_only and not pairs["bn.running_mean"].copy
    assert "bn.num_batches_tracked" not in pairs and "vq.codebook.ema_updates" not in pairs
    named_s, named_t = dict(student.named_parameters()), dict(teacher.named_parameters())
    assert pairs["conv.weight"].student is named_s["conv.weight"] and pairs["conv.weight"].teacher is named_t["conv.weight"]
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            from vq_seg_amd.averaging import AveragedNetwork
            AveragedNetwork(student, _Tiny, bad)


def test_averaged_network_state_round_trips():
    from vq_seg_amd.averaging import AveragedNetwork
    student, avg = _tiny_pair()
    with torch.no_grad():
        avg.module.conv.weight.add_(0.5)
        student.bn.num_batches_tracked.fill_(9)                           # integer buffers: the student's, copied when the state is asked for
    avg.updates = 5
    state = avg.state_dict()
    assert set(state) == {"module", "updates"} and state["updates"] == 5
    assert int(state["module"]["bn.num_batches_tracked"]) == 9
    state = {"module": {k: v.clone() for k, v in state["module"].items()}, "updates": 5}
    other = AveragedNetwork(_Tiny(), _Tiny, 0.99)
    other.load_state_dict(state)
    assert other.updates == 5 and not other.module.training
    back = other.state_dict()["module"]
    assert all(torch.equal(back[k], state["module"][k]) for k in back if k != "bn.num_batches_tracked" and k != "vq.codebook.ema_updates")
    avg.reset_from_student()
    assert avg.updates == 0 and torch.equal(avg.module.conv.weight, student.conv.weight)


def test_config_validation_and_no_cpu_path():
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer
    assert CPSConfig(model={}).ema_decay is None and CPSConfig(model={}).teacher_pseudo_labels is False
    CPSConfig(model={}, ema_decay=0.0), CPSConfig(model={}, ema_decay=0.999, teacher_pseudo_labels=True)
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            CPSConfig(model={}, ema_decay=bad)
    with pytest.raises(ValueError, match="ema_decay"):
        CPSConfig(model={}, teacher_pseudo_labels=True)
    with pytest.raises(ValueError, match="no CPU path"):
        CPSTrainer(CPSConfig(model={}, ema_decay=0.99), torch.device("cpu"))


def test_hip_adam_keeps_torch_adams_layout_with_an_average_attached():
    from vq_seg_amd.optim import HipAdam
    student, avg = _tiny_pair()
    ref = torch.optim.Adam(student.parameters(), lr=1e-3, betas=(0.9, 0.999))
    for p in student.parameters():
        p.grad = torch.ones_like(p)
    ref.step()
    opt = HipAdam(student.parameters(), lr=1e-3)
    opt.attach_average(avg)
    opt.load_state_dict(ref.state_dict())
    a, b = opt.state_dict(), ref.state_dict()
    assert set(a) == set(b) == {"state", "param_groups"}
    assert list(a["state"]) == list(b["state"]) and all(set(a["state"][k]) == set(b["state"][k]) == {"step", "exp_avg", "exp_avg_sq"} for k in a["state"])
    assert [set(g) for g in a["param_groups"]] == [set(g) for g in b["param_groups"]]
    with pytest.raises(Exception, match="no CPU"):                        # and no CPU path with an average either
        opt.step()
    assert avg.updates == 0
