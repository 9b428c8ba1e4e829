"""vqseg_adam_step_f32 and the weight-image kernels through the C ABI, on every path, against tests/optim_cases.py:
  * p, m, v bit for bit against the float32 emulation of `adam_one` (flat vector body, its tail, the scalar body, the 3 x 3 and 1 x 1
    convolution tiles, any order of the item table, special values), and per element against one float64 step;
  * every image the step writes, and every image of the four pack entry points, bit for bit against NumPy layouts written from the
    documented index order, padding zero, past the 4096-workgroup cap of the grid-stride kernels;
  * every p / g / m / v / image buffer between sentinel words that must survive;
  * the host paths of optim.HipAdam against torch.optim.Adam on the CPU: moments bit for bit, parameters within
    optim_cases.TORCH_P_BAR_ULP.
Measured figures (pytest -s prints them before it asserts): profiles/optim_parity.md."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from tests import optim_cases as C

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def lib():
    from vq_seg_amd import _hip
    return _hip.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def _step(params, hyper, order="sorted", label=""):
    rc = C.adam_launch(params, C.adam_items(params, order, seed=5), hyper)
    assert rc == 0, (label, lib().vqseg_last_error())


def _same_bits(a, b, label):
    for name, x, y in zip("pmv", a, b):
        assert (C.f32_bits(x) == C.f32_bits(y)).all(), f"{label}: {name} differs between the two runs"


# ------------------------------------------------------------------------------------------------ flat path
@pytest.mark.parametrize("n", C.FLAT_NUMELS)
def test_flat_chunks_vector_body_tail_and_scalar_body(n):
    """all four pointers 16-byte aligned: the f32x4 body and its `end4` tail; exactly one of p, g, m, v one float off: the scalar body.
    Each run bit-equal to the emulation, the five runs bit-identical to each other, the gradient and every guard untouched."""
    state = C.flat_state(n)
    runs = {}
    for off in (None, "p", "g", "m", "v"):
        P = C.AdamParam(dev(), state, shift={off: 1} if off else None)
        misaligned = [name for name in "pgmv" if P.buf[name].ptr % 16]
        assert misaligned == ([off] if off else []), "the case must decide `vec` in adam_flat_chunk"
        _step([P], C.HYPER, label=(n, off))
        runs[off] = P.results()
        C.check_adam_emulation(runs[off], state, C.HYPER, f"flat {n}, {off or 'no'} pointer offset")
        assert (C.f32_bits(P.buf["g"].get()) == C.f32_bits(state[1])).all() and P.guards_intact(), (n, off)
        _same_bits(runs[off], runs[None], f"flat {n}: vector body against the scalar body ({off} offset)")
    C.check_adam_fp64(runs[None], state, C.HYPER, f"flat {n}")


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("eps", [1e-8, 0.0])
@pytest.mark.parametrize("betas", C.VALUE_BETAS)
@pytest.mark.parametrize("step", C.VALUE_STEPS)
def test_special_values_follow_ieee_arithmetic(step, betas, eps):
    """+-0, subnormal, underflowing / overflowing squares, +-inf and NaN gradients, v = 0 (with eps = 0: 0 / 0 and x / 0), subnormal
    moments, +-0 parameters: the emulation's bits, NaNs by position, through the vector and the scalar body"""
    state = C.special_values()
    hyper = (3e-3, betas[0], betas[1], eps, step)
    runs = []
    for shift in (None, {"g": 1}):
        P = C.AdamParam(dev(), state, shift=shift)
        _step([P], hyper, label=hyper)
        runs.append(P.results())
        C.check_adam_emulation(runs[-1], state, hyper, f"special values, step {step}, betas {betas}, eps {eps}, {'scalar' if shift else 'vector'} body")
        assert P.guards_intact()
    for name, a, b in zip("pmv", *runs):
        C.check_bits(a, b, f"special values {name}: vector body against scalar body")


# ------------------------------------------------------------------------------------------------ convolution tiles
def _image_sets(cin):
    sets = [((), None), (("fwd",), None), (("tr",), None)]
    if cin % 32 == 0:
        for c1 in C.s3_splits(cin):
            sets += [(("s3",), c1), (("fwd", "tr", "s3"), c1)]
    else:
        sets.append((("fwd", "tr"), None))
    return sets


@pytest.mark.parametrize("k,cout,cin", [(3, a, b) for a, b in C.K3_SHAPES] + [(1, a, b) for a, b in C.K1_SHAPES])
def test_convolution_tiles_update_and_rewrite_the_images(k, cout, cin):
    """adam_conv_tile<3, 32> / <1, 128> with every image subset (none: the return before the barrier): p, m, v bit-equal to the
    emulation AND to the flat path on the same data; every image bit-equal to the NumPy layout of the new p; padding zero; guards"""
    state = C.tile_state(k, cout, cin)
    flat = C.AdamParam(dev(), state)
    _step([flat], C.HYPER)
    want = C.check_adam_emulation(flat.results(), state, C.HYPER, f"k{k} {cout}x{cin} flat")
    C.check_adam_fp64(flat.results(), state, C.HYPER, f"k{k} {cout}x{cin}")
    assert C.work_items(state[0].size, k, cout, cin) == C.WORK_ITEM_COUNTS[(state[0].size, k, cout, cin)]
    for images, c1 in _image_sets(cin):
        label = f"k{k} {cout}x{cin} images {images or 'none'} c1 {c1}"
        P = C.AdamParam(dev(), state, k=k, cout=cout, cin=cin, c1=c1 or cin, images=images)
        _step([P], C.HYPER, label=label)
        got = P.results()
        C.check_adam_emulation(got, state, C.HYPER, label)
        _same_bits(got, flat.results(), f"{label}: tile path against flat path")
        for name, img in C.expected_images(want[0], k, cout, cin, c1 or cin, images).items():
            C.check_image(P.img[name].get(), img, f"{label}: {name}", padding=C.image_padding(name, k, cout, cin))
        assert P.guards_intact(), label


# ------------------------------------------------------------------------------------------------ item table
def _mixed_table():
    specs = [dict(state=C.flat_state(8195)), dict(state=C.tile_state(1, 40, 129), k=1, cout=40, cin=129, images=("fwd", "tr")),
             dict(state=C.flat_state(5)), dict(state=C.tile_state(3, 40, 33), k=3, cout=40, cin=33, images=("fwd", "tr")),
             dict(state=tuple(np.zeros(0, np.float32) for _ in range(4))),                         # numel = 0: no work item
             dict(state=C.tile_state(3, 64, 64), k=3, cout=64, cin=64, c1=32, images=("fwd", "tr", "s3")),
             dict(state=C.tile_state(1, 64, 256), k=1, cout=64, cin=256, c1=224, images=("s3",)), dict(state=C.flat_state(4096))]
    return specs, [C.AdamParam(dev(), **s) for s in specs]


def test_item_table_in_any_order_and_work_item_counts():
    L = lib()
    for (numel, k, cout, cin), want in C.WORK_ITEM_COUNTS.items():
        assert L.vqseg_adam_work_items(numel, k, cout, cin) == want, (numel, k, cout, cin)
    results = {}
    for order in ("sorted", "reversed", "shuffled"):
        specs, params = _mixed_table()
        assert sum(p.n_items() for p in params) == 3 + 4 + 1 + 4 + 0 + 4 + 4 + 1
        _step(params, C.HYPER, order=order, label=order)
        results[order] = []
        for i, (s, P) in enumerate(zip(specs, params)):
            got = P.results()
            want = C.check_adam_emulation(got, s["state"], C.HYPER, f"table ({order}) parameter {i}")
            if P.numel:
                C.check_adam_fp64(got, s["state"], C.HYPER, f"table ({order}) parameter {i}")
            for name, img in C.expected_images(want[0], P.k, P.cout, P.cin, P.c1, tuple(P.img)).items():
                C.check_image(P.img[name].get(), img, f"table ({order}) parameter {i}: {name}", padding=C.image_padding(name, P.k, P.cout, P.cin))
            assert P.guards_intact(), (order, i)
            results[order].append(got + tuple(P.img[name].get() for name in sorted(P.img)))
    for order in ("reversed", "shuffled"):
        for a, b in zip(results[order], results["sorted"]):
            assert all((x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(a, b)), order


def test_refused_calls_leave_every_buffer_untouched():
    L = lib()
    _, params = _mixed_table()
    items = C.adam_items(params)
    lr, b1, b2, eps, step = C.HYPER
    refused = [dict(hyper=(lr, b1, b2, eps, 0)), dict(hyper=(lr, 1.0, b2, eps, step)), dict(hyper=(lr, b1, 1.0, eps, step)),
               dict(hyper=(lr, b1, b2, -1e-8, step)), dict(hyper=C.HYPER, null_params=True), dict(hyper=C.HYPER, null_items=True),
               dict(hyper=C.HYPER, n_items=0)]
    for kw in refused:
        hyper = kw.pop("hyper")
        assert C.adam_launch(params, items, hyper, **kw) != 0, (hyper, kw)
        assert L.vqseg_last_error(), (hyper, kw)
    assert all(P.untouched() and P.guards_intact() for P in params)
    _step(params, C.HYPER)                                               # and the same table is served once the arguments are valid
    assert not any(P.untouched() for P in params if P.numel)


# ------------------------------------------------------------------------------------------------ pack kernels
def _pack(name, w, out_elems, call):
    """run one pack entry point on a guarded weight and guarded outputs (None: a NULL output) -> {output: uint16 image}"""
    wb = C.Guarded(dev(), w.size, "f32", values=w)
    outs = {k: (C.Guarded(dev(), n, "i16") if n is not None else None) for k, n in out_elems.items()}
    rc = call(wb.ptr, {k: (b.ptr if b is not None else None) for k, b in outs.items()})
    assert rc == 0, (name, lib().vqseg_last_error())
    torch.cuda.synchronize()
    assert wb.guards_intact() and (C.f32_bits(wb.get()) == C.f32_bits(w).reshape(-1)).all(), name
    assert all(b.guards_intact() for b in outs.values() if b is not None), f"{name}: a guard word was overwritten"
    return {k: b.get() for k, b in outs.items() if b is not None}


def _check_single(w, flip, with_lo, label):
    L = lib()
    cout, cin, kh, kw = w.shape
    n = int(L.vqseg_conv_packed_elems(cout, cin, kh, kw, flip))
    assert n == (C.tr_elems if flip else C.fwd_elems)(cout, cin, kh, kw), label
    got = _pack(label, w, {"hi": n, "lo": n if with_lo else None},
                lambda wp, o: L.vqseg_conv_pack_weights_f32(wp, cout, cin, kh, kw, flip, o["hi"], o["lo"], stream()))
    ref = C.image_tr if flip else C.image_fwd
    pad = C.padding_mask((cin if flip else cout) * kh * kw, cout if flip else cin)
    C.check_image(got["hi"], ref(w), f"{label} hi", padding=pad)
    if with_lo:
        C.check_image(got["lo"], ref(w, lo=True), f"{label} lo", padding=pad)
        in_image_order = w[:, :, ::-1, ::-1].transpose(1, 2, 3, 0) if flip else w.transpose(0, 2, 3, 1)
        C.check_lo_property(np.ascontiguousarray(in_image_order), got["hi"][~pad], got["lo"][~pad], label)


@pytest.mark.parametrize("shape", [(64, 3, 7, 7), (5, 7, 1, 3), (40, 24, 3, 3), (33, 65, 1, 1)])
@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("with_lo", [False, True])
def test_pack_weights_against_the_numpy_layout(shape, flip, with_lo):
    _check_single(C.weight(sum(shape), shape), flip, with_lo, f"pack_weights {shape} flip {flip}")


def _check_s3(w, c1, label):
    L = lib()
    cout, cin, kh, kw = w.shape
    got = _pack(label, w, {"s3": cout * kh * kw * 3 * cin}, lambda wp, o: L.vqseg_conv_pack_weights_s3_f32(wp, cout, cin, c1, kh, kw, o["s3"], stream()))
    C.check_image(got["s3"], C.image_s3(w, c1), label)


@pytest.mark.parametrize("cout,cin,k,c1", [(64, 64, 3, 32), (64, 64, 3, 64), (32, 96, 1, 64)])
def test_pack_weights_s3_against_the_numpy_layout(cout, cin, k, c1):
    _check_s3(C.weight(cout + cin + c1, (cout, cin, k, k)), c1, f"pack_weights_s3 {cout}x{cin} k{k} c1 {c1}")


def _check_s2(w, with_lo, label):
    L = lib()
    cout, cin, k, _ = w.shape
    n = int(L.vqseg_conv_packed_s2_elems(cout, cin, k))
    assert n == cin * k * k * ((cout + 31) // 32 * 32) == C.image_s2(w).size, label
    got = _pack(label, w, {"hi": n, "lo": n if with_lo else None}, lambda wp, o: L.vqseg_conv_pack_weights_s2_f32(wp, cout, cin, k, o["hi"], o["lo"], stream()))
    pad = C.padding_mask(cin * k * k, cout)
    C.check_image(got["hi"], C.image_s2(w), f"{label} hi", padding=pad)
    if with_lo:
        C.check_image(got["lo"], C.image_s2(w, lo=True), f"{label} lo", padding=pad)


@pytest.mark.parametrize("cout,cin,k", [(40, 24, 3), (64, 64, 3), (33, 65, 1)])
@pytest.mark.parametrize("with_lo", [False, True])
def test_pack_weights_s2_against_the_numpy_layout(cout, cin, k, with_lo):
    """the parity-class sub-images of the stride-2 data gradient: classes (0,0), (0,1), (1,0), (1,1), even parity = taps (2, 0)"""
    _check_s2(C.weight(cout + cin + k, (cout, cin, k, k)), with_lo, f"pack_weights_s2 {cout}x{cin} k{k}")


@pytest.mark.parametrize("k,cout,cin", [(3, a, b) for a, b in C.K3_SHAPES] + [(1, a, b) for a, b in C.K1_SHAPES])
def test_pack_all_against_the_numpy_layout_with_each_output_null_in_turn(k, cout, cin):
    L = lib()
    w = C.weight(k + cout + cin, (cout, cin, k, k))
    names = ("fwd", "tr", "s3") if cin % 32 == 0 else ("fwd", "tr")
    sizes = {"fwd": C.fwd_elems(cout, cin, k, k), "tr": C.tr_elems(cout, cin, k, k), "s3": cout * k * k * 3 * cin}
    for c1 in (C.s3_splits(cin) if cin % 32 == 0 else [cin]):
        for null in (None,) + names:
            present = tuple(n for n in names if n != null)
            if not present:
                continue
            label = f"pack_all k{k} {cout}x{cin} c1 {c1} outputs {present}"
            got = _pack(label, w, {n: (sizes[n] if n in present else None) for n in ("fwd", "tr", "s3")},
                        lambda wp, o: L.vqseg_conv_pack_all_f32(wp, cout, cin, k, c1, o["fwd"], o["tr"], o["s3"], stream()))
            for name, img in C.expected_images(w, k, cout, cin, c1, present).items():
                C.check_image(got[name], img, f"{label}: {name}", padding=C.image_padding(name, k, cout, cin))


@pytest.mark.parametrize("kernel", ["fwd", "s3", "s2"])
def test_grid_stride_pass_of_the_pack_kernels(kernel):
    """just over the 4096 x 256 elements one pass of a capped grid covers: the elements of the second pass against the same layouts"""
    if kernel == "fwd":
        w = C.weight(41, (512, 256, 3, 3))
        assert C.fwd_elems(512, 256, 3, 3) > C.PACK_GRID_CAP
        _check_single(w, 0, True, "pack_weights 512x256x3x3 past the grid cap")
    elif kernel == "s3":
        w = C.weight(42, (256, 160, 3, 3))
        assert 256 * 9 * 3 * 160 > C.PACK_GRID_CAP
        _check_s3(w, 128, "pack_weights_s3 256x160x3x3 past the grid cap")
    else:
        w = C.weight(43, (512, 256, 3, 3))
        assert 256 * 9 * 512 > C.PACK_GRID_CAP
        _check_s2(w, True, "pack_weights_s2 512x256 k3 past the grid cap")


# ------------------------------------------------------------------------------------------------ HipAdam host paths
SHAPES = [(5001,), (40, 24, 3, 3), (64, 32, 3, 3), (3, 32)]


def _twins(with_kinds=True):
    cpu = [nn.Parameter(torch.from_numpy(C.adam_data(800 + i, int(np.prod(s)))[0].reshape(s).copy())) for i, s in enumerate(SHAPES)]
    gpu = [nn.Parameter(p.detach().to(dev())) for p in cpu]
    if with_kinds:
        for q in gpu:
            if q.dim() == 4:
                q._vq_kinds = {"fwd", "tr"} | ({("s3", q.shape[1])} if q.shape[1] % 32 == 0 else set())
    return cpu, gpu


def _grad(step, i):
    return torch.from_numpy(C.adam_data(900 + 10 * step + i, int(np.prod(SHAPES[i])))[1].reshape(SHAPES[i]).copy())


def _images_match(q, label):
    w = q.detach().cpu().numpy()
    for kind, img in q._vq_pack["all"].items():
        want = C.image_s3(w, kind[1]) if isinstance(kind, tuple) else (C.image_fwd(w) if kind == "fwd" else C.image_tr(w))
        C.check_image(img.cpu().numpy(), want, f"{label} {kind}")


def _compare(ref, opt, cpu, gpu, before, label):
    """moments bit for bit, parameters within the bar of the emulation against torch, the installed images those of the new weight;
    then the CPU parameter takes the GPU's value, so the next step starts from identical state and the bar holds per step"""
    torch.cuda.synchronize()
    for i, (p, q) in enumerate(zip(cpu, gpu)):
        if p not in ref.state or not ref.state[p]:
            assert q not in opt.state or not opt.state[q], (label, i)
            assert torch.equal(q.detach().cpu(), p.detach())
            continue
        got = (q.detach().cpu().numpy(), opt.state[q]["exp_avg"].cpu().numpy(), opt.state[q]["exp_avg_sq"].cpu().numpy())
        want = (p.detach().numpy(), ref.state[p]["exp_avg"].numpy(), ref.state[p]["exp_avg_sq"].numpy())
        C.check_against_torch(got, want, before[i], f"{label} parameter {i}")
        assert float(opt.state[q]["step"]) == float(ref.state[p]["step"]) and opt.state[q]["step"].device.type == "cpu"
        if getattr(q, "_vq_kinds", None) and getattr(q, "_vq_pack", None):
            _images_match(q, f"{label} parameter {i}")
        with torch.no_grad():
            p.copy_(q.detach().cpu())


def test_hip_adam_first_gradient_on_a_later_step_two_step_counts_two_launches():
    from vq_seg_amd.optim import HipAdam
    cpu, gpu = _twins()
    ref = torch.optim.Adam(cpu, lr=3e-3, foreach=False, fused=False)
    opt = HipAdam(gpu, lr=3e-3)
    late = 1                                                             # the 40 x 24 x 3 x 3 weight gets its first gradient on step 3 of 5
    bufs = [torch.empty(s, device=dev()) for s in SHAPES]                # fixed gradient storage: the tables can be reused
    sigs = []
    for step in range(1, 6):
        before = [p.detach().numpy().copy() for p in cpu]
        for i, (p, q) in enumerate(zip(cpu, gpu)):
            g = None if (i == late and step < 3) else _grad(step, i)
            p.grad, q.grad = g, (None if g is None else bufs[i].copy_(g))
        ref.step()
        opt.step()
        _compare(ref, opt, cpu, gpu, before, f"late gradient, step {step}")
        if step >= 3:
            assert float(opt.state[gpu[late]]["step"]) == step - 2 and float(opt.state[gpu[0]]["step"]) == step
            subs = {k: t for k, t in opt._tables.items() if isinstance(k, tuple)}
            assert len(subs) == 2, "two step counts -> two sub-tables (two launches), kept from step to step"
            assert sorted(len(t["images"]) for t in subs.values()) == [1, 3]
            sigs.append(tuple(t["sig"] for _, t in sorted(subs.items())))
            assert gpu[late]._vq_pack is not None and set(gpu[late]._vq_pack["all"]) == {"fwd", "tr"}
    assert len(set(sigs)) == 1 and len(opt._tables) == 3, "the sub-tables of steps 3, 4 and 5 are the same two"


def test_hip_adam_rebuilds_its_table_when_a_gradient_is_reallocated():
    from vq_seg_amd.optim import HipAdam
    cpu, gpu = _twins()
    ref = torch.optim.Adam(cpu, lr=3e-3, foreach=False, fused=False)
    opt = HipAdam(gpu, lr=3e-3)
    keep, sigs = [], []
    for step in range(1, 4):
        before = [p.detach().numpy().copy() for p in cpu]
        for i, (p, q) in enumerate(zip(cpu, gpu)):
            p.grad = _grad(step, i)
            q.grad = p.grad.to(dev())                                    # a NEW allocation every step (the old ones are kept alive)
            keep.append(q.grad)
        ref.step()
        opt.step()
        _compare(ref, opt, cpu, gpu, before, f"reallocated gradient, step {step}")
        sigs.append(opt._tables[0]["sig"])
    assert len({id(t) for t in keep}) == len(keep) and len(set(sigs)) == 3, "every step saw other gradient pointers"


def test_hip_adam_takes_lr_as_a_tensor():
    from vq_seg_amd.optim import HipAdam
    cpu, gpu = _twins()
    ref = torch.optim.Adam(cpu, lr=torch.tensor(3e-3), foreach=False, fused=False)
    opt = HipAdam(gpu, lr=torch.tensor(3e-3))
    for step in range(1, 3):
        before = [p.detach().numpy().copy() for p in cpu]
        for i, (p, q) in enumerate(zip(cpu, gpu)):
            p.grad = _grad(step, i)
            q.grad = p.grad.to(dev())
        ref.step()
        opt.step()
        _compare(ref, opt, cpu, gpu, before, f"tensor lr, step {step}")


def test_hip_adam_accepts_a_state_dict_with_device_side_step_counters():
    from vq_seg_amd.optim import HipAdam
    cpu, gpu = _twins()
    ref = torch.optim.Adam(cpu, lr=3e-3, foreach=False, fused=False)
    first = HipAdam(gpu, lr=3e-3)
    opt = first
    for step in range(1, 4):
        before = [p.detach().numpy().copy() for p in cpu]
        for i, (p, q) in enumerate(zip(cpu, gpu)):
            p.grad = _grad(step, i)
            q.grad = p.grad.to(dev())
        if step == 2:                                                    # what a fused / capturable optimiser's checkpoint holds
            sd = copy.deepcopy(first.state_dict())
            for st in sd["state"].values():
                st["step"] = st["step"].to(dev())
            opt = HipAdam(gpu, lr=3e-3)
            opt.load_state_dict(sd)
            assert all(opt.state[q]["step"].device.type == "cuda" for q in gpu)
        ref.step()
        opt.step()
        _compare(ref, opt, cpu, gpu, before, f"device-side step, step {step}")


@pytest.mark.parametrize("case", ["two_s3_kinds", "s3_kind_with_ragged_cin"])
def test_hip_adam_serves_a_weight_without_an_image_plan_through_the_flat_path(case):
    """a 3 x 3 weight whose images vqseg_conv_pack_all_f32 does not serve: updated as a plain parameter, its stale `_vq_pack` dropped,
    and the next convolution reads the new weight"""
    from vq_seg_amd import nnf
    from vq_seg_amd.optim import HipAdam, _image_plan
    torch.manual_seed(0)
    cin = 64 if case == "two_s3_kinds" else 24
    conv, bn = nn.Conv2d(cin, 64, 3, padding=1, bias=False).to(dev()), nn.BatchNorm2d(64).to(dev())
    x = torch.rand(2, cin, 16, 16, device=dev()).contiguous(memory_format=torch.channels_last).bfloat16().requires_grad_(True)
    params = list(conv.parameters()) + list(bn.parameters())
    opt = HipAdam(params, lr=0.05)
    cpu = [nn.Parameter(p.detach().cpu().clone()) for p in params]
    ref = torch.optim.Adam(cpu, lr=0.05, foreach=False, fused=False)
    for it in range(2):
        y0 = nnf.conv_bn_act(x, conv, bn)
        y0.float().square().mean().backward()
        conv.weight._vq_kinds |= {("s3", 32), ("s3", 64)} if case == "two_s3_kinds" else {("s3", cin)}
        assert _image_plan(conv.weight) is None
        assert getattr(conv.weight, "_vq_pack", None) is not None, "the forward pass left a cache that the step must drop"
        before = [p.detach().numpy().copy() for p in cpu]
        for p, q in zip(cpu, params):
            p.grad = q.grad.detach().cpu().clone()
        ref.step()
        opt.step()
        assert conv.weight._vq_pack is None and opt._tables[0]["images"][0] is None
        _compare(ref, opt, cpu, params, before, f"{case}, step {it + 1}")
        opt.zero_grad()
    y1 = nnf.conv_bn_act(x, conv, bn)
    fresh_c, bn2 = copy.deepcopy(conv), copy.deepcopy(bn)
    fresh_c.weight._vq_pack = None
    assert torch.equal(y1, nnf.conv_bn_act(x, fresh_c, bn2)) and not torch.equal(y1, y0)
