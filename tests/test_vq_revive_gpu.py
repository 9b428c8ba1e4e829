"""Dead-code revival of the EMA codebook on the GPU (include/vqseg.h, EMA EXTENSION): vqseg_vq_revive_candidates and
vqseg_vq_ema_update_revive_f32 against the CPU restatement of tests/vq_revive_cases.py, then the module, the trainer and two
data-parallel ranks.  Bars (see tests/vq_revive_cases.py): candidates and revived state bit for bit; everything that is not revived
bit-equal to vqseg_vq_ema_update_f32 -- the OLD entry point -- on the same inputs and within the bars tests/vq_tail_cases.ema_reference
counts against float64.  Every output buffer starts as NaN (integers: -1) with guard elements behind it that must keep that fill."""
import numpy as np
import pytest
import torch

from tests import synth
from tests import vq_revive_cases as RC
from tests import vq_tail_cases as T
from tests.test_dp_cpu import spawn
from tests.test_nn_kernels_gpu import BF16, F32, dev, nan_like

pytestmark = pytest.mark.gpu
G = T.GUARD
SEED = (1 << 64) - 59                                                  # above 2^63: the seed crosses the boundary as an unsigned 64-bit


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def guarded(n, dtype=F32):
    """-> (the first n elements, the guard behind them) of one NaN / -1 filled buffer"""
    buf = nan_like((n + G,), dtype)
    return buf[:n], buf[n:]


def intact(tail):
    torch.cuda.synchronize()
    return T.guard_intact(tail.float().cpu().numpy() if tail.is_floating_point() else tail.cpu().numpy(), integer=not tail.is_floating_point())


# ---------------------------------------------------------------------------------------------------------------------
# 1. the candidates kernel
# ---------------------------------------------------------------------------------------------------------------------
CAND_CASES = [(1, 8, 4, False), (1, 8, 4, True), (37, 8, 5, False), (37, 8, 5, True), (300, 252, 33, False),
              (4096, 64, 40, False), (4096, 64, 40, True), (1000, 516, 1000, False), (257, 520, 1000, True)]     # (N, C, K, bf16 rows)


def _run_candidates(shards, t, k, bf16):
    from vq_seg_amd import _hip
    world, (n, c) = len(shards), shards[0].shape
    counter = torch.tensor(t, dtype=torch.int64, device=dev())
    total_c, total_o, want_c, want_o = None, None, None, None
    for rank, shard in enumerate(shards):
        x = torch.tensor(shard).to(dev())
        x = x.to(BF16) if bf16 else x                                      # the values are bf16-exact: the cast keeps them (NaN -> NaN)
        (cand, gc), (okf, go) = guarded(k * c), guarded(k)
        _hip.vq_revive_candidates(x, SEED, counter, k, rank, world, out=(cand.view(k, c), okf))
        assert intact(gc) and intact(go), "the guard elements behind cand / ok were written"
        wc, wo = RC.candidates(shard, SEED, t, k, rank, world)
        assert (bits(cand).reshape(k, c) == T.f32_bits(wc)).all(), f"rank {rank} of {world}, t {t}: cand differs from the picked rows"
        assert (bits(okf) == T.f32_bits(wo)).all(), f"rank {rank} of {world}, t {t}: ok differs"
        total_c, total_o = (cand.clone(), okf.clone()) if rank == 0 else (total_c + cand, total_o + okf)           # what the all-reduce forms
        want_c, want_o = (wc, wo) if rank == 0 else (want_c + wc, want_o + wo)
    assert int(counter) == t, "the candidates kernel must not move the counter"
    assert (bits(total_c).reshape(k, c) == T.f32_bits(want_c)).all() and (bits(total_o) == T.f32_bits(want_o)).all()
    return want_o


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("n,c,k,bf16", CAND_CASES, ids=[f"{n}x{c}-K{k}-{'bf16' if b else 'f32'}" for n, c, k, b in CAND_CASES])
def test_candidates_are_the_hashed_rows_bit_for_bit(n, c, k, bf16, world):
    """vqseg_vq_revive_candidates once per rank on that rank's shard, at counter values 0 and 3: cand and ok bit-equal to the
    restatement on every rank, and their sum over ranks (what the all-reduce forms) too.  Then one NaN and one Inf planted at rows
    the hash selects: those codes' ok is 0."""
    rows = T.bf16_exact(T.uniform(9000 + n + c + world, (world * n, c), -4.0, 4.0))
    shards = [rows[r * n:(r + 1) * n] for r in range(world)]
    for t in (0, 3):
        ok_sum = _run_candidates(shards, t, k, bf16)
        assert (ok_sum == 1).all()                                         # finite rows: every code has exactly one owner
    t = 3
    rank = RC.pick(SEED, t, k - 1, n, world)[0]                            # a rank that owns at least one candidate
    hit = RC.picked_rows(n, SEED, t, k, rank, world)
    planted = np.array(rows)
    own = planted[rank * n:(rank + 1) * n]
    own[hit[0], c - 1] = np.nan
    own[hit[-1], 0] = -np.inf
    ok_sum = _run_candidates([planted[r * n:(r + 1) * n] for r in range(world)], t, k, bf16)
    bad = [kk for kk in range(k) if RC.pick(SEED, t, kk, n, world) in ((rank, hit[0]), (rank, hit[-1]))]
    assert bad and (ok_sum[bad] == 0).all() and (np.delete(ok_sum, bad) == 1).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the update kernel
# ---------------------------------------------------------------------------------------------------------------------
def _update(k, c, decay, tau, scenario, raw=False, **kw):
    """one _hip.vq_ema_update call on the fixture's state (raw: vqseg_vq_ema_update_f32 itself, through the C ABI)
    -> (cluster_size, embed_avg, codebook) NumPy, guards checked"""
    from vq_seg_amd import _hip
    _, _, counts, sums, cs, avg, _, _ = RC.update_inputs(k, c, scenario)
    (d_cs, g1), (d_avg, g2), (d_cb, g3) = guarded(k), guarded(k * c), guarded(k * c)
    d_cs.copy_(torch.tensor(cs))
    d_avg.copy_(torch.tensor(avg).reshape(-1))
    d_sums, d_counts = torch.tensor(sums).to(dev()), torch.tensor(counts).to(dev())
    if raw:
        total = torch.empty(1, device=dev())
        rc = _hip.lib().vqseg_vq_ema_update_f32(d_cs.data_ptr(), d_avg.data_ptr(), d_cb.data_ptr(), d_sums.data_ptr(), d_counts.data_ptr(), c, k,
                                                decay, T.EMA_EPS, total.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, _hip.lib().vqseg_last_error()
    else:
        _hip.vq_ema_update(d_cs, d_avg.view(k, c), d_cb.view(k, c), d_sums, d_counts, decay, T.EMA_EPS, **kw)
    assert intact(g1) and intact(g2) and intact(g3), "the guard elements behind an output were written"
    return d_cs.cpu().numpy(), d_avg.view(k, c).cpu().numpy(), d_cb.view(k, c).cpu().numpy()


@pytest.mark.parametrize("scenario", RC.SCENARIOS)
@pytest.mark.parametrize("tau", RC.TAUS)
@pytest.mark.parametrize("k,c,decay", RC.UPDATE_CASES)
def test_update_revives_expired_codes_and_keeps_the_rest_bit_for_bit(k, c, decay, tau, scenario):
    """vqseg_vq_ema_update_revive_f32 with none, about a fifth and all of the codes expiring.  Revived codes: codebook = the candidate,
    embed_avg = float32(candidate) * float32(tau), cluster_size = tau, all bit for bit; `revived` = the restated count; the counter
    advanced by one.  Every other entry: torch.equal with what vqseg_vq_ema_update_f32 writes from the same inputs, and within
    T.ema_reference's counted bars of the float64 restatement.  The fixture keeps every updated count a relative 1e-4 away from tau
    (asserted in RC.revive_reference), so no code is left out."""
    exp, bars = RC.revive_reference(k, c, decay, tau, scenario)
    *_, cand, okf = RC.update_inputs(k, c, scenario)
    rv = exp["revived"]
    old = dict(zip(("cluster_size", "embed_avg", "codebook"), _update(k, c, decay, tau, scenario, raw=True)))
    for kw in (dict(), dict(threshold=0.0)):
        also_old = _update(k, c, decay, tau, scenario, **kw)
        assert all((T.f32_bits(a) == T.f32_bits(b)).all() for a, b in zip(old.values(), also_old)), "threshold = 0 must be today's call"
    counter, (revived, gr) = torch.tensor(5, dtype=torch.int64, device=dev()), guarded(1, torch.int64)
    new = dict(zip(old, _update(k, c, decay, tau, scenario, candidates=torch.tensor(cand).to(dev()), ok=torch.tensor(okf).to(dev()),
                                threshold=tau, counter=counter, revived=revived)))
    assert intact(gr)
    assert int(revived) == int(rv.sum()), f"revived {int(revived)} against the restated {int(rv.sum())}"
    assert int(counter) == 6, "the counter must advance by exactly one"
    print(f"[revive] K {k} C {c} decay {decay} tau {tau} {scenario}: {int(rv.sum())} of {k} revived, "
          f"{int(((bars['cluster_size'][0] < tau) & ~rv).sum())} expired with an unusable candidate")
    tau32 = np.float32(tau)
    assert (T.f32_bits(new["cluster_size"][rv]) == T.f32_bits(tau32)).all()
    assert (T.f32_bits(new["codebook"][rv]) == T.f32_bits(cand[rv])).all()
    assert (T.f32_bits(new["embed_avg"][rv]) == T.f32_bits(cand[rv] * tau32)).all()
    assert (new["cluster_size"][okf > 0] >= tau32).all()                    # the invariant of the rule
    for name in old:
        assert torch.equal(torch.tensor(new[name][~rv]), torch.tensor(old[name][~rv])), f"{name}: a code that was not revived differs from today's update"
        ref, bound = bars[name]
        err = np.abs(new[name][~rv].astype(np.float64) - ref[~rv])
        if err.size:
            worst = float((err / np.maximum(bound[~rv], 1e-300)).max())
            T.note("revive", f"K {k} C {c} decay {decay} tau {tau} {scenario} {name}", worst, 1.0)
            assert (err <= bound[~rv]).all(), f"{name}: off by {worst:.3g} of its counted bar"
        assert (new[name][rv].astype(np.float64) == exp[name][rv]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the module
# ---------------------------------------------------------------------------------------------------------------------
TAU, DECAY, EPS = 2.0, 0.9, 1e-5


def _module(tau=TAU, ema=True, **kw):
    """the issue's module on a spread-out codebook; half of the codes start with a moving count of 0 (they expire), half with 100"""
    from vq_seg_amd.vector_quantizer import VectorQuantizer
    if tau is not None:
        kw["threshold_ema_dead_code"] = tau
    vq = VectorQuantizer(dim=64, num_embeddings=40, decay=DECAY, eps=EPS, ema_update=ema, **kw).to(dev())
    W = synth.relu_features(10, (40, 64)).to(dev())
    with torch.no_grad():
        vq.codebook.embedding.weight.copy_(W)
        if ema:
            vq.codebook.embed_avg.copy_(W)
            vq.codebook.cluster_size.copy_(torch.tensor([0.0, 100.0] * 20))
    return vq.train()


def _x(step, amp):
    x = synth.relu_features(90 + step, (2, 64, 8, 8)).to(dev())
    return x.bfloat16() if amp else x


def _forward(vq, x, amp, grad=None):
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
        q, idx, loss, dead = vq(x)
    if grad is not None:
        ((q.float() * grad).sum() + 0.5 * loss.sum()).backward()
    return q, idx, loss, dead


def _state(vq):
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in vq.state_dict().items()}


def _same(a, b):
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16-autocast"])
def test_module_revives_expired_codes_from_the_batch(amp):
    """One training forward of VectorQuantizer(..., ema_update=True, threshold_ema_dead_code=2.0): the output and the input gradient are
    those of the codebook BEFORE the move (the frozen module's); every code the restatement marks expired is then the restated input row
    bit for bit; everything else is the threshold-0 module's update; the next forward quantises with the revived codes; an eval forward
    changes nothing.  (On the parent commit the keyword is a TypeError.)"""
    from vq_seg_amd import _hip
    g = synth.uniform(11, (2, 64, 8, 8), -1, 1).to(dev())
    runs = {}
    for name, vq in (("frozen", _module(None, ema=False)), ("ema", _module(0.0)), ("revive", _module(TAU, revive_seed=77))):
        x = _x(0, amp).clone().requires_grad_(True)
        before = _state(vq)
        q, idx, loss, _ = _forward(vq, x, amp, g)
        runs[name] = (vq, before, q, idx, loss, x.grad)
    vq, before, q, idx, loss, gx = runs["revive"]
    for other in ("frozen", "ema"):
        _, _, q0, idx0, loss0, gx0 = runs[other]
        assert torch.equal(q, q0) and torch.equal(idx, idx0) and torch.equal(loss, loss0) and torch.equal(gx, gx0), other
    rows = _x(0, amp).float().permute(0, 2, 3, 1).reshape(-1, 64).cpu().numpy()
    exp = RC.module_step_reference(before["codebook.cluster_size"].cpu().numpy(), before["codebook.embed_avg"].cpu().numpy(), [rows],
                                   idx.reshape(-1).cpu().numpy(), DECAY, EPS, TAU, 77, 0)
    rv = exp["revived"]
    assert 0 < rv.sum() < 40, "the fixture must revive some codes and keep some"
    cb, after, plain = vq.codebook, _state(vq), _state(runs["ema"][0])
    assert int(cb.revived) == int(rv.sum()) and int(cb.ema_updates) == 1
    for name in ("cluster_size", "embed_avg"):
        got = after[f"codebook.{name}"].cpu().numpy()
        assert (T.f32_bits(got[rv]) == T.f32_bits(exp[name][rv].astype(np.float32))).all(), name
        assert (T.f32_bits(got[~rv]) == T.f32_bits(plain[f"codebook.{name}"].cpu().numpy()[~rv])).all(), name
    w = after["codebook.embedding.weight"].cpu().numpy()
    picked = np.stack([rows[RC.pick(77, 0, k, rows.shape[0], 1)[1]] for k in range(40)])
    assert (T.f32_bits(w[rv]) == T.f32_bits(picked[rv])).all(), "a revived code is not its input row bit for bit"
    assert (T.f32_bits(w[~rv]) == T.f32_bits(plain["codebook.embedding.weight"].cpu().numpy()[~rv])).all()
    assert (after["codebook.cluster_size"] >= TAU).all()
    # the prepared image of the old codebook is retired: the next (eval) forward assigns with the revived codes, and moves nothing
    vq.eval()
    with torch.no_grad():
        _, idx2, _, _ = _forward(vq, _x(1, amp), amp)
    rows2 = _x(1, amp).permute(0, 2, 3, 1).reshape(-1, 64).contiguous()
    assert torch.equal(idx2.reshape(-1), _hip.vq_assign(rows2, after["codebook.embedding.weight"]))
    assert not torch.equal(idx2.reshape(-1), _hip.vq_assign(rows2, before["codebook.embedding.weight"])), "the fixture cannot tell the two codebooks apart"
    assert _same(_state(vq), after), "an eval forward must neither update nor revive"


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16-autocast"])
def test_module_resume_and_threshold_zero(amp):
    """Four steps straight through == two steps, state_dict into a fresh module, two more (the counter travels as a buffer: the hash
    picks the same rows); ema_update=True with threshold 0 is bit-identical to a module built without the keyword."""
    straight = _module(TAU, revive_seed=5)
    for step in range(4):
        _forward(straight, _x(step, amp), amp)
    first = _module(TAU, revive_seed=5)
    for step in range(2):
        _forward(first, _x(step, amp), amp)
    from vq_seg_amd.vector_quantizer import VectorQuantizer
    second = VectorQuantizer(dim=64, num_embeddings=40, decay=DECAY, eps=EPS, ema_update=True, threshold_ema_dead_code=TAU, revive_seed=5).to(dev())
    second.load_state_dict(_state(first))
    second.train()
    for step in range(2, 4):
        _forward(second, _x(step, amp), amp)
    assert int(straight.codebook.ema_updates) == 4 and _same(_state(straight), _state(second))
    zero, without = _module(0.0), _module(None)
    for step in range(2):
        _forward(zero, _x(step, amp), amp)
        _forward(without, _x(step, amp), amp)
    assert "codebook.ema_updates" not in _state(zero) and _same(_state(zero), _state(without))


# ---------------------------------------------------------------------------------------------------------------------
# 4. the trainer
# ---------------------------------------------------------------------------------------------------------------------
def test_cps_steps_keep_every_moving_count_at_the_threshold_and_checkpoint_the_counter(tmp_path):
    from vq_seg_amd.trainer import CPSConfig, CPSTrainer, SyntheticCropWeed
    d = torch.device("cuda:0")
    model = {"name": "vqreptunet1x1", "params": {"encoder_name": "resnet50", "num_classes": 3, "depth": 5,
                                                 "vq_cfg": {"num_embeddings": [0, 0, 64, 64, 64], "distance": "euclidean", "kmeans_init": True,
                                                            "ema_update": True, "threshold_ema_dead_code": 1.0},
                                                 "margin": 0.0, "scale": 1.0, "use_feature": False, "encoder_weights": None}}
    make = lambda: CPSTrainer(CPSConfig(model=model, recipe="v1", total_iters=10, amp_dtype=torch.bfloat16), d)
    torch.manual_seed(0)
    tr = make()
    data = SyntheticCropWeed(64, 2, d, seed=5)
    books = [m.codebook[i].codebook for m in tr.models for i in (2, 3, 4)]
    for _ in range(3):
        (l_in, l_tg), ul_in = data.labelled(), data.unlabelled()
        out = tr.step(l_in, l_tg, ul_in)
        assert all(bool(torch.isfinite(v).all()) for v in out.values()), out
        for cb in books:
            assert torch.isfinite(cb.embedding.weight).all() and (cb.cluster_size >= 1.0).all()
    counters = [int(cb.ema_updates) for cb in books]
    assert all(n >= 3 for n in counters), counters
    path = str(tmp_path / "revive.pt")
    tr.save_checkpoint(path)
    torch.manual_seed(1)
    other = make()
    assert all(int(m.codebook[i].codebook.ema_updates) == 0 for m in other.models for i in (2, 3, 4))
    other.load_checkpoint(path)
    assert [int(m.codebook[i].codebook.ema_updates) for m in other.models for i in (2, 3, 4)] == counters
    for a, b in zip(tr.models, other.models):
        assert all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))


# ---------------------------------------------------------------------------------------------------------------------
# 5. data parallel
# ---------------------------------------------------------------------------------------------------------------------
def _dp_inputs(rank, step):
    """multiples of 1/64 in [0, 1]: a code's fp32 sum over at most 256 such rows is exact, so it does not depend on the order or on
    which rank added what -- the only thing an all-reduce of per-rank sums could change against one process on all rows"""
    return torch.tensor(np.random.RandomState(500 + 10 * step + rank).randint(0, 65, size=(2, 64, 8, 8)) / 64.0, dtype=torch.float32).cuda()


def _dp_module(tau):
    from vq_seg_amd.vector_quantizer import VectorQuantizer
    vq = VectorQuantizer(dim=64, num_embeddings=40, decay=DECAY, eps=EPS, ema_update=True, threshold_ema_dead_code=tau, revive_seed=9).cuda()
    W = torch.tensor(np.random.RandomState(499).randint(0, 65, size=(40, 64)) / 64.0, dtype=torch.float32).cuda()
    with torch.no_grad():
        vq.codebook.embedding.weight.copy_(W)
        vq.codebook.embed_avg.copy_(W)
        vq.codebook.cluster_size.fill_(1.0)
    return vq.train()


def _dp_job(rank, world):
    from vq_seg_amd.vector_quantizer import vq_img
    torch.cuda.set_device(0)
    calls, real = [], vq_img._all_reduce_sum

    def spy(t):
        calls.append(t.numel())
        return real(t)

    vq_img._all_reduce_sum = spy
    per_step = {}
    try:
        for tau in (TAU, 0.0):
            vq = _dp_module(tau)
            per_step[tau] = []
            for step in range(3):
                del calls[:]
                vq(_dp_inputs(rank, step))
                per_step[tau].append(len(calls))
            if tau:
                torch.cuda.synchronize()
                state = {k: v.detach().cpu() for k, v in vq.state_dict().items()}
                revived = int(vq.codebook.revived)
    finally:
        vq_img._all_reduce_sum = real
    return state, per_step, revived


def test_two_ranks_revive_what_one_process_on_both_shards_revives():
    """Two ranks (one GPU, gloo standing in for RCCL as in tests/test_dp_gpu.py), three updates: codebook, embed_avg, cluster_size and
    ema_updates identical across ranks and torch.equal to one process on the concatenated batches; as many all-reduces per EMA step
    as with threshold 0 (the candidates travel in the message of the sums)."""
    out = spawn(_dp_job)
    (s0, n0, r0), (s1, n1, r1) = out
    assert list(s0) == ["codebook.cluster_size", "codebook.embed_avg", "codebook.ema_updates", "codebook.embedding.weight"]
    assert all(torch.equal(s0[k], s1[k]) for k in s0) and r0 == r1
    assert n0 == n1 and n0[TAU] == n0[0.0] == [2, 2, 2], n0
    vq = _dp_module(TAU)
    total = 0
    for step in range(3):
        vq(torch.cat([_dp_inputs(0, step), _dp_inputs(1, step)], dim=0))
        total += int(vq.codebook.revived)
    assert total > 0, "the fixture revived nothing"
    one = {k: v.detach().cpu() for k, v in vq.state_dict().items()}
    assert int(one["codebook.ema_updates"]) == 3
    for k in s0:
        assert torch.equal(s0[k], one[k]), f"{k}: two ranks differ from one process on the concatenated batches"
