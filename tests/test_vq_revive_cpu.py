"""Dead-code revival of the EMA codebook, everything that needs no GPU: the known answers of the candidate hash, the constructor
contracts, the state_dict layout, the argument validation of the two entry points, and the facts the GPU fixtures of
tests/vq_revive_cases.py rest on (no updated moving count near the threshold; none / some / all codes expire)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import vq_revive_cases as RC
from vq_seg_amd import _hip
from vq_seg_amd.vector_quantizer import VectorQuantizer, make_vq_module


@pytest.mark.parametrize("args,h,where", RC.KNOWN, ids=[str(i) for i in range(len(RC.KNOWN))])
def test_hash_known_answers(args, h, where):
    assert RC.revive_hash(*args) == h
    assert RC.pick(*args, n=300, world=2) == where
    g = h % 600                                                       # world = 1 on the concatenated rows picks the same row
    assert RC.pick(*args, n=600, world=1) == (0, g) and g == where[0] * 300 + where[1]


def test_candidates_restatement_adds_up_over_ranks_to_the_single_process_pick():
    rows = RC.T.uniform(1, (3 * 37, 8))
    whole, ok = RC.candidates(rows, 42, 3, 50, 0, 1)
    parts = [RC.candidates(rows[r * 37:(r + 1) * 37], 42, 3, 50, r, 3) for r in range(3)]
    assert (sum(p[0] for p in parts) == whole).all() and (sum(p[1] for p in parts) == ok).all() and (ok == 1).all()
    assert (np.stack([p[1] for p in parts]).sum(0) == 1).all()         # exactly one owner per code
    assert sorted(RC.picked_rows(37, 42, 3, 50, 1, 3)) == sorted(j for o, j in (RC.pick(42, 3, k, 37, 3) for k in range(50)) if o == 1)


def test_constructor_contracts():
    with pytest.raises(ValueError, match="ema_update=True"):
        VectorQuantizer(dim=8, num_embeddings=4, threshold_ema_dead_code=2.0)
    with pytest.raises(ValueError, match=">= 0"):
        VectorQuantizer(dim=8, num_embeddings=4, ema_update=True, threshold_ema_dead_code=-1.0)
    with pytest.raises(ValueError, match=">= 0"):
        VectorQuantizer(dim=8, num_embeddings=4, threshold_ema_dead_code=-1.0)
    vq = VectorQuantizer(dim=8, num_embeddings=4, ema_update=True, threshold_ema_dead_code=2.0, revive_seed=7)
    assert vq.codebook.threshold_ema_dead_code == 2.0 and vq.codebook.revive_seed == 7 and vq.codebook.revived is None
    assert vq.codebook.ema_updates.dtype == torch.int64 and vq.codebook.ema_updates.shape == () and int(vq.codebook.ema_updates) == 0


def test_state_dict_gains_the_counter_only_with_a_threshold():
    plain = ["codebook.embedding.weight"]
    ema = ["codebook.cluster_size", "codebook.embed_avg"] + plain       # a module's own buffers come before its submodules' entries
    assert list(VectorQuantizer(dim=8, num_embeddings=4).state_dict()) == plain
    assert list(VectorQuantizer(dim=8, num_embeddings=4, ema_update=True).state_dict()) == ema
    assert list(VectorQuantizer(dim=8, num_embeddings=4, ema_update=True, threshold_ema_dead_code=0.0).state_dict()) == ema
    assert list(VectorQuantizer(dim=8, num_embeddings=4, ema_update=True, threshold_ema_dead_code=2.0).state_dict()) == ema[:2] + ["codebook.ema_updates"] + plain
    mods = make_vq_module({"num_embeddings": [0, 0, 16, 16, 16], "ema_update": True, "threshold_ema_dead_code": 2.0, "revive_seed": 3},
                          (3, 64, 256, 512, 1024, 2048), 5)
    assert all(m.codebook.threshold_ema_dead_code == 2.0 and m.codebook.revive_seed == 3 for m in list(mods)[2:])
    assert [k for k in mods.state_dict() if k.endswith("ema_updates")] == [f"{i}.codebook.ema_updates" for i in (2, 3, 4)]


def test_entry_points_validate_their_arguments_without_a_device():
    L = _hip.lib()
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) & ~15                               # a 16-byte aligned host address: never dereferenced by the checks
    cands = lambda bf, n, c, k, rank, world, x=p: L.vqseg_vq_revive_candidates(bf, x, n, c, k, 5, p, rank, world, p, p, None)
    for bad in (dict(x=None),):
        assert cands(0, 8, 8, 4, 0, 1, **bad) == -1 and b"null pointer" in L.vqseg_last_error()
    assert L.vqseg_vq_revive_candidates(0, p, 8, 8, 4, 5, None, 0, 1, p, p, None) == -1 and b"null pointer" in L.vqseg_last_error()
    assert L.vqseg_vq_revive_candidates(0, p, 8, 8, 4, 5, p, 0, 1, None, p, None) == -1 and b"null pointer" in L.vqseg_last_error()
    assert L.vqseg_vq_revive_candidates(0, p, 8, 8, 4, 5, p, 0, 1, p, None, None) == -1 and b"null pointer" in L.vqseg_last_error()
    assert cands(0, 0, 8, 4, 0, 1) == -1 and b"n_rows and n_codes must be positive" in L.vqseg_last_error()
    assert cands(0, 8, 8, 0, 0, 1) == -1 and b"n_rows and n_codes must be positive" in L.vqseg_last_error()
    assert cands(0, 8, 8, 4, 0, 0) == -1 and b"world must be >= 1" in L.vqseg_last_error()
    assert cands(0, 8, 8, 4, 2, 2) == -1 and b"rank 2 outside [0, 2)" in L.vqseg_last_error()
    assert cands(0, 8, 8, 4, -1, 2) == -1 and b"rank -1 outside [0, 2)" in L.vqseg_last_error()
    assert cands(0, 8, 6, 4, 0, 1) == -1 and b"multiple of 4" in L.vqseg_last_error()            # the assign entry points' messages
    assert cands(1, 8, 6, 4, 0, 1) == -1 and b"multiple of 4" in L.vqseg_last_error()
    assert cands(1, 8, 12, 4, 0, 1) == -1 and b"channels % 8 == 0" in L.vqseg_last_error()
    assert cands(0, 8, 8, 4, 0, 1, x=p + 4) == -1 and b"16-byte aligned" in L.vqseg_last_error()

    def update(cand=p, ok=p, tau=2.0, counter=p, revived=p, c=8, k=4, decay=0.8, cs=p):
        return L.vqseg_vq_ema_update_revive_f32(cs, p, p, p, p, c, k, decay, 1e-5, p, cand, ok, tau, counter, revived, None)
    assert update(cs=None) == -1 and b"bad argument" in L.vqseg_last_error()                    # today's checks, today's messages
    assert update(c=0) == -1 and b"bad argument" in L.vqseg_last_error()
    assert update(decay=1.5) == -1 and b"0 <= decay <= 1" in L.vqseg_last_error()
    for kw in (dict(cand=None), dict(ok=None), dict(counter=None), dict(revived=None)):
        assert update(**kw) == -1 and b"ema update with revival: null pointer" in L.vqseg_last_error()
    for tau in (-1.0, float("nan"), float("inf")):
        assert update(tau=tau) == -1 and b"finite threshold >= 0" in L.vqseg_last_error()


def test_wrappers_refuse_wrong_types_before_touching_a_device():
    E = _hip.HipLibraryError
    z = torch.zeros
    with pytest.raises(E, match="counter: expected torch.int64"):
        _hip.vq_revive_candidates(z(8, 16), 0, z(1, dtype=torch.int32), 4, 0, 1)
    with pytest.raises(E, match="rows: expected torch.float32 or torch.bfloat16"):
        _hip.vq_revive_candidates(z(8, 16, dtype=torch.float16), 0, z((), dtype=torch.int64), 4, 0, 1)
    with pytest.raises(E, match="candidates: the sizes passed along need 64"):
        _hip.vq_revive_candidates(z(8, 16), 0, z((), dtype=torch.int64), 4, 0, 1, out=(z(4, 8), z(4)))
    with pytest.raises(E, match="out: the sizes passed along need 64"):
        _hip.vq_code_sums(z(8, 16), z(8, dtype=torch.int64), 4, out=z(4, 8))
    args = (z(4), z(4, 16), z(4, 16), z(4, 16), z(4, dtype=torch.int64), 0.9, 1e-5)
    with pytest.raises(E, match="revived: expected torch.int64"):
        _hip.vq_ema_update(*args, candidates=z(4, 16), ok=z(4), threshold=2.0, counter=z((), dtype=torch.int64), revived=z(()))
    with pytest.raises(E, match="candidates: expected a tensor, got None"):
        _hip.vq_ema_update(*args, threshold=2.0)
    with pytest.raises(E, match="no CPU fallback"):
        _hip.vq_ema_update(*args, candidates=z(4, 16), ok=z(4), threshold=2.0, counter=z((), dtype=torch.int64), revived=z((), dtype=torch.int64))


@pytest.mark.parametrize("k,c,decay", RC.UPDATE_CASES)
def test_update_fixtures_keep_every_count_away_from_the_threshold_and_cover_none_some_all(k, c, decay):
    for tau in RC.TAUS:
        share = {}
        for scenario in RC.SCENARIOS:
            exp, bars = RC.revive_reference(k, c, decay, tau, scenario)              # asserts the 1e-4 margin itself
            *_, ok = RC.update_inputs(k, c, scenario)
            expired = bars["cluster_size"][0] < tau
            assert (exp["revived"] == (expired & (ok > 0))).all()
            assert (exp["cluster_size"][(ok > 0)] >= tau).all()                       # the invariant of the rule
            share[scenario] = expired.mean()
            if scenario == "fifth":
                assert exp["revived"].any(), "no code revived"
                assert k < 33 or (expired & ~exp["revived"]).any(), "no expired code with an unusable candidate"
                assert k < 33 or tau < 2.0 or abs(share[scenario] - 0.2) <= 0.02, share
        assert share["none"] == 0.0 and share["all"] == 1.0 and 0.0 < share["fifth"] < 1.0, share
