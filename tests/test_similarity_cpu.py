"""The similarity transforms without a GPU: the matrices, the float64 restatement of the warp against torch's own affine_grid +
grid_sample, the CPU path of similarity_transform / inverse_similarity_transform / warp_batch (exact cases, a ramp image, round
trips, labels), the order of the draws, step_transforms, the CPSConfig fields, the argument checks of _hip.affine_warp and of
the entry point with the library loaded, and the reference trainer's import through compat/."""
import os
import random
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import synth, warp_cases as W
from vq_seg_amd import _hip
from vq_seg_amd.data import (inverse_similarity_transform, similarity_matrices, similarity_transform, step_transforms, warp_batch)
from vq_seg_amd.data import augmentations as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def m2(row):
    return np.array([[row[0], row[1]], [row[3], row[4]]], dtype=np.float64)


def test_matrices_are_exact_at_quarter_turns_and_invert():
    want = {0.0: [1, 0, 0, 0, 1, 0], 90.0: [0, -1, 0, 1, 0, 0], 180.0: [-1, 0, 0, 0, -1, 0], 270.0: [0, 1, 0, -1, 0, 0], -90.0: [0, 1, 0, -1, 0, 0],
            360.0: [1, 0, 0, 0, 1, 0]}
    for a, row in want.items():
        got = similarity_matrices([3], [a])
        assert got.dtype == np.float32 and got.shape == (1, 6) and got[0].tolist() == [float(v) for v in row], (a, got)
    assert similarity_matrices([1], [0.0])[0].tolist() == [-1, 0, 0, 0, 1, 0] and similarity_matrices([2], [0.0])[0].tolist() == [1, 0, 0, 0, -1, 0]
    assert similarity_matrices([5], [90.0])[0].tolist() == [0, 1, 0, 1, 0, 0]                     # F_h R(90)
    for c in range(10):
        for a in (0.0, 17.3, -33.7, 90.0, 123.4, 180.0, 270.0):
            f, b = similarity_matrices([c], [a]), similarity_matrices([c], [a], inverse=True)
            assert (f[:, (2, 5)] == 0).all() and (b[:, (2, 5)] == 0).all()
            assert np.abs(m2(b[0]) @ m2(f[0]) - np.eye(2)).max() <= 1e-6 and np.abs(m2(f[0]) @ m2(b[0]) - np.eye(2)).max() <= 1e-6, (c, a)
            if c in (0, 9):
                assert f[0].tolist() == [1, 0, 0, 0, 1, 0] and b[0].tolist() == [1, 0, 0, 0, 1, 0]
    a = np.deg2rad(17.3)                                                    # a pure rotation samples xs = cos a dx - sin a dy, ys = sin a dx + cos a dy
    assert np.allclose(m2(similarity_matrices([3], [17.3])[0]), [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]], atol=1e-7)
    assert np.array_equal(similarity_matrices([4], [-17.3]), similarity_matrices([3], [-17.3]))   # the angle is signed; the code does not sign it again
    assert similarity_matrices([3, 1], [10.0, 0.0]).shape == (2, 6)
    for bad in (([10], [0.0]), ([-1], [0.0]), ([3, 3], [1.0]), ([3], [float("nan")])):
        with pytest.raises(ValueError):
            similarity_matrices(*bad)


@pytest.mark.parametrize("h,w", [(16, 16), (33, 20)])
def test_restatement_equals_affine_grid_and_grid_sample(h, w):
    src = synth.uniform(7, (2, 3, h, w), -1.0, 1.0).double()
    for flip in (None, "h", "v"):
        for angle in W.ANGLES + [90.0, 45.0]:
            mats = W.matrices(angle, flip, 2)
            m = mats.astype(np.float64)
            theta = torch.tensor([[[r[0], r[1] * h / w, 0.0], [r[3] * w / h, r[4], 0.0]] for r in m], dtype=torch.float64)
            grid = F.affine_grid(theta, (2, 3, h, w), align_corners=False)
            want = F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=False).numpy()
            assert np.abs(W.bilinear(src.numpy(), mats) - want).max() <= 1e-9, (flip, angle)


def test_cpu_path_exact_cases_pass_every_bit():
    t = synth.uniform(3, (2, 3, 16, 16), -1.0, 1.0)
    t[0, 0, 2, 3], t[1, 2, 5, 0], t[0, 1, 0, 0] = float("nan"), -0.0, float("inf")
    bits = lambda x: x.view(torch.int32)                                    # noqa: E731
    out, aug, angle = similarity_transform(t, 1)
    assert (aug, angle) == (1, 0.0) and torch.equal(bits(out), bits(t.flip(-1)))
    out, aug, angle = similarity_transform(t, 2)
    assert (aug, angle) == (2, 0.0) and torch.equal(bits(out), bits(t.flip(-2)))
    quarter = warp_batch(t, similarity_matrices([3, 3], [90.0, 90.0]))
    assert torch.equal(bits(quarter), bits(torch.rot90(t, 1, (-2, -1))))
    assert torch.equal(bits(warp_batch(t, similarity_matrices([0, 9], [12.0, 34.0]))), bits(t))
    u = synth.uniform(4, (2, 3, 5, 7), -1.0, 1.0)                           # non-square: half turn = both flips
    assert torch.equal(warp_batch(u, similarity_matrices([3, 3], [180.0, 180.0])), u.flip(-1, -2))
    b = u.bfloat16()
    assert torch.equal(warp_batch(b, similarity_matrices([1, 2], [0.0, 0.0])), torch.stack([b[0].flip(-1), b[1].flip(-2)]))


def test_cpu_path_reproduces_a_ramp_under_rotation():
    h, w = 33, 20
    x, y = torch.arange(w, dtype=torch.float64)[None, :], torch.arange(h, dtype=torch.float64)[:, None]
    img = (0.3 * x - 0.2 * y + 0.1).float()[None, None]
    mats = similarity_matrices([3], [17.3])
    out = warp_batch(img, mats).double().numpy()[0, 0]
    xs, ys = (v[0] for v in W.coords(mats, h, w))
    inside = (np.floor(xs) >= 0) & (np.floor(xs) + 1 <= w - 1) & (np.floor(ys) >= 0) & (np.floor(ys) + 1 <= h - 1)
    assert inside.sum() > 0.5 * h * w
    want = 0.3 * xs - 0.2 * ys + 0.1                                        # bilinear interpolation reproduces a linear image
    assert np.abs(out - want)[inside].max() <= W.tol_f32(img.numpy(), h, w)
    assert np.abs(out - W.bilinear(img.numpy(), mats)[0, 0]).max() <= W.tol_f32(img.numpy(), h, w)      # the padded border too


def test_round_trips_are_exact_for_flips_and_quarter_turns():
    t = synth.uniform(5, (2, 3, 16, 16), -1.0, 1.0)
    for code in (1, 2):
        out, aug, angle = similarity_transform(t, code)
        assert torch.equal(inverse_similarity_transform(out, aug, angle), t)
    for code in (3, 4, 5, 6, 7, 8):
        for angle in (90.0, -90.0, 180.0, 270.0):
            fwd = warp_batch(t, similarity_matrices([code] * 2, [angle] * 2))
            assert torch.equal(inverse_similarity_transform(fwd, code, angle), t), (code, angle)
    for code in (0, 9):
        out, aug, angle = similarity_transform(t, code)
        assert angle == 0.0 and torch.equal(out, t) and torch.equal(inverse_similarity_transform(out, aug, angle), t)
    single = t[0, 0]                                                        # a bare (H, W) map
    assert torch.equal(similarity_transform(single, 1)[0], single.flip(-1))


def test_integer_labels_take_the_nearest_pixel():
    lab = torch.zeros(1, 24, 24, dtype=torch.int64)
    lab[:, :, 12:] = 2
    back = inverse_similarity_transform(lab, 3, 30.0)
    assert back.dtype == torch.int64 and set(back.unique().tolist()) == {0, 2}                   # no invented class 1
    filled = inverse_similarity_transform(lab, 3, 30.0, fill=255)
    assert set(filled.unique().tolist()) == {0, 2, 255} and filled[0, 0, 0] == 255 and torch.equal(filled == 255, (filled != back))
    fwd, aug, angle = similarity_transform(lab.to(torch.uint8), 4)
    assert fwd.dtype == torch.uint8 and angle < 0 and set(fwd.unique().tolist()) <= {0, 2}
    want, decided = W.nearest(lab.numpy()[:, None], similarity_matrices([3], [30.0], inverse=True), 255)
    assert np.array_equal(filled.numpy()[:, None][decided], want[decided]) and decided.mean() > 0.99
    with pytest.raises(ValueError, match="floating"):
        warp_batch(lab, similarity_matrices([3], [30.0]), mode="bilinear")


def test_draws_are_the_references_in_its_order():
    t = torch.zeros(1, 1, 4, 4)
    seen = set()
    for seed in range(16):
        random.seed(seed), torch.manual_seed(seed)
        code = random.randint(0, 9)
        py_after = random.getstate()
        t_before = torch.get_rng_state()
        drawn = float(torch.empty(1).uniform_(0.0, 90.0).item())
        t_after = torch.get_rng_state()
        assert not torch.equal(t_before, t_after)
        random.seed(seed), torch.manual_seed(seed)
        _out, aug, angle = similarity_transform(t)
        seen.add(aug)
        assert aug == code and random.getstate() == py_after                # exactly one randint(0, 9)
        assert torch.equal(torch.get_rng_state(), t_before if code in (1, 2) else t_after)      # one uniform_(0, 90), none for the flips
        assert angle == (drawn if code in (3, 5, 7) else -drawn if code in (4, 6, 8) else 0.0)
    assert seen & {1, 2} and seen & {0, 9} and seen & {3, 4, 5, 6, 7, 8}
    random.seed(0), torch.manual_seed(0)
    py_state = random.getstate()
    assert similarity_transform(t, 1)[1:] == (1, 0.0) and random.getstate() == py_state          # a given code draws no code


def test_step_transforms_are_a_pure_function_of_seed_rank_iteration():
    random.seed(5), np.random.seed(5), torch.manual_seed(5)
    state = (np.random.get_state()[1].copy(), random.getstate(), torch.get_rng_state())
    a = step_transforms(6, 42, 0, 7, "sample")
    assert a == step_transforms(6, 42, 0, 7, "sample") and len(a[0]) == len(a[1]) == 6 and len(set(zip(*a))) > 1
    assert a != step_transforms(6, 42, 0, 8, "sample") and a != step_transforms(6, 42, 1, 7, "sample") and a != step_transforms(6, 43, 0, 7, "sample")
    b = step_transforms(6, 42, 0, 7, "batch")
    assert len(set(zip(*b))) == 1 and (b[0][0], b[1][0]) == (a[0][0], a[1][0])
    for c, ang in zip(*step_transforms(64, 1, 0, 0, "sample")):
        assert 0 <= c <= 9 and -90.0 < ang < 90.0
        assert (ang > 0) if c in (3, 5, 7) else (ang < 0) if c in (4, 6, 8) else ang == 0.0
    assert set(step_transforms(64, 1, 0, 0, "sample")[0]) == set(range(10))
    codes, angles = step_transforms(32, 1, 0, 0, "sample", codes=(1, 4), max_angle=10.0)
    assert set(codes) == {1, 4} and all(-10.0 < v <= 0.0 for v in angles)
    assert np.array_equal(np.random.get_state()[1], state[0]) and random.getstate() == state[1] and torch.equal(torch.get_rng_state(), state[2])
    boxes = A.step_boxes(4, 64, 64, 0.25, 42, 0, 7, "sample")              # CutMix's key is untouched
    np_rng, py_rng = A.step_generators(42, 0, 7)
    assert boxes == [A.draw_box(64, 64, 0.25, np_rng, py_rng) for _ in range(4)]
    for bad in (dict(per="image"), dict(codes=()), dict(codes=(10,)), dict(codes=(-1, 2))):
        with pytest.raises(ValueError):
            step_transforms(4, 42, 0, 7, **bad)


def test_config_fields_and_their_validation():
    from vq_seg_amd.trainer import CPSConfig
    cfg = CPSConfig(model={})
    assert cfg.easy_aug is None and cfg.easy_aug_per == "batch" and cfg.easy_aug_max_angle == 90.0 and tuple(cfg.easy_aug_codes) == tuple(range(10))
    assert CPSConfig(model={}, easy_aug="similarity", easy_aug_per="sample", easy_aug_codes=[1, 3], easy_aug_max_angle=180.0).easy_aug_codes == (1, 3)
    for bad in (dict(easy_aug="rotate"), dict(easy_aug_per="image"), dict(easy_aug_codes=()), dict(easy_aug_codes=(10,)), dict(easy_aug_codes=(-1,)),
                dict(easy_aug_max_angle=-1.0), dict(easy_aug_max_angle=180.5)):
        with pytest.raises(ValueError):
            CPSConfig(model={}, **bad)


def test_affine_warp_abi_refuses_bad_arguments_before_any_launch():
    L = _hip.lib()
    assert hasattr(L, "vqseg_affine_warp_f") and "vqseg_affine_warp_f" in _hip.SYMBOLS
    x = torch.zeros(2, 3, 4, 6)
    ok = similarity_matrices([3, 1], [17.3, 0.0])
    calls = _hip.AFFINE_WARP_CALLS
    with pytest.raises(_hip.HipLibraryError, match="float64"):
        _hip.affine_warp(x.double(), ok)                                                         # bilinear takes f32 / bf16
    with pytest.raises(_hip.HipLibraryError, match="int64"):
        _hip.affine_warp(torch.zeros(2, 4, 6, dtype=torch.int64), ok, mode="bilinear")           # unsupported width / mode pair
    with pytest.raises(_hip.HipLibraryError, match="complex64"):
        _hip.affine_warp(x.to(torch.complex64), ok, mode="nearest")
    with pytest.raises(_hip.HipLibraryError, match="shape and layout"):
        _hip.affine_warp(x, ok, out=torch.zeros(2, 3, 4, 5))
    with pytest.raises(_hip.HipLibraryError, match="shape and layout"):
        _hip.affine_warp(x, ok, out=torch.zeros(2, 3, 4, 6).contiguous(memory_format=torch.channels_last))
    with pytest.raises(_hip.HipLibraryError, match="shape and layout"):
        _hip.affine_warp(x, ok, out=torch.zeros(2, 3, 4, 12)[:, :, :, ::2])                     # out rows not dense
    with pytest.raises(_hip.HipLibraryError, match="dense"):
        _hip.affine_warp(torch.zeros(2, 3, 4, 12)[:, :, :, ::2], ok)                             # src rows not dense
    with pytest.raises(_hip.HipLibraryError, match="dense"):
        _hip.affine_warp(torch.zeros(2, 8, 6)[:, ::2], ok)
    for mats in (ok[:1], np.concatenate([ok, ok[:1]]), np.zeros((2, 4), dtype=np.float32), [], "rows"):
        with pytest.raises(_hip.HipLibraryError, match="per sample|six numbers"):
            _hip.affine_warp(x, mats)
    for v in (float("nan"), float("inf"), -float("inf")):
        bad = ok.copy()
        bad[1, 3] = v
        with pytest.raises(_hip.HipLibraryError, match="finite"):
            _hip.affine_warp(x, bad)
    bad = ok.copy()
    bad[0, 2] = 1.0
    with pytest.raises(_hip.HipLibraryError, match="reserved"):
        _hip.affine_warp(x, bad)
    with pytest.raises(_hip.HipLibraryError, match="mode"):
        _hip.affine_warp(x, ok, mode="bicubic")
    with pytest.raises(_hip.HipLibraryError, match="tensor"):
        _hip.affine_warp(torch.zeros(4, 6), ok)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        _hip.affine_warp(x, ok)                                                                  # everything in order but the device
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        _hip.affine_warp(torch.zeros(2, 4, 6, dtype=torch.int64), ok, mode="nearest", fill=255)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        _hip.affine_warp(x, ok, out=torch.zeros(4, 3, 4, 6)[::2])                                # a larger sample stride is a valid out
    assert _hip.AFFINE_WARP_CALLS == calls                                                       # nothing reached the library
    # the entry point's own checks (a caller that is not the wrapper); 16 and 32 stand for two distinct device addresses

    def rc(mode=0, eb=4, src=16, out=32, n=2, p=3, h=4, w=6, ss=72, so=72, sp=24, sx=1, mats=ok):
        return L.vqseg_affine_warp_f(mode, eb, src, out, n, p, h, w, ss, so, sp, sx, mats.ctypes.data if mats is not None else None, 0, None)

    nan = ok.copy()
    nan[1, 0] = float("nan")
    inf = ok.copy()
    inf[0, 4] = float("inf")
    shifted = ok.copy()
    shifted[1, 5] = 0.5
    assert rc(mats=nan) == -1 and b"finite" in L.vqseg_last_error()
    assert rc(mats=inf) == -1 and b"finite" in L.vqseg_last_error()
    assert rc(mats=shifted) == -1 and b"reserved" in L.vqseg_last_error()
    assert rc(mode=2) == -1 and b"mode" in L.vqseg_last_error()
    assert rc(mode=-1) == -1 and b"mode" in L.vqseg_last_error()
    assert rc(eb=3) == -1 and b"width" in L.vqseg_last_error()
    assert rc(eb=8) == -1 and b"bilinear" in L.vqseg_last_error()                                # bilinear on 8-byte elements
    assert rc(eb=1) == -1 and b"bilinear" in L.vqseg_last_error()
    assert rc(sx=2) == -1 and b"layout" in L.vqseg_last_error()
    assert rc(sp=1, sx=2) == -1 and b"layout" in L.vqseg_last_error()
    assert rc(sp=25) == -1 and b"layout" in L.vqseg_last_error()
    assert rc(ss=71) == -1 and b"sample stride" in L.vqseg_last_error()
    assert rc(so=71) == -1 and b"sample stride" in L.vqseg_last_error()
    assert rc(out=16) == -1 and b"out of place" in L.vqseg_last_error()
    assert rc(src=None) == -1 and b"null" in L.vqseg_last_error()
    assert rc(out=None) == -1 and b"null" in L.vqseg_last_error()
    assert rc(mats=None) == -1 and b"null" in L.vqseg_last_error()
    for kw in (dict(n=0), dict(p=0), dict(h=0), dict(w=-1)):
        assert rc(**kw) == -1 and b"positive" in L.vqseg_last_error()
    assert rc(h=(1 << 24) + 1, p=1, sp=0) == -1 and b"2^24" in L.vqseg_last_error()


def test_reference_trainers_import_through_compat(tmp_path):
    script = tmp_path / "easyhard_head.py"
    script.write_text(textwrap.dedent('''
        import sys
        sys.path.insert(0, sys.argv[1])
        from data.augmentations import CutMix, similarity_transform, inverse_similarity_transform
        import vq_seg_amd.data.augmentations as real
        assert similarity_transform is real.similarity_transform and inverse_similarity_transform is real.inverse_similarity_transform
        import torch
        x = torch.arange(12.0).reshape(1, 1, 3, 4)
        out, aug, angle = similarity_transform(x, 2)
        assert torch.equal(inverse_similarity_transform(out, aug, angle), x)
        print("imported", CutMix.__name__)
    '''))
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    res = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "compat")], cwd=str(tmp_path), env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stdout.strip().splitlines()[-1] == "imported CutMix"
