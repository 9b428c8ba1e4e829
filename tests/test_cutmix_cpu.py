"""CutMix / CutOut without a GPU: the box draw, the masks and the CPU arithmetic against what the reference's own
data/augmentations.py gave for the same seeds (tests/golden/cutmix_ref.npz, written by tools/make_cutmix_golden.py), the drop-in
`from data import CutMix`, and the argument checks of the box-mix wrapper with the library loaded."""
import os
import random
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

from tests import synth
from vq_seg_amd import _hip
from vq_seg_amd.data import CutMix, CutOut, aug_dict, augmentation, draw_box, make_aug, make_cutout_mask
from vq_seg_amd.data import augmentations as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "cutmix_ref.npz"))
CASES = [(int(h), int(w), float(r), int(s)) for h, w, r, s in GOLD["cases"]]
BATCH, PLANES = (int(v) for v in GOLD["batch"])
IDS = [f"{h}x{w}-r{r}-s{s}" for h, w, r, s in CASES]


def seed_all(seed):
    np.random.seed(seed)
    random.seed(seed)


def inputs(h, w, seed):                                      # tools/make_cutmix_golden.py: inputs()
    x = synth.uniform(100 + seed, (BATCH, PLANES, h, w), -1.0, 1.0)
    lab = (synth.uniform(200 + seed, (BATCH, h, w), 0.0, 3.0)).long()
    logits = synth.uniform(300 + seed, (BATCH, 3, h, w), -4.0, 4.0)
    return x, lab, logits


def test_fixture_covers_what_it_must():
    sizes = {(h, w) for h, w, _r, _s in CASES}
    assert any(h != w for h, w in sizes) and (4, 4, 0.25) in {(h, w, r) for h, w, r, _s in CASES}
    i3 = CASES.index((8, 8, 0.25, 3))                        # the reference's draw for seed 3: rows 1-4, columns 0-5
    want = np.ones((8, 8), dtype=np.int64)
    want[1:4, 0:5] = 0
    assert np.array_equal(GOLD[f"mask_{i3}"], want)
    j3 = CASES.index((5, 7, 0.2, 3))
    want = np.ones((5, 7), dtype=np.int64)
    want[1:2, 0:4] = 0
    assert np.array_equal(GOLD[f"mask_{j3}"], want)
    assert any((GOLD[f"mask_{i}"] == 1).all() for i in range(len(CASES)))      # an empty box is among the cases


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_boxes_and_generator_state_equal_the_reference(i):
    h, w, ratio, seed = CASES[i]
    want = torch.from_numpy(GOLD[f"mask_{i}"])
    seed_all(seed)
    box = draw_box(h, w, ratio)
    nxt = [np.random.randint(0, 1 << 30), random.randint(0, 1 << 30)]
    assert nxt == GOLD[f"next_{i}"].tolist()                 # the same draws were consumed from both global generators
    y1, x1, ch, cw = box
    assert 0 <= y1 and y1 + ch <= h and 0 <= x1 and x1 + cw <= w
    assert torch.equal(A.box_mask((h, w), box), want)
    if not bool((want == 1).all()):                          # a visible box: the tuple itself is the bounding box of the zeros
        rows, cols = np.where((GOLD[f"mask_{i}"] == 0).any(1))[0], np.where((GOLD[f"mask_{i}"] == 0).any(0))[0]
        assert box == (rows.min(), cols.min(), len(rows), len(cols))
    seed_all(seed)
    m = make_cutout_mask((h, w), ratio)
    assert m.dtype == torch.int64 and torch.equal(m, torch.from_numpy(GOLD[f"cutout_mask_{i}"]))
    for cls in (CutMix, CutOut):
        seed_all(seed)
        m = cls(ratio)._make_mask((h, w))
        assert m.dtype == torch.int64 and torch.equal(m, want)
    # non-global generators give the same box and leave the global ones alone
    seed_all(seed + 1000)
    before = (np.random.get_state()[1].copy(), random.getstate())
    rs, pr = np.random.RandomState(seed), random.Random(seed)
    assert draw_box(h, w, ratio, rs, pr) == box
    assert np.array_equal(np.random.get_state()[1], before[0]) and random.getstate() == before[1]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_cutmix_and_augmentation_on_cpu_equal_the_reference(i):
    h, w, ratio, seed = CASES[i]
    x, lab, logits = inputs(h, w, seed)
    keep = (x.clone(), lab.clone(), logits.clone())
    seed_all(seed)
    cm = CutMix(ratio)
    mixed, mask = cm(x)
    assert mixed.dtype == torch.float32 and torch.equal(mixed, torch.from_numpy(GOLD[f"mix_f_{i}"]))
    assert torch.equal(mask, torch.from_numpy(GOLD[f"mask_{i}"]))
    mixed_l, mask_l = cm(lab, mask)                          # the mask handed back in: the pseudo targets' mix
    assert mask_l is mask and mixed_l.dtype == torch.int64 and torch.equal(mixed_l, torch.from_numpy(GOLD[f"mix_i_{i}"]))
    seed_all(seed)
    a_in, a_lab, a_log = augmentation(x, lab, logits, {"name": "cutmix", "ratio": ratio})
    assert [np.random.randint(0, 1 << 30), random.randint(0, 1 << 30)] == GOLD[f"aug_next_{i}"].tolist()
    assert torch.equal(a_in, torch.from_numpy(GOLD[f"aug_in_{i}"])) and torch.equal(a_log, torch.from_numpy(GOLD[f"aug_log_{i}"]))
    assert a_lab.dtype == torch.int64 and torch.equal(a_lab, torch.from_numpy(GOLD[f"aug_lab_{i}"]))
    # the selection (mix_boxes: what the trainer uses on CPU tensors) gives the same values as the reference's arithmetic
    seed_all(seed)
    boxes = [draw_box(h, w, ratio) for _ in range(BATCH)]
    assert torch.equal(A.mix_boxes(x, boxes), a_in) and torch.equal(A.mix_boxes(lab, boxes), a_lab)
    assert all(torch.equal(a, b) for a, b in zip((x, lab, logits), keep))                     # inputs untouched


def test_cutout_is_the_evident_intent_and_spares_the_callers_label():
    h, w, ratio, seed = 8, 8, 0.25, 3
    x, lab, logits = inputs(h, w, seed)
    seed_all(seed)
    out, mask = CutOut(ratio)(x)
    assert torch.equal(out, x * mask) and torch.equal(mask, torch.from_numpy(GOLD[f"mask_{CASES.index((8, 8, 0.25, 3))}"]))
    keep = lab.clone()
    seed_all(seed)
    a_in, a_lab, a_log = augmentation(x, lab, logits, A_cfg("cutout", ratio))
    seed_all(seed)
    masks = [make_cutout_mask((h, w), ratio) for _ in range(BATCH)]
    assert torch.equal(lab, keep)                            # deviation from the reference, on purpose: the caller's label is not written
    for s in range(BATCH):
        assert torch.equal(a_in[s], x[s] * masks[s]) and torch.equal(a_log[s], logits[s] * masks[s])
        assert torch.equal(a_lab[s], torch.where(masks[s] == 0, torch.full_like(lab[s], 255), lab[s]))


class A_cfg:                                                 # attribute access, as the reference's EasyDict config gives
    def __init__(self, name, ratio):
        self.name, self.ratio = name, ratio


def test_draw_box_refuses_what_the_reference_cannot_draw():
    with pytest.raises(ValueError, match="no box width"):
        draw_box(8, 2, 0.5)                                  # np.random.randint(2, 2)
    assert draw_box(8, 2, 0.25)[3] == 1                      # randint(1, 2): the narrowest draw that works
    with pytest.raises(ValueError, match="no box width"):
        draw_box(8, 8, 0.9)                                  # randint(8, 8)
    with pytest.raises(ValueError, match="ratio"):
        draw_box(8, 8, -0.1)
    with pytest.raises(ValueError, match="ratio"):
        draw_box(8, 8, 1.0)
    with pytest.raises(ValueError, match="positive"):
        draw_box(0, 8, 0.25)


def test_make_aug_and_registry():
    cfg = {"name": "cutmix", "ratio": .25}
    aug = make_aug(cfg)
    assert isinstance(aug, CutMix) and aug.ratio == .25
    assert isinstance(make_aug({"name": "cutout", "ratio": .1}), CutOut)
    assert aug_dict == {"cutmix": CutMix, "cutout": CutOut}
    with pytest.raises(KeyError):
        make_aug({"name": "rotate"})


def test_step_boxes_are_a_pure_function_of_seed_rank_iteration():
    seed_all(5)
    state = (np.random.get_state()[1].copy(), random.getstate())
    a = A.step_boxes(4, 64, 64, 0.25, 42, 0, 7, "sample")
    assert a == A.step_boxes(4, 64, 64, 0.25, 42, 0, 7, "sample") and len(set(a)) > 1
    assert a != A.step_boxes(4, 64, 64, 0.25, 42, 0, 8, "sample") and a != A.step_boxes(4, 64, 64, 0.25, 42, 1, 7, "sample")
    b = A.step_boxes(4, 64, 64, 0.25, 42, 0, 7, "batch")
    assert len(set(b)) == 1 and b[0] == a[0]
    np_rng, py_rng = A.step_generators(42, 0, 7)
    assert a == [draw_box(64, 64, 0.25, np_rng, py_rng) for _ in range(4)]
    assert np.array_equal(np.random.get_state()[1], state[0]) and random.getstate() == state[1]          # global generators untouched
    with pytest.raises(ValueError):
        A.step_boxes(4, 64, 64, 0.25, 42, 0, 7, "image")


def test_drop_in_import_through_compat(tmp_path):
    script = tmp_path / "aug_head.py"
    script.write_text(textwrap.dedent('''
        import sys
        sys.path.insert(0, sys.argv[1])
        from data import CutMix, make_aug
        from data.augmentations import augmentation, make_cutout_mask
        import vq_seg_amd.data.augmentations as real
        assert CutMix is real.CutMix and augmentation is real.augmentation
        print(type(make_aug({"name": "cutmix", "ratio": 0.25})).__name__)
    '''))
    env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
    res = subprocess.run([sys.executable, str(script), os.path.join(ROOT, "compat")], cwd=str(tmp_path), env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    assert res.stdout.strip().splitlines()[-1] == "CutMix"


def test_box_mix_abi_refuses_bad_arguments_before_any_launch():
    L = _hip.lib()
    assert hasattr(L, "vqseg_box_mix_f") and "vqseg_box_mix_f" in _hip.SYMBOLS
    x = torch.zeros(2, 3, 4, 6)
    ok = [(0, 0, 1, 1)] * 2
    calls = _hip.BOX_MIX_CALLS
    with pytest.raises(_hip.HipLibraryError, match="float64"):
        _hip.box_mix(x.double(), ok)                                             # wrong dtype
    with pytest.raises(_hip.HipLibraryError, match="shape and layout"):
        _hip.box_mix(x, ok, out=torch.zeros(2, 3, 4, 5))                         # wrong element count
    with pytest.raises(_hip.HipLibraryError, match="shape and layout"):
        _hip.box_mix(x, ok, out=torch.zeros(2, 3, 4, 6).contiguous(memory_format=torch.channels_last))
    with pytest.raises(_hip.HipLibraryError, match="dense"):
        _hip.box_mix(torch.zeros(2, 3, 4, 12)[:, :, :, ::2], ok)                 # rows not dense
    with pytest.raises(_hip.HipLibraryError, match="dense"):
        _hip.box_mix(torch.zeros(2, 8, 6)[:, ::2], ok)
    for bad in ((0, 0, 5, 1), (0, 0, 1, 7), (3, 0, 2, 1), (0, 5, 1, 2), (-1, 0, 1, 1), (0, 0, -1, 1)):
        with pytest.raises(_hip.HipLibraryError, match="outside"):
            _hip.box_mix(x, [ok[0], bad])                                        # a box outside the image
    for boxes in ([ok[0]], ok + ok[:1], [], (0, 0, 1, 1)):
        with pytest.raises(_hip.HipLibraryError, match="per sample"):
            _hip.box_mix(x, boxes)                                               # n boxes != n samples
    with pytest.raises(_hip.HipLibraryError, match="mode"):
        _hip.box_mix(x, ok, mode="blend")
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        _hip.box_mix(x, ok)                                                      # everything in order but the device
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        _hip.box_mix(torch.zeros(2, 4, 6, dtype=torch.int64), ok, mode="fill", fill=255)
    assert _hip.BOX_MIX_CALLS == calls                                           # nothing reached the library
    # the entry point's own checks (a caller that is not the wrapper)
    bx = np.array([[0, 0, 1, 1], [0, 0, 1, 7]], dtype=np.int32)

    def rc(mode=0, eb=4, src=16, out=32, n=2, p=3, h=4, w=6, ss=72, sp=24, sx=1, boxes=bx):
        return L.vqseg_box_mix_f(mode, eb, src, out, n, p, h, w, ss, sp, sx, boxes.ctypes.data if boxes is not None else None, 0, None)

    good = np.array([[0, 0, 1, 1], [3, 5, 1, 1]], dtype=np.int32)
    assert rc() == -1 and b"outside" in L.vqseg_last_error()
    assert rc(boxes=good, eb=3) == -1 and b"width" in L.vqseg_last_error()
    assert rc(boxes=good, mode=2) == -1 and b"mode" in L.vqseg_last_error()
    assert rc(boxes=good, sx=2) == -1 and b"layout" in L.vqseg_last_error()
    assert rc(boxes=good, sp=1, sx=2) == -1 and b"layout" in L.vqseg_last_error()
    assert rc(boxes=good, sp=25) == -1 and b"layout" in L.vqseg_last_error()
    assert rc(boxes=good, ss=71) == -1 and b"sample stride" in L.vqseg_last_error()
    assert rc(boxes=good, out=16) == -1 and b"out of place" in L.vqseg_last_error()
    assert rc(boxes=good, src=None) == -1 and b"null" in L.vqseg_last_error()
    assert rc(boxes=None) == -1 and b"null" in L.vqseg_last_error()
    assert rc(boxes=good, n=0) == -1 and b"positive" in L.vqseg_last_error()


def test_config_default_is_off():
    from vq_seg_amd.trainer import CPSConfig
    cfg = CPSConfig(model={})
    assert cfg.cutmix_ratio is None and cfg.cutmix_boxes == "batch"
