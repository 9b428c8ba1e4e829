"""Writes tests/golden/cutmix_ref.npz: what the REFERENCE's data/augmentations.py (imported through oracle/ref_harness.install())
draws and computes for seeded global generators -- boxes (as masks), CutMix outputs for float and int64 batches, augmentation()
outputs for `cutmix`, and the next draw of each global generator afterwards (the generators' state).  Data only; needs the
reference tree, so it runs where the goldens are made, never in a test.

    python tools/make_cutmix_golden.py
"""
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402
from tests import synth  # noqa: E402

# (H, W, ratio, seed): square, non-square, the smallest size a quarter box can be drawn for, an empty box (cut_h = 0: 3 x 9), the lost last row of the inclusive y1 draw (8 x 8, seed 6)
CASES = [(8, 8, 0.25, 3), (5, 7, 0.2, 3), (4, 4, 0.25, 0), (4, 4, 0.25, 1), (6, 10, 0.25, 7), (9, 13, 0.1, 11), (7, 5, 0.3, 5),
         (3, 9, 0.02, 2), (8, 8, 0.25, 4), (8, 8, 0.25, 5), (8, 8, 0.25, 6), (12, 6, 0.5, 9)]
BATCH, PLANES = 3, 2


def inputs(h, w, seed):
    """deterministic batches (tests/synth.py generators): float image-like, int64 label-like, float logits-like"""
    x = synth.uniform(100 + seed, (BATCH, PLANES, h, w), -1.0, 1.0)
    lab = (synth.uniform(200 + seed, (BATCH, h, w), 0.0, 3.0)).long()
    logits = synth.uniform(300 + seed, (BATCH, 3, h, w), -4.0, 4.0)
    return x, lab, logits


def seed_all(seed):
    np.random.seed(seed)
    random.seed(seed)


def main():
    ref_harness.install()
    import data.augmentations as ref                         # the reference's module
    out = {"cases": np.array(CASES, dtype=np.float64), "batch": np.array([BATCH, PLANES])}
    for i, (h, w, ratio, seed) in enumerate(CASES):
        x, lab, logits = inputs(h, w, seed)
        seed_all(seed)
        out[f"mask_{i}"] = ref.CutMix(ratio)._make_mask((h, w)).numpy()
        out[f"next_{i}"] = np.array([np.random.randint(0, 1 << 30), random.randint(0, 1 << 30)], dtype=np.int64)
        seed_all(seed)
        out[f"cutout_mask_{i}"] = ref.make_cutout_mask((h, w), ratio).numpy()
        seed_all(seed)
        mixed, mask = ref.CutMix(ratio)(x)
        out[f"mix_f_{i}"] = mixed.numpy()
        assert np.array_equal(mask.numpy(), out[f"mask_{i}"])
        mixed_l, _ = ref.CutMix(ratio)(lab, mask)            # the mask handed back in, as train_vqpt_easyhard_aug.py:119-123 does
        out[f"mix_i_{i}"] = mixed_l.numpy()
        assert mixed_l.dtype == torch.int64
        seed_all(seed)
        a_in, a_lab, a_log = ref.augmentation(x, lab.clone(), logits, ref_harness.AttrDict(name="cutmix", ratio=ratio))
        out[f"aug_in_{i}"], out[f"aug_lab_{i}"], out[f"aug_log_{i}"] = a_in.numpy(), a_lab.numpy(), a_log.numpy()
        out[f"aug_next_{i}"] = np.array([np.random.randint(0, 1 << 30), random.randint(0, 1 << 30)], dtype=np.int64)
    path = os.path.join(ROOT, "tests", "golden", "cutmix_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for i, (h, w, ratio, seed) in enumerate(CASES):
        rows, cols = np.where((out[f"mask_{i}"] == 0).any(1))[0], np.where((out[f"mask_{i}"] == 0).any(0))[0]
        print((h, w, ratio, seed), "rows", (rows.min(), rows.max() + 1) if len(rows) else None, "cols", (cols.min(), cols.max() + 1) if len(cols) else None)


if __name__ == "__main__":
    main()
