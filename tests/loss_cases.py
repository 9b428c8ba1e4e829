"""Inputs of the focal / class-weight fixtures (tests/golden/focal_ref.npz): generated from seeds on any machine, so the golden
file holds only what the reference computed from them (tools/make_loss_golden.py) and the tests rebuild the same inputs."""
import torch

from tests import synth

SHAPES = [(3, 3, 9, 13), (2, 3, 17, 31)]          # (B, C, H, W); C = 3: the reference's mask stack is hard-wired (focal_loss.py:13)
ALPHA = 0.25
GAMMAS = (0, 2, 3)
REDUCTIONS = ("sum", "mean", "none")
WEIGHT = (0.5, 0.8, 1.0)                          # deprecated/train_vq_pt_unet_withtest.py:283
IGNORE = 255
MODULE_CASES = [(2, "mean", 0), (2, "mean", 1), (3, "sum", 1)]       # (gamma, reduction, weighted) of FocalLoss in module form


def inputs(s: int):
    """-> logits (B, C, H, W) in [-8, 8) (the reference stays finite), targets (B, H, W) with ~20 % ignored pixels -- and, for
    shape 0, image 1 ignored entirely --, the same targets without ignored pixels, a cotangent (B, HW) for reduction 'none'"""
    b, c, h, w = SHAPES[s]
    logits = synth.uniform(500 + s, (b, c, h, w), -8.0, 8.0)
    clean = synth.labels(510 + s, (b, h, w), c)
    target = torch.where(synth.uniform(520 + s, (b, h, w)) < 0.2, torch.full_like(clean, IGNORE), clean)
    if s == 0:
        target[1] = IGNORE
    cot = synth.uniform(530 + s, (b, h * w), -1.0, 1.0)
    return logits, target, clean, cot


def weight():
    return torch.tensor(WEIGHT, dtype=torch.float32)


def missing_class_labels():
    """labels in which class 1 never occurs"""
    return synth.labels(540, (2, 11, 7), 2) * 2


def focal_key(s, gamma, weighted, reduction):
    return f"focal_{s}_g{gamma}_w{int(weighted)}_{reduction}"


def module_key(s, gamma, weighted, reduction):
    return f"module_{s}_g{gamma}_w{int(weighted)}_{reduction}"
