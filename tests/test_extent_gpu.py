"""Extent suite: no training-step kernel writes or reads outside its buffers.

Every case of tests/extent_cases.py is called three times on the same input values (tests/extent.py, run_case): P on plain
tensors, A with the inputs embedded in 0xff bytes and the outputs, in-outs and workspaces guarded and pre-filled with 0xff, B the
same with 0x00.  Asserted: all three calls return 0; after A and B every band of every buffer, inputs included, holds its bytes;
every output and in-out result is bit-identical in P, A and B; no input changed; a workspace, prepared image or packed image of
exactly the size the size function returns suffices (the band starts at the next byte), and one byte less is refused with nothing
written.  No parity is checked here: the kernel is compared with itself under other surroundings.

What a refusal returns: the header gives VQSEG_ENOSPC to "workspace too small" and VQSEG_EINVAL to bad arguments (an unaligned
pointer, a variant switched off); the checks below assert exactly those."""
import contextlib
import re

import pytest
import torch

from tests import extent as E
from tests import extent_cases as C
from tests.test_nn_kernels_gpu import dev, lib, option

pytestmark = pytest.mark.gpu

VQSEG_EINVAL, VQSEG_ENOSPC = -1, -2


@contextlib.contextmanager
def options(opts):
    with contextlib.ExitStack() as stack:
        for key, value in opts.items():
            stack.enter_context(option(key, value))
        yield


# The kernel family a convolution case names is the one its launches take: the top hexadecimal digit of "conv_last_variant"
# (include/vqseg.h: 1 LDS-DMA implicit GEMM, 2 generic implicit GEMM, 3 3x3 patch kernel, 4 nine-tap / 5 1x1 / 6 per-tap weight gradient).
KERNEL_FAMILY = {
    ("vqseg_conv2d_f", "vqseg_conv2d_affine_f", "vqseg_conv2d_affine_bits_f", "vqseg_conv2d_dgrad_s2_f"):
        [("ldsdma", 1), ("generic", 2), ("precise", 2), ("patch", 3)],
    ("vqseg_conv2d_wgrad_f", "vqseg_conv2d_wgrad2_f"): [("ninetap", 4), ("1x1-ldsdma", 5), ("im2col-ldsdma", 5), ("pertap", 6)],
    ("vqseg_conv2d_dgrad_s2_fold_f", "vqseg_reflect_ring_f"): [("", 1)],
}


def named_family(case):
    for entries, keys in KERNEL_FAMILY.items():
        if case.entry in entries:
            return next((digit for key, digit in keys if key in case.name), None)
    return None


@pytest.mark.parametrize("case", C.CASES, ids=[f"{c.entry[6:]}-{c.name}" for c in C.CASES])
def test_extent(case):
    L = lib()
    spec, call, opts, short = case.build(L)
    what = f"{case.entry} {case.name} ({case.granule})"
    with options(opts):
        assert L.vqseg_set_option(b"conv_last_variant", 0) >= 0 and L.vqseg_set_option(b"vq_filter_launches", 0) >= 0
        runs = E.run_case(spec, call, dev(), torch.cuda.synchronize, what)
        for t in runs if (case.entry, case.name) in C.POST else ():
            C.POST[(case.entry, case.name)](L, t)
        variant = L.vqseg_set_option(b"conv_last_variant", 0)
        filtered = L.vqseg_set_option(b"vq_filter_launches", 0)
        if case.entry.startswith("vqseg_vq_") and "filter-" in case.name + "-" and case.entry != "vqseg_vq_prepare_f32":
            if "filter-off" in case.name:
                assert filtered == 0, f"{what}: {filtered} launches took the candidate filter with its option at 0"
            else:
                assert filtered >= 3, f"{what}: {filtered} of the three launches took the candidate filter the case is meant for"
        if named_family(case) is not None:
            assert variant >> 24 == named_family(case), f"{what}: the launch took kernel {variant:#x}, the case is meant for family {named_family(case)}"
        if short is not None:
            E.run_short(spec, short, dev(), torch.cuda.synchronize, what, codes=(VQSEG_ENOSPC,))


def test_table_is_complete():
    """every entry point the extent suite is to cover (extent_cases.ENTRY_POINTS: the training step's kernels) is declared in the
    header and has a ragged and a smallest case (tests/test_extent_harness_cpu.py checks the table without a GPU as well)"""
    header = open(__file__.replace("tests/test_extent_gpu.py", "include/vqseg.h")).read()
    declared = set(re.findall(r"\b(vqseg_\w+)\s*\(", header))
    assert not set(C.ENTRY_POINTS) - declared, sorted(set(C.ENTRY_POINTS) - declared)
    C.check_table()


UNALIGNED_IDS = [f"{e[6:]}-{n}-{q}" for e, n, q in C.UNALIGNED]


@pytest.mark.parametrize("entry,name,pointer", C.UNALIGNED, ids=UNALIGNED_IDS)
def test_pointer_at_8_mod_16_is_refused_and_nothing_is_written(entry, name, pointer):
    """where the header asks for 16-byte alignment the entry point checks it: VQSEG_EINVAL before anything is enqueued"""
    (case,) = [c for c in C.CASES if (c.entry, c.name) == (entry, name)]
    spec, call, opts, _short = case.build(lib())
    assert spec[pointer] is not None and spec[pointer].align == 16, "the case does not hand this pointer over at 16 bytes"
    spec[pointer].align = 8                                    # guarded / embedded: address == 8 mod 16
    with options(opts):
        E.run_short(spec, call, dev(), torch.cuda.synchronize, f"{entry} {name} with `{pointer}` at 8 mod 16", codes=(VQSEG_EINVAL,))


SWITCHED_OFF = [
    # entry point, case, the option that takes its kernel away: the header promises VQSEG_EINVAL and callers take the other path
    ("vqseg_conv2d_dgrad_s2_fold_f", "ragged-reflect-bn64", "conv_dgrad_s2_merge"),
    ("vqseg_conv2d_dgrad_s2_fold_f", "smallest-zero", "conv_dgrad_s2_merge"),
    ("vqseg_stem7_conv_f", "stat-reflect-ragged", "stem_fused"),
    ("vqseg_stem7_conv_f", "split3-zero-smallest", "stem_fused"),
]


@pytest.mark.parametrize("entry,name,key", SWITCHED_OFF, ids=[f"{e[6:]}-{n}" for e, n, _ in SWITCHED_OFF])
def test_variant_switched_off_refuses_and_writes_nothing(entry, name, key):
    """with its option at 0 the entry point returns VQSEG_EINVAL before anything is enqueued: every byte of every buffer as it was"""
    (case,) = [c for c in C.CASES if (c.entry, c.name) == (entry, name)]
    spec, call, opts, _short = case.build(lib())
    with options(dict(opts, **{key: 0})):
        E.run_short(spec, call, dev(), torch.cuda.synchronize, f"{entry} {name} with {key} = 0", codes=(VQSEG_EINVAL,))
