"""CPU-side checks of the split-3 row type of the VQ launch path: the option that selects its kernels, and the Python wrappers' refusals
before any device is touched (the GPU side: tests/test_vq_s3_filter_gpu.py)."""
import pytest
import torch

from vq_seg_amd import _hip, nnf


def test_vq_s3_filter_is_a_flag_with_default_one():
    L = _hip.lib()
    k = b"vq_s3_filter"
    assert L.vqseg_set_option(k, 1) == 1                      # the default
    assert L.vqseg_set_option(k, 7) == 1
    assert L.vqseg_set_option(k, 0) == 1                      # 7 was stored as 1
    assert L.vqseg_set_option(k, 1) == 0
    assert L.vqseg_set_option(k, -1) == -1 and L.vqseg_set_option(k, 1) == 1


def test_wrappers_refuse_mismatched_s3_rows_before_touching_a_device():
    W = torch.zeros(256, 32)
    with pytest.raises(_hip.HipLibraryError, match="2C columns"):
        _hip.vq_assign(torch.zeros(8, 32, dtype=torch.bfloat16), W, s3=True)
    with pytest.raises(_hip.HipLibraryError, match="2C columns"):
        _hip.vq_forward_group([torch.zeros(8, 32, dtype=torch.bfloat16)], [W], [None], False, [1.0], s3=True)
    with pytest.raises(_hip.HipLibraryError, match="eval-mode"):
        _hip.vq_forward_group([torch.zeros(8, 64, dtype=torch.bfloat16)], [W], [None], True, [1.0], s3=True)
    with pytest.raises(_hip.HipLibraryError, match="expected torch.bfloat16"):
        _hip.vq_assign(torch.zeros(8, 64), W, s3=True)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        _hip.vq_assign(torch.zeros(8, 64, dtype=torch.bfloat16), W, s3=True)


def test_s3_from_rows_checks_layout():
    rows = torch.zeros(2, 4, 4, 16, dtype=torch.bfloat16)
    t = nnf.s3_from_rows(rows, 8)
    assert isinstance(t, nnf.S3) and t.shape == (2, 8, 4, 4) and t.rows is rows
    for bad, c in ((rows, 16), (rows.float(), 8), (rows[..., ::2], 4), (rows[0], 8)):
        with pytest.raises(ValueError, match="split-3 rows"):
            nnf.s3_from_rows(bad, c)
