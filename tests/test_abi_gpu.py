"""GPU-side checks of the one launch path (_hip.launch): a tensor that is not on the GPU is refused by the call it belongs to --
also where a null pointer would have meant "absent" -- nothing is enqueued, nothing of the refused call reaches the next one, and a
failed entry point is reported under its own name.  Every refusal happens on the host."""
import pytest
import torch

from vq_seg_amd import _hip, nnf

pytestmark = pytest.mark.gpu
E = _hip.HipLibraryError


def test_mixed_device_call_with_a_cpu_tensor_in_a_nullable_argument():
    m, c = 64, 32
    g = torch.Generator().manual_seed(1)
    y = torch.randn(m, c, generator=g).to(torch.bfloat16)
    rr = torch.randn(m, c, generator=g).to(torch.bfloat16)
    coef = torch.randn(4, c, generator=g).cuda()
    with pytest.raises(E, match="residual: the HIP path needs .* got cpu. There is no CPU fallback."):
        nnf._bn_apply(y.cuda(), rr, coef, m, c, True)               # NULL would have meant "no residual": a wrong result
    second = nnf._bn_apply(y.cuda(), rr.cuda(), coef, m, c, True)
    third = nnf._bn_apply(y.cuda(), rr.cuda(), coef, m, c, True)
    none = nnf._bn_apply(y.cuda(), None, coef, m, c, True)
    torch.cuda.synchronize()
    assert torch.equal(second.view(torch.int16), third.view(torch.int16))        # no state leaks from the refused call
    assert not torch.equal(second.view(torch.int16), none.view(torch.int16))     # ... and the residual is what made the difference


def test_mixed_device_call_with_a_cpu_tensor_in_a_required_argument():
    from oracle import torch_ref
    n, c, k = 128, 16, 8
    g = torch.Generator().manual_seed(2)
    codebook = torch.randn(k, c, generator=g)
    # every row 0.05-sigma noise around one code; the codes are ~sqrt(2 c) apart: no near-tie that rounding could decide
    rows = codebook[torch.randint(0, k, (n,), generator=g)] + 0.05 * torch.randn(n, c, generator=g)
    with pytest.raises(E, match="codebook: the HIP path needs .* got cpu. There is no CPU fallback."):
        _hip.vq_assign(rows.cuda(), codebook)
    idx = _hip.vq_assign(rows.cuda(), codebook.cuda())
    _, ref_idx, _ = torch_ref.vq_lookup(rows, codebook)
    assert torch.equal(idx.cpu(), ref_idx)


def test_a_failed_entry_point_is_reported_under_its_own_name():
    rows = torch.zeros(128, 6, dtype=torch.bfloat16, device="cuda")  # C = 6: refused by the entry point's shape check, before any launch
    codebook = torch.zeros(8, 6, device="cuda")
    with pytest.raises(E, match=r"vqseg_vq_assign_bf16 failed \(code -1\): .*multiple of 4"):
        _hip.vq_assign(rows, codebook)
    with pytest.raises(E, match=r"vqseg_vq_assign_f32 failed \(code -1\): .*multiple of 4"):
        _hip.vq_assign(rows.float(), codebook)
    with pytest.raises(E, match=r"vqseg_vq_forward_bf16 failed \(code -1\): .*multiple of 4"):
        _hip.vq_forward(rows, codebook, False, 1.0)
    with pytest.raises(E, match=r"vqseg_vq_assign_bf16 failed \(code -1\): .*multiple of 4"):
        _hip.launch("vqseg_vq_assign_bf16", rows.device, None, None, None, 16, 6, 8, None, None, None, 0)


def test_a_failed_fused_batchnorm_entry_point_zeroes_the_modules_counters():
    bn = torch.nn.BatchNorm2d(8).cuda()
    bn._vq_sync = torch.tensor([3, 0, 1, 0], dtype=torch.int32, device="cuda")
    with pytest.raises(E, match="vqseg_bn_apply_f failed"):         # null arguments: the entry point returns an error code, launches nothing
        nnf._check_fused_bn("vqseg_bn_apply_f", bn.weight.device, bn, 1, None, None, None, None, 0, 0, 0, None)
    assert int(bn._vq_sync.abs().sum()) == 0
