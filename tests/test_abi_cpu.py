"""CPU-side checks of the C-ABI boundary: the library loads, exports every symbol the header
declares, validates arguments, and refuses CPU tensors (no fallback)."""
import os
import re

import pytest
import torch

from vq_seg_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    text = open(os.path.join(ROOT, "include", "vqseg.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vqseg_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    L = _hip.lib()
    declared = header_symbols()
    assert len(declared) >= 10
    for name in declared:
        assert hasattr(L, name), f"{name} declared in include/vqseg.h but not exported"
        assert name in _hip.SYMBOLS, f"{name} has no ctypes signature in vq_seg_amd/_hip.py"
    assert sorted(_hip.SYMBOLS) == declared
    assert L.vqseg_abi_version() == 1


def header_signatures():
    """name -> (restype, argtypes) as ctypes, parsed from the prototypes of include/vqseg.h (the header is the truth)"""
    import ctypes as C
    text = open(os.path.join(ROOT, "include", "vqseg.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}

    def ctype(decl):
        toks = [t for t in decl.replace("*", " * ").split() if t != "const"]
        if len(toks) > 1 and toks[-1] not in scalars and toks[-1] not in ("void", "char", "hipStream_t", "*"):
            toks.pop()                                          # the parameter's name
        if toks == ["char", "*"]:
            return C.c_char_p
        if "*" in toks or toks == ["hipStream_t"]:
            return C.c_void_p
        return scalars[" ".join(toks)]

    sigs = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(vqseg_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        sigs[name] = (ctype(ret), [ctype(p) for p in params.split(",") if p.strip() != "void"])
    return sigs


def test_ctypes_signatures_are_the_headers():
    """Symbol names alone would let a c_int stand where the header says int64_t: every parameter and return type of every
    prototype, mapped to ctypes, equals what _hip.SYMBOLS binds."""
    sigs = header_signatures()
    assert sorted(sigs) == header_symbols()
    for name, sig in sigs.items():
        assert _hip.SYMBOLS[name] == sig, f"{name}: include/vqseg.h says {sig}, _hip.SYMBOLS binds {_hip.SYMBOLS[name]}"


def test_workspace_and_argument_validation_without_gpu():
    L = _hip.lib()
    assert L.vqseg_vq_workspace_bytes(8192, 512, 512) >= 512 * 512 * 4
    assert L.vqseg_vq_workspace_bytes(0, 512, 512) == 0
    assert L.vqseg_kmeans_workspace_bytes(8192, 512, 512) > L.vqseg_vq_workspace_bytes(8192, 512, 512)
    # null pointers / bad shapes are rejected before anything touches a device
    rc = L.vqseg_vq_assign_f32(None, None, None, 16, 6, 8, None, None, None, 0, None)
    assert rc == -1 and b"multiple of 4" in L.vqseg_last_error()
    rc = L.vqseg_vq_assign_f32(None, None, None, 16, 8, 8, None, None, None, 0, None)
    assert rc == -1 and b"null" in L.vqseg_last_error()
    # the bf16 entry points make the shared shape check first, then their own (8 bf16 = one 16-byte segment)
    rc = L.vqseg_vq_assign_bf16(None, None, None, 16, 6, 8, None, None, None, 0, None)
    assert rc == -1 and b"multiple of 4" in L.vqseg_last_error()
    rc = L.vqseg_vq_assign_bf16(None, None, None, 16, 12, 8, None, None, None, 0, None)
    assert rc == -1 and b"channels % 8 == 0" in L.vqseg_last_error()
    assert L.vqseg_kernel_name(b"vqseg_vq_forward_f32") == b"vq_assign_f32_kernel"


def test_no_cpu_fallback():
    from vq_seg_amd.vector_quantizer import VectorQuantizer
    vq = VectorQuantizer(dim=16, num_embeddings=8)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        vq(torch.rand(1, 16, 4, 4))


def test_make_vq_module_contract():
    from vq_seg_amd.vector_quantizer import Identity, VectorQuantizer, make_vq_module
    enc = (3, 64, 256, 512, 1024, 2048)
    cfg = {"num_embeddings": [0, 0, 512, 512, 512], "distance": "euclidean", "kmeans_init": True}
    mods = make_vq_module(cfg, enc, 5)
    assert [type(m) for m in mods] == [Identity, Identity, VectorQuantizer, VectorQuantizer, VectorQuantizer]
    assert mods[2].codebook.embedding.weight.shape == (512, 512)
    assert mods[4].codebook.embedding.weight.shape == (512, 2048)
    assert mods[2].codebook.initted is False                     # kmeans_init -> N(0,1) until first train forward
    assert list(mods.state_dict()) == [f"{i}.codebook.embedding.weight" for i in (2, 3, 4)]
    x = torch.rand(1, 4, 2, 2)
    assert mods[0](x)[0] is x and mods[0](x)[1:] == (None, None, None)
    every = make_vq_module({"num_embeddings": 16}, enc, 5)
    assert all(isinstance(m, VectorQuantizer) for m in every) and every[0].codebook.initted
    w = every[0].codebook.embedding.weight
    assert w.abs().max() <= 1 / 16                               # U(-1/K, 1/K), vq_img.py:156-158
    with pytest.raises(ValueError):
        make_vq_module({"num_embeddings": [0, 0, -1, 4, 4]}, enc, 5)
    with pytest.raises(TypeError):
        make_vq_module({"num_embeddings": "512"}, enc, 5)
    with pytest.raises(AssertionError):
        make_vq_module({"num_embeddings": [0, 512]}, enc, 5)
    with pytest.raises(NotImplementedError):
        VectorQuantizer(dim=8, num_embeddings=4, distance="cosine")


# ---------------------------------------------------------------------------------------------------------------------------
# The ctypes boundary takes untyped pointers: every tensor crosses it through _hip.tptr, which checks the element type against
# the flag / entry point it travels with, density, the element count the sizes imply, and the device -- type and size BEFORE the
# device, so a box without a GPU can feed every wrapper the wrong thing (the r2 fault was a bf16 buffer
# behind the f32 entry point).
# ---------------------------------------------------------------------------------------------------------------------------
def test_tptr_checks_type_flag_size_density_then_device():
    E = _hip.HipLibraryError
    f32, bf = torch.zeros(4, 8), torch.zeros(4, 8, dtype=torch.bfloat16)
    assert _hip.tptr(None, "x") is None
    with pytest.raises(E, match="expected torch.bfloat16, got torch.float32"):
        _hip.tptr(f32, "rows", bf=1)
    with pytest.raises(E, match="expected torch.float32, got torch.bfloat16"):
        _hip.tptr(bf, "rows", bf=0)
    with pytest.raises(E, match="expected torch.bfloat16"):
        _hip.tptr(f32, "split-3 rows", bf=2)
    with pytest.raises(E, match="expected torch.int16"):
        _hip.tptr(bf, "packed weights", dtype=torch.int16)
    with pytest.raises(E, match="need 64 elements, the tensor has 32"):
        _hip.tptr(f32, "rows", bf=0, numel=64)
    with pytest.raises(E, match="at least 33"):
        _hip.tptr(f32, "rows", bf=0, numel=33, at_least=True)
    with pytest.raises(E, match="dense"):
        _hip.tptr(f32[:, ::2], "rows", bf=0)
    with pytest.raises(E, match="expected a tensor"):
        _hip.tptr([1.0], "rows")
    # everything else right: only now the device matters.  tptr does not raise -- the other tensors of the same call get their type /
    # size checks first -- and what it returns is nothing ctypes converts to a pointer: the fact travels with the argument
    import ctypes
    p = _hip.tptr(f32, "rows", bf=0, numel=32)
    assert p is not None and not isinstance(p, int) and not hasattr(p, "_as_parameter_") and p + 64 is p
    with pytest.raises(TypeError):
        ctypes.c_void_p.from_param(p)
    called = []
    proto = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p)
    fn = proto(lambda ptr: called.append(ptr) or 0)
    assert fn(None) == 0 and called == [None]
    with pytest.raises(ctypes.ArgumentError):                        # refused before the foreign function is entered
        fn(p)
    assert called == [None]
    with pytest.raises(E, match="rows: the HIP path needs .* no CPU fallback"):
        _hip.launch("vqseg_vq_assign_f32", f32.device, p, None, None, 4, 8, 8, None, None, None, 0)
    with pytest.raises(E, match="rows: the HIP path needs .* no CPU fallback"):
        _hip.on_gpu(p)
    p = _hip.tptr(f32, "rows", bf=0)
    with pytest.raises(E, match="expected torch.int64"):            # a later type error of the same call wins: it raises at once
        _hip.tptr(f32, "idx", dtype=torch.int64)
    with pytest.raises(E, match="logits: expected a float32"):       # dense=False: a strided view, everything else still checked
        _hip.tptr(bf, "logits", dtype=torch.float32, numel=32, dense=False)
    assert type(_hip.tptr(f32[:, ::2], "logits", dtype=torch.float32, numel=16, dense=False)) is type(p)


WRONG = [
    # (what, call)  -- CPU tensors of the WRONG type / size into each _hip wrapper: the error must name the type / size, not the device
    ("vq_forward f64 rows", lambda: _hip.vq_forward(torch.zeros(8, 16, dtype=torch.float64), torch.zeros(4, 16), False, 1.0), "expected torch.float32"),
    ("vq_forward f16 rows", lambda: _hip.vq_forward(torch.zeros(8, 16, dtype=torch.float16), torch.zeros(4, 16), False, 1.0), "expected torch.float32"),
    ("vq_forward bf16 codebook", lambda: _hip.vq_forward(torch.zeros(8, 16), torch.zeros(4, 16, dtype=torch.bfloat16), False, 1.0), "codebook: expected torch.float32"),
    ("vq_forward codebook width", lambda: _hip.vq_forward(torch.zeros(8, 16), torch.zeros(4, 32), False, 1.0), "codebook: the sizes passed along need 64"),
    ("vq_forward prepared blob", lambda: _hip.vq_forward(torch.zeros(8, 16), torch.zeros(4, 16), False, 1.0, prepared=torch.zeros(3, dtype=torch.uint8)),
     "prepared codebook: the sizes"),
    ("vq_assign f16 rows", lambda: _hip.vq_assign(torch.zeros(8, 16, dtype=torch.float16), torch.zeros(4, 16)), "expected torch.float32"),
    ("vq_assign strided rows", lambda: _hip.vq_assign(torch.zeros(8, 32)[:, ::2], torch.zeros(4, 16)), "dense"),
    ("vq_forward_group mixed", lambda: _hip.vq_forward_group([torch.zeros(8, 16), torch.zeros(8, 16, dtype=torch.bfloat16)], [torch.zeros(4, 16)] * 2,
                                                             [None, None], False, [1.0, 1.0]), "one row type per call"),
    ("vq_backward bf16 grad", lambda: _hip.vq_backward(torch.zeros(8, 16, dtype=torch.bfloat16), None, torch.zeros(8, 16), torch.zeros(8, 16), 1.0),
     "grad_quant: expected torch.float32"),
    ("vq_backward size", lambda: _hip.vq_backward(torch.zeros(4, 16), None, torch.zeros(8, 16), torch.zeros(8, 16), 1.0), "grad_quant: the sizes"),
    ("vq_backward_bf16 f32 rows", lambda: _hip.vq_backward_bf16(torch.zeros(8, 16, dtype=torch.bfloat16), None, torch.zeros(8, 16),
                                                                torch.zeros(8, dtype=torch.int64), torch.zeros(4, 16), 1.0), "rows: expected torch.bfloat16"),
    ("vq_backward_bf16 i32 idx", lambda: _hip.vq_backward_bf16(torch.zeros(8, 16, dtype=torch.bfloat16), None, torch.zeros(8, 16, dtype=torch.bfloat16),
                                                               torch.zeros(8, dtype=torch.int32), torch.zeros(4, 16), 1.0), "idx: expected torch.int64"),
    ("kmeans bf16 samples", lambda: _hip.kmeans(torch.zeros(8, 16, dtype=torch.bfloat16), torch.zeros(4, 16), 2), "samples: expected torch.float32"),
    ("kmeans means width", lambda: _hip.kmeans(torch.zeros(8, 16), torch.zeros(4, 8), 2), "means: the sizes"),
    ("kmeans_accumulate", lambda: _hip.kmeans_accumulate(torch.zeros(8, 16), torch.zeros(4, 16, dtype=torch.float64)), "means: expected torch.float32"),
    ("kmeans_finalize i32 counts", lambda: _hip.kmeans_finalize(torch.zeros(4, 16), torch.zeros(4, dtype=torch.int32), torch.zeros(4, 16)), "counts: expected torch.int64"),
    ("vq_code_sums i32 idx", lambda: _hip.vq_code_sums(torch.zeros(8, 16), torch.zeros(8, dtype=torch.int32), 4), "idx: expected torch.int64"),
    ("vq_ema_update", lambda: _hip.vq_ema_update(torch.zeros(4), torch.zeros(4, 16), torch.zeros(4, 16, dtype=torch.bfloat16), torch.zeros(4, 16),
                                                 torch.zeros(4, dtype=torch.int64), 0.9, 1e-5), "codebook: expected torch.float32"),
    ("vq_prepare", lambda: _hip.vq_prepare(torch.zeros(4, 16, dtype=torch.bfloat16)), "codebook: expected torch.float32"),
]


@pytest.mark.parametrize("what,call,msg", WRONG, ids=[w[0] for w in WRONG])
def test_hip_wrappers_refuse_wrong_types_and_sizes_before_touching_a_device(what, call, msg):
    with pytest.raises((_hip.HipLibraryError, ValueError), match=msg):
        call()


def test_nnf_kernels_refuse_wrong_types_before_touching_a_device():
    """The autograd functions behind nnf.* hand their tensors over through the same helper: wrong element types raise in Python."""
    from vq_seg_amd import nnf
    E = _hip.HipLibraryError
    x64 = torch.zeros(1, 8, 4, 4, dtype=torch.float64)
    for fn in (lambda: nnf._MaxPool.apply(x64), lambda: nnf._Bilinear.apply(x64, 8, 8, False),
               lambda: nnf._Head1x1.apply(x64, torch.zeros(3, 8, 1, 1))):
        with pytest.raises(E, match="float32 .* or bfloat16"):
            fn()
    xb = torch.zeros(1, 8, 4, 4, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with pytest.raises(E, match="head weight: expected torch.float32"):
        nnf._Head1x1.apply(xb, torch.zeros(3, 8, 1, 1, dtype=torch.bfloat16))
    with pytest.raises(E, match="split-3 rows: expected torch.bfloat16"):   # an S3 object whose rows are not bf16
        nnf.S3(torch.zeros(1, 4, 4, 16), 8).float()
    with pytest.raises(E, match="need 256 elements"):               # ... or whose channel count disagrees with its rows
        nnf.S3(torch.zeros(1, 4, 4, 8, dtype=torch.bfloat16), 8).float()
    with pytest.raises(E, match="logits: expected a float32"):
        nnf._strided_f32(torch.zeros(2, 3, 4, 4, dtype=torch.bfloat16), "logits", 96)
    with pytest.raises(E, match="logits: the sizes passed along need 96"):
        nnf._strided_f32(torch.zeros(1, 3, 4, 4), "logits", 96)
    with pytest.raises(E, match="no CPU fallback"):
        nnf.softmax_stats(torch.zeros(1, 3, 4, 4), True, True)       # all types right on a CPU tensor: the device error surfaces


def test_an_orphaned_tptr_result_does_not_reach_a_later_call():
    """Nothing about a call is kept between tptr() and its launch: a result that is dropped (an unrelated exception between the two)
    neither fails the next valid call under the wrong tensor's name nor hides that call's own errors."""
    from vq_seg_amd import nnf
    _hip.tptr(torch.zeros(4), "orphan", dtype=torch.float32)
    with pytest.raises(_hip.HipLibraryError, match="logits") as e:
        nnf.softmax_stats(torch.zeros(1, 3, 4, 4), True, True)
    assert "orphan" not in str(e.value) and "no CPU fallback" in str(e.value)
    _hip.tptr(torch.zeros(4), "orphan", dtype=torch.float32)
    with pytest.raises(_hip.HipLibraryError, match="expected torch.float32") as e:
        _hip.vq_forward(torch.zeros(8, 16, dtype=torch.float64), torch.zeros(4, 16), False, 1.0)
    assert "orphan" not in str(e.value)


def test_hip_adam_has_no_cpu_path_and_keeps_torch_adams_layout():
    """optim.HipAdam (r4): a torch.optim.Adam whose step is the HIP kernel -- CPU parameters are refused (no fallback), the
    argument checks of the entry point and the work-item count are host-side."""
    from vq_seg_amd.optim import HipAdam
    p = torch.nn.Parameter(torch.ones(4, 4))
    opt = HipAdam([p], lr=0.1)
    assert isinstance(opt, torch.optim.Adam) and opt.defaults["betas"] == (0.9, 0.999) and opt.defaults["eps"] == 1e-8
    p.grad = torch.ones(4, 4)
    with pytest.raises(_hip.HipLibraryError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(p.detach(), torch.ones(4, 4))              # nothing was updated behind the error
    opt.state[p]["exp_avg_sq"] = torch.zeros(4, 4, dtype=torch.float64)
    with pytest.raises(_hip.HipLibraryError, match="exp_avg_sq: expected torch.float32"):
        opt.step()                                                # a type error of a later tensor wins over the parameter's device error
    L = _hip.lib()
    assert L.vqseg_adam_work_items(4096 * 3 + 1, 0, 0, 0) == 4
    assert L.vqseg_adam_work_items(64 * 32 * 9, 3, 64, 32) == 2 and L.vqseg_adam_work_items(256 * 64, 1, 256, 64) == 8
    assert L.vqseg_adam_step_f32(None, None, 0, 1e-3, 0.9, 0.999, 1e-8, 1, None) == -1
    # the second source of a two-use weight gradient must come with its tensors
    assert L.vqseg_conv2d_wgrad2_f(None, None, None, 1, None, None, None, 1, 8, 4, 4, 8, 4, 4, 8, 3, 3, 1, 1, 0, 0, 8, 0, 0, None, 0, None, None) == -1


def test_profile_begin_raises_on_any_non_zero_code_and_collect_only_on_a_negative_one(monkeypatch):
    """the begin calls answer 0 or an error code -- a HIP error code is positive -- and the collect calls a count"""
    class Stub:
        vqseg_profile_begin = vqseg_conv_profile_begin = staticmethod(lambda capacity: 2)          # hipErrorOutOfMemory
        vqseg_profile_collect = vqseg_conv_profile_collect = staticmethod(lambda *a: 2)            # two records
        vqseg_last_error = staticmethod(lambda: b"profile_begin: out of memory")
    with pytest.raises(_hip.HipLibraryError, match=r"vqseg_profile_begin failed \(code -1\)"):
        _hip.profile_begin(0)                                     # the library itself: capacity out of range
    monkeypatch.setattr(_hip, "lib", lambda: Stub)
    with pytest.raises(_hip.HipLibraryError, match=r"vqseg_profile_begin failed \(code 2\): profile_begin: out of memory"):
        _hip.profile_begin()
    with pytest.raises(_hip.HipLibraryError, match=r"vqseg_conv_profile_begin failed \(code 2\)"):
        _hip.conv_profile_begin()
    assert len(_hip.profile_collect(4)) == 2 and len(_hip.conv_profile_collect(4)) == 2


def test_a_failed_fused_batchnorm_launch_zeroes_the_modules_counters(monkeypatch):
    """the opt-in fused BatchNorm launches hand over through per-module counters that must read zero between launches; an
    entry point that returns an error may leave them dirty -- the host wrapper zeroes them before raising."""
    import torch
    from torch import nn
    from vq_seg_amd import _hip, nnf
    bn = nn.BatchNorm2d(8)
    bn._vq_sync = torch.tensor([3, 0, 1, 0], dtype=torch.int32)
    with pytest.raises(_hip.HipLibraryError):                   # the launch is refused (no GPU here): the error passes through the wrapper
        nnf._check_fused_bn("vqseg_bn_apply_f", torch.device("cpu"), bn, 1, None, None, None, None, 0, 0, 0, None)
    assert int(bn._vq_sync.abs().sum()) == 0
    bn._vq_sync = torch.tensor([3, 0, 1, 0], dtype=torch.int32)
    monkeypatch.setattr(nnf, "_launch", lambda name, dev, *args: None)
    nnf._check_fused_bn("vqseg_bn_apply_f", torch.device("cpu"), bn, 1, None, None, None, None, 0, 0, 0, None)
    assert bn._vq_sync.tolist() == [3, 0, 1, 0]                 # a clean launch touches nothing


# ---------------------------------------------------------------------------------------------------------------------------
# vqseg_set_option is pure host code.  The defaults ARE the dispatch the benchmark measures (profiles/LEDGER.md records each as a
# decision), so they are pinned here, together with what every key does to a value: key -> (default, a second legal value, what
# that value reads back as -- flags store value ? 1 : 0).
# ---------------------------------------------------------------------------------------------------------------------------
OPTIONS = {
    "conv3x3_patch_min_workgroups": (128, 1, 1),
    "conv_wgrad1x1_narrow": (1, 0, 0),
    "stem_fused": (1, 0, 0),
    "conv_wgrad_round_pct": (100, 400, 400),
    "conv_wgrad_xcd": (1, 0, 0),
    "conv_dgrad_s2_merge": (1, 0, 0),
    "conv_wgrad3x3_fill": (1, 0, 0),
    "conv_wgrad3x3_stride2": (1, 0, 0),
    "conv_short_k_small_tile": (1, 3, 3),
    "conv_short_k_single_buffer": (8, 0, 0),
    "conv3x3_patch_unroll": (1, 2, 2),
    "conv_linear_prologue": (1, 0, 0),
    "conv_xcd_pair": (8, 4, 4),
    "conv3x3_patch_xcd_pair": (0, 7, 1),
    "conv3x3_patch_chunk_stage": (1, 0, 0),
    "conv3x3_patch_tile512": (2, 0, 0),
    "conv3x3_patch_tile512_launches": (0, 5, 5),
    "conv3x3_patch_tile512_min_workgroups": (512, 1, 1),
    "conv3x3_patch_wide_tile_s3": (1, 0, 0),
    "conv3x3_patch_wide_tile": (1, 0, 0),
    "conv_last_variant": (0, 0x1248314, 0x1248314),
    "vq_max_tiles_per_wave": (8, 2, 2),
    "vq_fine_split": (1, 0, 0),
    "vq_bf16_filter": (1, 0, 0),
    "vq_filter_force_all": (0, 7, 1),
    "vq_filter_launches": (0, 9, 9),
    "debug_skip_small": (0, 7, 7),
    "bn_bwd_premask": (1, 0, 0),
    "nn_grid_cap": (8192, 256, 256),
    "im2col_strip": (1, 0, 0),
    "bilinear_up2": (1, 2, 2),
}
FLAGS = ["stem_fused", "conv_dgrad_s2_merge", "conv_linear_prologue", "conv3x3_patch_xcd_pair", "conv3x3_patch_chunk_stage",
         "conv3x3_patch_wide_tile_s3", "conv3x3_patch_wide_tile", "vq_fine_split", "vq_bf16_filter", "vq_filter_force_all", "bn_bwd_premask",
         "im2col_strip"]


@pytest.fixture
def option_lib():
    """the library with every option at its default, before and after (it is process-wide and the other tests share it)"""
    assert not os.environ.get("VQSEG_OPTS"), "the defaults are pinned without VQSEG_OPTS"
    L = _hip.lib()
    yield L
    for key, (default, _v, _r) in OPTIONS.items():
        assert L.vqseg_set_option(key.encode(), default) >= 0
    for key, (default, _v, _r) in OPTIONS.items():
        assert L.vqseg_set_option(key.encode(), default) == default, key


@pytest.mark.parametrize("key", sorted(OPTIONS))
def test_option_default_and_stored_value(option_lib, key):
    L = option_lib
    default, second, stored = OPTIONS[key]
    k = key.encode()
    assert L.vqseg_set_option(k, default) == default             # the default, and setting it again changes nothing
    assert L.vqseg_set_option(k, default) == default
    assert L.vqseg_set_option(k, second) == default              # returns the previous value ...
    assert L.vqseg_set_option(k, default) == stored              # ... and stored the new one its own way


def test_option_flags_store_zero_or_one(option_lib):
    L = option_lib
    for key in FLAGS:
        k, default = key.encode(), OPTIONS[key][0]
        L.vqseg_set_option(k, 7)
        assert L.vqseg_set_option(k, 0) == 1, key
        assert L.vqseg_set_option(k, 1 << 20) == 0, key
        assert L.vqseg_set_option(k, default) == 1, key


def test_option_odd_cases(option_lib):
    L = option_lib
    # out of range: ignored, the previous value is still the answer
    for bad in (5, 9, 401, 1 << 30):
        assert L.vqseg_set_option(b"conv_wgrad_round_pct", bad) == 100
    assert L.vqseg_set_option(b"conv_wgrad_round_pct", 10) == 100
    assert L.vqseg_set_option(b"conv_wgrad_round_pct", 401) == 10
    assert L.vqseg_set_option(b"conv_wgrad_round_pct", 100) == 10
    # bilinear_up2: 0 / 1 / 2 as given, anything above reads back as 1
    assert L.vqseg_set_option(b"bilinear_up2", 0) == 1
    assert L.vqseg_set_option(b"bilinear_up2", 3) == 0
    assert L.vqseg_set_option(b"bilinear_up2", 2) == 1
    assert L.vqseg_set_option(b"bilinear_up2", 1000) == 2
    assert L.vqseg_set_option(b"bilinear_up2", 1) == 1
    # out of range answered like an unknown key, nothing stored
    for key, bad in ((b"nn_grid_cap", 255), (b"nn_grid_cap", 0), (b"vq_max_tiles_per_wave", 3), (b"vq_max_tiles_per_wave", 0),
                     (b"vq_max_tiles_per_wave", 16), (b"no_such_option", 1), (b"", 1), (b"stem_fused ", 1), (b"STEM_FUSED", 1)):
        assert L.vqseg_set_option(key, bad) == -1, (key, bad)
        assert L.vqseg_last_error() == b"set_option: unknown key", (key, bad)
    assert L.vqseg_set_option(b"nn_grid_cap", 8192) == 8192 and L.vqseg_set_option(b"vq_max_tiles_per_wave", 8) == 8
    for tiles in (1, 2, 4, 8):
        assert L.vqseg_set_option(b"vq_max_tiles_per_wave", tiles) == (8 if tiles == 1 else tiles // 2)
    assert L.vqseg_set_option(b"nn_grid_cap", (1 << 31) - 1) == 8192
    assert L.vqseg_set_option(b"nn_grid_cap", 8192) == (1 << 31) - 1
    # a null key and a negative value fail before any table is looked at -- for known keys too, which keep their value
    assert L.vqseg_set_option(None, 1) == -1 and L.vqseg_last_error() == b"set_option: null key or negative value"
    for key in sorted(OPTIONS):
        assert L.vqseg_set_option(key.encode(), -1) == -1, key
        assert L.vqseg_last_error() == b"set_option: null key or negative value", key
        assert L.vqseg_set_option(key.encode(), OPTIONS[key][0]) == OPTIONS[key][0], key
    with pytest.raises(_hip.HipLibraryError, match="unknown option 'no_such_option' or bad value 1"):
        _hip.set_option("no_such_option", 1)


def test_option_table_of_the_integration_guide_lists_the_same_keys_and_defaults():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rows = re.findall(r"^\| `([a-z0-9_]+)` \| (\d+) \| (int|flag|range|set) \|", text, flags=re.M)
    assert {k: int(d) for k, d, _ in rows} == {k: v[0] for k, v in OPTIONS.items()}
    assert len(rows) == len(OPTIONS)
    assert sorted(k for k, _, kind in rows if kind == "flag") == sorted(FLAGS)


# ---------------------------------------------------------------------------------------------------------------------------
# vqseg_vq_tiles_per_wave: the code tiles per wave T of the distance launch (vq_group_tiles, vq_host.hip).  The rule, with
# groups_i = ceil(N_i / 128) row groups and tiles_i = ceil(K_i / 32) code tiles per level, wgs(t) = sum_i groups_i * tiles_i / t, t
# "divides" when tiles_i % t == 0 for every level:
#   1. "vq_fine_split" on: the largest t in {cap, cap / 2, ...}, t >= 4, that divides with wgs(t) >= 4096;
#   2. else the largest t in {cap, ..., 1} that divides with wgs(t) >= 512; t = 1 is taken whatever its wgs.
# cap = "vq_max_tiles_per_wave" (8).  Every row below is worked out by hand from this rule (the arithmetic in its comment).
# ---------------------------------------------------------------------------------------------------------------------------
T_CASES = [
    # options, rows per level, codes per level, T
    ({}, [172032], [512], 4),                                     # 1344 groups x 16 tiles: fine split, t=8 2688 < 4096, t=4 5376
    ({"vq_fine_split": 0}, [172032], [512], 8),                   # rule 2 alone: t=8 2688 >= 512
    ({}, [172032], [1024], 8),                                    # 32 tiles: fine split already at t=8: 1344 x 4 = 5376
    ({"vq_max_tiles_per_wave": 4}, [172032], [512], 4),           # fine split from t=4: 5376
    ({"vq_max_tiles_per_wave": 2}, [172032], [512], 2),           # the fine split never looks below 4; rule 2: t=2 1344 x 8
    ({}, [32700], [2048], 4),                                     # 256 groups x 64 tiles: t=8 2048 < 4096, t=4 exactly 4096
    ({"vq_fine_split": 0}, [32700], [2048], 8),                   # rule 2: t=8 2048 >= 512
    ({}, [32640], [2048], 8),                                     # 255 groups: t=4 4080 < 4096, no fine split; rule 2 t=8 2040
    ({}, [8100], [2040], 8),                                      # 64 groups x 64 tiles (2040 -> 2048 codes): t=8 exactly 512
    ({}, [8064], [2040], 4),                                      # 63 groups: t=8 504 < 512, t=4 1008
    ({"vq_max_tiles_per_wave": 4}, [8100], [2040], 4),            # t=4 1024
    ({"vq_max_tiles_per_wave": 2}, [8100], [2040], 2),            # t=2 2048
    ({"vq_max_tiles_per_wave": 1}, [8100], [2040], 1),
    ({}, [8100], [1912], 4),                                      # 60 tiles: 60 % 8 = 4, t=4 64 x 15 = 960
    ({}, [100000], [96], 1),                                      # 3 tiles: neither 8, 4 nor 2 divides
    ({}, [100000], [192], 2),                                     # 6 tiles: t=2 782 x 3 = 2346
    ({}, [128], [256], 1),                                        # 1 group x 8 tiles: at most 8 workgroups, t=1 whatever its count
    ({}, [1000], [1024], 1),                                      # 8 groups x 32 tiles: t=2 128 < 512 -> t=1 (256 workgroups)
    ({}, [32768, 8192, 2048], [512, 512, 512], 8),                # grouped: 336 groups x 16 tiles: t=8 672 (< 4096: no fine split) >= 512
    ({}, [131072, 32768, 8192], [512, 512, 512], 4),              # 1344 groups: fine split, t=8 2688, t=4 5376
    ({}, [32768, 8192], [512, 384], 4),                           # tiles 16 and 12: 12 % 8 != 0; t=4 256 x 4 + 64 x 3 = 1216
    ({}, [32768, 8192], [512, 96], 1),                            # tiles 16 and 3: only t=1 divides both
    ({"vq_fine_split": 0}, [131072, 32768, 8192], [512, 512, 512], 8),
]


@pytest.mark.parametrize("opts,rows,codes,want", T_CASES, ids=[f"{i}-T{c[3]}" for i, c in enumerate(T_CASES)])
def test_vq_tiles_per_wave_follows_the_documented_rule(option_lib, opts, rows, codes, want):
    for k, v in opts.items():
        _hip.set_option(k, v)
    assert _hip.vq_tiles_per_wave(rows, codes) == want
    if len(rows) == 1:
        assert _hip.vq_tiles_per_wave(rows[0], codes[0]) == want


def test_vq_tiles_per_wave_refuses_bad_arguments(option_lib):
    import ctypes
    L = option_lib
    one_n, one_k = (ctypes.c_int64 * 1)(128), (ctypes.c_int * 1)(64)
    assert L.vqseg_vq_tiles_per_wave(0, one_n, one_k) == -1 and L.vqseg_vq_tiles_per_wave(5, one_n, one_k) == -1
    assert L.vqseg_vq_tiles_per_wave(1, None, one_k) == -1 and L.vqseg_vq_tiles_per_wave(1, one_n, None) == -1
    assert L.vqseg_vq_tiles_per_wave(1, (ctypes.c_int64 * 1)(0), one_k) == -1
    assert L.vqseg_vq_tiles_per_wave(1, one_n, (ctypes.c_int * 1)(0)) == -1
    assert b"tiles_per_wave" in L.vqseg_last_error()
    with pytest.raises(ValueError):
        _hip.vq_tiles_per_wave([128, 128], [64])
    with pytest.raises(_hip.HipLibraryError, match="vqseg_vq_tiles_per_wave failed"):
        _hip.vq_tiles_per_wave([128] * 5, [64] * 5)
