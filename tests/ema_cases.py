"""The averaged ("teacher") weights of vqseg_adam_ema_step_f32: emulation, counted bar, assertion function and the builder of the
second launch table.  Not a test module; builds on tests/optim_cases.py (imported, not edited).  tests/test_ema_kernel_gpu.py feeds
`check_ema` what the kernel returned, tests/test_ema_teacher_cpu.py feeds it emulations that carry one defect each.  Nothing here
touches the GPU at import.

Bars.  None is fitted to a kernel's output.
  * e' against `ema_emulate` -- d = p' - e rounded once, fma(w, d, e) rounded once, w = float32(1 - decay) formed in double: bit for
    bit, NaNs by position, signed zeros by bits; a copy record: the bits of p';
  * `ema_emulate` against float64 e + w (p' - e) from the same float32 inputs and the same float32 w: per element h(e') + w h(p' - e),
    h(x) = ulp32(x) / 2 as in optim_cases.fp64_bars (one rounding of the fma at the size of the result, one of the difference scaled by w)."""
import numpy as np

from tests import optim_cases as C

DECAY = 0.99                                      # the kernel cases' decay: w = float32(0.01) is not a power of two
DEFECTS = ("unfused", "decay_for_w", "old_p", "copy_ignored", "skip_last")


def ema_weight(decay):
    """w of the entry point: 1 - decay in double, cast once"""
    return np.float32(1.0 - float(decay))


def ema_emulate(e, p_new, decay, copy, defect=None, p_old=None):
    """e' of one launch, float32, operation by operation -> float32 array.  copy: the bits of p_new.
    defect (tests/test_ema_teacher_cpu.py): 'unfused' (product and add rounded separately), 'decay_for_w' (decay where 1 - decay belongs),
    'old_p' (the average of the parameter BEFORE this step: needs p_old), 'copy_ignored', 'skip_last'."""
    f = np.float32
    e, p_new = np.array(e, dtype=f), np.array(p_new, dtype=f)
    if copy and defect != "copy_ignored":
        out = p_new.copy()
    else:
        w = f(float(decay)) if defect == "decay_for_w" else ema_weight(decay)
        src = np.array(p_old, dtype=f) if defect == "old_p" else p_new
        with np.errstate(all="ignore"):
            d = (src - e).astype(f)
            out = (e + (w * d).astype(f)).astype(f) if defect == "unfused" else C.fma32(w, d, e)
    if defect == "skip_last" and e.size:
        out.reshape(-1)[-1] = e.reshape(-1)[-1]
    return out


def ema_fp64(e, p_new, decay):
    """-> (e' in float64 from the float32 inputs and the float32 w, the counted per-element bar)"""
    w = float(ema_weight(decay))
    e, p_new = (np.asarray(t, dtype=np.float32).astype(np.float64) for t in (e, p_new))
    d = p_new - e
    ref = e + w * d
    h = lambda x: C.ulp32(x) / 2
    # h() at |x| + the error x inherits, and the factor 1 + 2^-10 for second-order terms, as optim_cases.fp64_bars does
    in_e = w * h(d)
    return ref, (h(np.abs(ref) + in_e) + in_e) * (1 + 2.0 ** -10)


def check_ema(got, e_old, p_new, decay, copy, label, defect=None, p_old=None):
    """THE assertion of the averaged values: bit-equal to the emulation (NaN by position) -> the expected e'"""
    want = ema_emulate(e_old, p_new, decay, copy, defect=defect, p_old=p_old) if defect else ema_emulate(e_old, p_new, decay, copy)
    C.check_bits(got, want, f"{label} e against the float32 emulation ({'copy' if copy else 'average'})")
    return want


def ema_data(seed, n):
    """a teacher as a history of averaging leaves it: near the student's range, not equal to it"""
    rs = np.random.RandomState(seed)
    return rs.uniform(-0.25, 0.25, size=n).astype(np.float32)


def special_e(n, seed=91):
    """n averaged values cycling through +-0, subnormals, +-inf, NaN and ordinary ones, shuffled"""
    f = np.float32
    vals = np.array([f(0.0), f(-0.0), f(1e-45), f(-3e-42), f(1.1754942e-38), f(-7e-40), f(np.inf), f(-np.inf), f(np.nan), f(0.1), f(-1e-30),
                     f(3.3e38), f(-0.2)], dtype=f)
    out = vals[np.arange(n) % vals.size]
    return np.ascontiguousarray(out[np.random.RandomState(seed).permutation(n)])


# ---------------------------------------------------------------------------------------------------------------------
# the second launch table
# ---------------------------------------------------------------------------------------------------------------------
class EmaParam:
    """the VqsegEmaParam record that goes with one optim_cases.AdamParam, with its guarded buffers.  e_values None: e == NULL (the record
    keeps no average).  images: subset of 'fwd', 'tr', 's3' (sizes of the AdamParam's geometry).  average_only: the AdamParam record is
    written with g = m = v = NULL."""

    def __init__(self, device, adam, e_values=None, copy=0, images=(), shift=0, average_only=False):
        self.adam, self.copy, self.average_only = adam, int(copy), average_only
        self.e0 = None if e_values is None else np.ascontiguousarray(e_values, dtype=np.float32).reshape(-1)
        assert self.e0 is None or self.e0.size == adam.numel
        self.e = None if self.e0 is None else C.Guarded(device, adam.numel, "f32", shift, self.e0)
        k, cout, cin = adam.k, adam.cout, adam.cin
        sizes = {"fwd": C.fwd_elems(cout, cin, k, k), "tr": C.tr_elems(cout, cin, k, k), "s3": cout * k * k * 3 * cin} if k else {}
        self.img = {name: C.Guarded(device, sizes[name], "i16") for name in images}

    def record(self, rec):
        rec["e"] = 0 if self.e is None else self.e.ptr
        rec["copy"] = self.copy
        for name, b in self.img.items():
            rec[name] = b.ptr

    def result(self):
        return None if self.e is None else self.e.get()

    def guards_intact(self):
        return all(b.guards_intact() for b in ([self.e] if self.e is not None else []) + list(self.img.values()))

    def untouched(self):
        same = self.e is None or bool((C.f32_bits(self.e.get()) == C.f32_bits(self.e0)).all())
        return same and all((b.get() == C.I16_FILL).all() for b in self.img.values())


def ema_tables(params, emas):
    """(VqsegAdamParam records, VqsegEmaParam records) as numpy structured arrays"""
    from vq_seg_amd.optim import _EMA_REC, _REC
    rec, erec = np.zeros(len(params), dtype=_REC), np.zeros(len(params), dtype=_EMA_REC)
    for i, (p, e) in enumerate(zip(params, emas)):
        p.record(rec[i])
        e.record(erec[i])
        if e.average_only:
            rec[i]["g"] = rec[i]["m"] = rec[i]["v"] = 0
    return rec, erec


def ema_launch(params, emas, items, hyper, decay, copy_all=0, null_params=False, null_ema=False, null_items=False, n_items=None):
    """vqseg_adam_ema_step_f32 on the two tables -> its return code (synchronised)"""
    import torch
    from vq_seg_amd import _hip
    L = _hip.lib()
    dev = params[0].buf["p"].raw.device
    rec, erec = ema_tables(params, emas)
    rec_d = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    erec_d = torch.from_numpy(erec.view(np.uint8).copy()).to(dev)
    items_d = torch.from_numpy(np.ascontiguousarray(items, dtype=np.int32).reshape(-1).copy() if len(items) else np.zeros(2, dtype=np.int32)).to(dev)
    lr, b1, b2, eps, step = hyper
    n = int(len(items)) if n_items is None else n_items
    rc = L.vqseg_adam_ema_step_f32(None if null_params else rec_d.data_ptr(), None if null_ema else erec_d.data_ptr(),
                                   None if null_items else items_d.data_ptr(), n, float(lr), float(b1), float(b2), float(eps), int(step),
                                   float(decay), int(copy_all), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc
