"""Guard-band harness of the extent suite (tests/test_extent_gpu.py; tests/test_extent_harness_cpu.py shows on the CPU that
every check here can fail).

The parity suites ask whether the elements a kernel was supposed to write are right.  This module asks the other question: did
the kernel touch, or depend on, anything else?  A buffer handed to a kernel lies inside one larger allocation, at exactly the
alignment the entry point documents and no better, with a band in front of it and a band behind it:

  guarded(shape, dtype, device, fill)   an output / in-out / workspace view; bands of seeded pseudo-random bytes, a copy kept
  embedded(tensor, band_byte)           an input view with the tensor's values; bands of one byte value (0xff: NaN in f32 / bf16,
                                        -1 in the integer types, 255 in u8; 0x00: zeros), so that a read past the input that reaches
                                        a result gives different results under the two values
  assert_bands_intact(g, what)          both bands byte for byte against the copy
  same_bits(a, b)                       equality through an integer view (NaN equals NaN)

run_case drives one case -- a dict of tagged arguments and a function that makes the call from the materialised tensors --
through the three surroundings P (plain tensors), A (0xff around the inputs and in the outputs) and B (0x00) and asserts what
the extent suite asserts.  It works on CPU tensors as well as on the GPU."""
import torch

BAND_MIN = 4096
BAND_MAX = 1 << 20
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


class _Extent:
    """what the harness remembers about a guarded view: the allocation, where the view lies in it, the copy of both bands"""
    __slots__ = ("base", "start", "nbytes", "front", "back")


def band_bytes(nbytes):
    return min(max(BAND_MIN, int(nbytes)), BAND_MAX)


def _carve(nbytes, device, align, elem):
    """(allocation, byte offset of the view): a band on both sides, the view's address == align mod 2 * align"""
    assert align >= elem and align % elem == 0 and align & (align - 1) == 0, f"alignment {align} for {elem}-byte elements"
    band = band_bytes(nbytes)
    base = torch.empty(2 * band + nbytes + 2 * align, dtype=torch.uint8, device=device)
    start = band + (align - (base.data_ptr() + band) % (2 * align)) % (2 * align)
    assert (base.data_ptr() + start) % (2 * align) == align and band <= start and start + nbytes + band <= base.numel()
    return base, start


def _view(base, start, shape, dtype):
    n = 1
    for s in shape:
        n *= int(s)
    return base[start:start + n * torch.empty((), dtype=dtype).element_size()].view(dtype).view(tuple(shape))


def _finish(base, start, shape, dtype, nbytes):
    t = _view(base, start, shape, dtype)
    e = _Extent()
    e.base, e.start, e.nbytes = base, start, nbytes
    e.front, e.back = base[:start].clone(), base[start + nbytes:].clone()
    t._extent = e
    return t


def _nbytes(shape, dtype):
    n = torch.empty((), dtype=dtype).element_size()
    for s in shape:
        n *= int(s)
    return n


_SEED = [0]


def _noise(n, device):
    """seeded pseudo-random bytes (another stream per call, the same streams in every run)"""
    _SEED[0] += 1
    g = torch.Generator().manual_seed(0x5EED0000 + _SEED[0])
    return torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g).to(device)


def guarded(shape, dtype, device, fill, align=16):
    """A view of `shape` / `dtype` inside a larger allocation: data_ptr() % (2 * align) == align, a band of
    max(4096, nbytes) bytes (at most 1 MiB) of seeded pseudo-random bytes on either side, of which the harness keeps a copy.
    fill: a byte value for every byte of the view, or a tensor of the view's shape and type with its initial values."""
    shape = tuple(int(s) for s in shape)
    nbytes = _nbytes(shape, dtype)
    base, start = _carve(nbytes, device, align, torch.empty((), dtype=dtype).element_size())
    base.copy_(_noise(base.numel(), device))
    if isinstance(fill, torch.Tensor):
        assert tuple(fill.shape) == shape and fill.dtype == dtype, "initial values of another shape or type"
        _view(base, start, shape, dtype).copy_(fill)
    else:
        base[start:start + nbytes] = int(fill)
    return _finish(base, start, shape, dtype, nbytes)


def embedded(tensor, band_byte, align=16, device=None):
    """The values of `tensor` as an input view whose bands hold `band_byte` in every byte."""
    device = tensor.device if device is None else device
    shape, dtype = tuple(tensor.shape), tensor.dtype
    nbytes = _nbytes(shape, dtype)
    base, start = _carve(nbytes, device, align, tensor.element_size())
    base.fill_(int(band_byte))
    _view(base, start, shape, dtype).copy_(tensor)
    return _finish(base, start, shape, dtype, nbytes)


def band_damage(g):
    """None, or (first, last) changed byte offset RELATIVE TO THE VIEW'S END (negative: in front of the view's start, counted from
    its end all the same, so that one number line serves both bands)"""
    e = g._extent
    bad = []
    for band, origin, now in ((e.front, -e.nbytes - e.start, e.base[:e.start]), (e.back, 0, e.base[e.start + e.nbytes:])):
        diff = (band != now).nonzero()
        if diff.numel():
            bad += [origin + int(diff[0]), origin + int(diff[-1])]
    return (min(bad), max(bad)) if bad else None


def assert_bands_intact(g, what):
    d = band_damage(g)
    if d is not None:
        n = g._extent.nbytes
        where = lambda o: f"{o} bytes behind the view's end" if o >= 0 else f"{-o - n} bytes in front of the view's start" if o < -n else "inside?"
        raise AssertionError(f"{what}: bytes outside the {n}-byte view changed; first changed byte at offset {d[0]} from the view's end "
                             f"({where(d[0])}), last at {d[1]} ({where(d[1])})")


def as_ints(t):
    return t.contiguous().view(_INT_VIEW[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and torch.equal(as_ints(a).cpu(), as_ints(b).cpu())


def first_difference(a, b):
    d = (as_ints(a).cpu().reshape(-1) != as_ints(b).cpu().reshape(-1)).nonzero()
    return f"{d.numel()} of {a.numel()} elements differ, first at flat index {int(d[0])}, last at {int(d[-1])}"


# ------------------------------------------------------------------------------------------------------------------------------
# tagged arguments
# ------------------------------------------------------------------------------------------------------------------------------
class Arg:
    """kind: "in" (values), "out" (shape, dtype: its documented extent), "inout" (initial values), "ws" (bytes: exactly what the
    size function returns).  align: the alignment the entry point documents or checks for this pointer.  compare: the number of
    leading elements (or the flat element ranges [(start, stop), ..]) whose values are a result -- the rest of the extent is scratch
    or padding the header lets the kernel have: a dump row, a ring, statistics slots behind the last row, the alignment gaps of an
    opaque image; None: all of them."""

    def __init__(self, kind, value=None, shape=None, dtype=None, align=16, compare=None):
        self.kind, self.value, self.shape, self.dtype, self.align, self.compare = kind, value, shape, dtype, align, compare


def In(t, align=16):
    return Arg("in", value=t, align=max(align, t.element_size()))


def Out(shape, dtype, align=16, compare=None):
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    return Arg("out", shape=shape, dtype=dtype, align=max(align, torch.empty((), dtype=dtype).element_size()), compare=compare)


def InOut(t, align=16, compare=None):
    return Arg("inout", value=t, align=max(align, t.element_size()), compare=compare)


def Ws(nbytes, align=16):
    return Arg("ws", shape=(int(nbytes),), dtype=torch.uint8, align=align)


def _filled(shape, dtype, device, byte):
    return torch.full((_nbytes(shape, dtype),), byte, dtype=torch.uint8, device=device).view(dtype).view(tuple(shape))


def result_part(t, compare):
    """the elements of t whose values are a result: all (None), the first `compare`, or the flat ranges [(start, stop), ..]"""
    if compare is None:
        return t
    flat = t.reshape(-1)
    if isinstance(compare, int):
        return flat[:compare]
    return torch.cat([flat[a:b] for a, b in compare])


def materialise(spec, mode, device):
    """name -> tensor for one of the three surroundings: "P" plain tensors (outputs 0xff), "A" embedded / guarded with 0xff,
    "B" the same with 0x00.  None stays None (an absent optional argument)."""
    byte = 0x00 if mode == "B" else 0xff
    out = {}
    for name, a in spec.items():
        if a is None:
            out[name] = None
        elif a.kind == "in":
            out[name] = a.value.to(device).clone() if mode == "P" else embedded(a.value.to(device), byte, a.align)
        elif a.kind == "inout":
            out[name] = a.value.to(device).clone() if mode == "P" else guarded(a.value.shape, a.value.dtype, device, a.value.to(device), a.align)
        else:                                                    # out, ws
            out[name] = _filled(a.shape, a.dtype, device, byte) if mode == "P" else guarded(a.shape, a.dtype, device, byte, a.align)
    return out


def run_case(spec, call, device, sync=lambda: None, what=""):
    """The extent checks of one case.  `call(t)` makes the call from the dict of materialised tensors and returns its code.
      1  all three calls return 0
      2  after A and after B every band of every buffer -- outputs, workspaces, in-outs and inputs -- is intact
      3  every output and in-out result is bit-identical in P, A and B
      4  every input that is not in-out is unchanged
    Returns the three dicts (P, A, B)."""
    runs = {}
    for mode in ("P", "A", "B"):
        t = materialise(spec, mode, device)
        rc = call(t)
        sync()
        assert rc == 0, f"{what} [{mode}]: the call returned {rc}"
        runs[mode] = t
    for mode in ("A", "B"):
        for name, t in runs[mode].items():
            if t is not None:
                assert_bands_intact(t, f"{what} [{mode}] {spec[name].kind} `{name}`")
    for name, a in spec.items():
        if a is None:
            continue
        if a.kind == "in":
            for mode in ("P", "A", "B"):
                assert same_bits(runs[mode][name], a.value), f"{what} [{mode}]: the call changed its input `{name}`: " + \
                    first_difference(runs[mode][name], a.value)
        elif a.kind in ("out", "inout"):
            for x, y in (("A", "B"), ("P", "A")):
                rx, ry = result_part(runs[x][name], a.compare), result_part(runs[y][name], a.compare)
                assert same_bits(rx, ry), \
                    f"{what}: {a.kind} `{name}` differs between {x} and {y} " + \
                    ("(0xff against 0x00 around the inputs and in the outputs: an element never written, or a read past an input)"
                     if x == "A" else "(plain against guarded tensors: a dependence on alignment beyond the documented one)") + \
                    ": " + first_difference(rx, ry)
    return runs["P"], runs["A"], runs["B"]


def run_short(spec, call, device, sync=lambda: None, what="", codes=(-1, -2)):
    """The size argument one unit short (the caller's `call` passes it): the call must refuse with one of `codes` and leave every
    byte of every output, in-out and workspace, and of their bands, as it was."""
    t = materialise(spec, "A", device)
    before = {n: as_ints(v).clone() for n, v in t.items() if v is not None}
    rc = call(t)
    sync()
    assert rc in codes, f"{what}: one unit under the size the size function returns, the call returned {rc} (one of {codes} expected)"
    for n, v in t.items():
        if v is not None:
            assert torch.equal(as_ints(v), before[n]), f"{what}: the refused call changed `{n}`"
            assert_bands_intact(v, f"{what} (refused call) `{n}`")
