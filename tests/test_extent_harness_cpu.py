"""The extent harness (tests/extent.py) can fail: stand-in "kernels" written with torch indexing on CPU tensors that deliberately
write one element past the view, one before it, leave the last element unwritten, or read one element past an input are each
caught by the check meant for them, through the same run_case the GPU suite uses; a correct stand-in passes all checks."""
import pytest
import torch

from tests import extent as E
from tests import extent_cases

CPU = torch.device("cpu")
DTYPES = [torch.float32, torch.bfloat16, torch.int64, torch.uint8]


def _window(t, before, after):
    """t's elements with `before` elements in front and `after` behind it, through the storage t is a view of"""
    flat = t.reshape(-1)
    return flat.as_strided((flat.numel() + before + after,), (1,), flat.storage_offset() - before)


def _flip(window, i):
    """invert every bit of element i (whatever the band holds there, it changes)"""
    ints = window.view(E._INT_VIEW[window.element_size()])
    ints[i] = ~ints[i] if ints.dtype != torch.uint8 else 255 - ints[i]


def _values(n, dtype):
    v = torch.arange(1, n + 1, dtype=torch.float32) * 0.37 - 3
    return v.to(dtype) if dtype.is_floating_point else (torch.arange(1, n + 1) % 200).to(dtype)


def _spec(n, dtype, align=16):
    return {"x": E.In(_values(n, dtype), align), "y": E.Out((n,), dtype, align)}


def double_correct(t):
    t["y"].copy_(t["x"] + t["x"])
    return 0


def _plain(t):
    """run P hands the stand-ins ordinary tensors with nothing around them to reach: there they behave"""
    return not hasattr(t["y"], "_extent")


def double_writes_one_past(t):
    double_correct(t)
    if _plain(t):
        return 0
    _flip(_window(t["y"], 0, 1), -1)
    return 0


def double_writes_one_before(t):
    double_correct(t)
    if _plain(t):
        return 0
    _flip(_window(t["y"], 1, 0), 0)
    return 0


def double_leaves_last_unwritten(t):
    t["y"][:-1] = (t["x"] + t["x"])[:-1]
    return 0


def double_reads_one_past(t):
    """the last element takes the element behind the input instead of its own"""
    if _plain(t):
        return double_correct(t)
    xs = _window(t["x"], 0, 1)
    t["y"].copy_(xs[:-1] + torch.cat([xs[:-2], xs[-1:]]))
    return 0


def double_writes_its_input(t):
    double_correct(t)
    t["x"][0] = 0
    return 0


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[1] for d in DTYPES])
@pytest.mark.parametrize("n", [1, 5, 1025])
def test_correct_stand_in_passes_every_check(n, dtype):
    p, a, b = E.run_case(_spec(n, dtype), double_correct, CPU, what="correct")
    assert E.same_bits(p["y"], _values(n, dtype) + _values(n, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[1] for d in DTYPES])
@pytest.mark.parametrize("n", [1, 5, 1025])
@pytest.mark.parametrize("kernel,message", [
    (double_writes_one_past, r"bytes outside .* first changed byte at offset 0 from the view's end \(0 bytes behind"),
    (double_writes_one_before, r"bytes outside .* bytes in front of the view's start"),
    (double_leaves_last_unwritten, r"`y` differs between A and B .*first at flat index {last}, last at {last}"),
    (double_reads_one_past, r"`y` differs between A and B .*first at flat index {last}, last at {last}"),
    (double_writes_its_input, r"changed its input `x`"),
], ids=["one-past", "one-before", "last-unwritten", "reads-one-past", "writes-input"])
def test_each_planted_fault_is_caught(kernel, message, n, dtype):
    with pytest.raises(AssertionError, match=message.format(last=n - 1)):
        E.run_case(_spec(n, dtype), kernel, CPU, what=kernel.__name__)


def test_case_table_is_complete():
    """every entry point of the list has a ragged and a smallest case (no GPU needed: the table is built on import)"""
    extent_cases.check_table()


def test_one_past_names_the_changed_bytes():
    """the report gives the first and last changed byte relative to the view's end: a 4-byte element directly behind it"""
    spec = _spec(7, torch.float32)
    t = E.materialise(spec, "A", CPU)
    double_correct(t)
    assert E.band_damage(t["y"]) is None
    _flip(_window(t["y"], 0, 1), -1)
    first, last = E.band_damage(t["y"])
    assert (first, last) == (0, 3)
    _flip(_window(t["y"], 1, 0), 0)
    assert E.band_damage(t["y"]) == (-7 * 4 - 4, 3)


@pytest.mark.parametrize("dtype,align", [(d, a) for d in DTYPES for a in (4, 8, 16, 64) if a >= torch.empty((), dtype=d).element_size()])
def test_views_have_the_stated_alignment_and_no_better(dtype, align):
    for make in (lambda: E.guarded((3, 5), dtype, CPU, 0xff, align), lambda: E.embedded(_values(15, dtype).reshape(3, 5), 0x00, align)):
        g = make()
        assert g.data_ptr() % (2 * align) == align
        e = g._extent
        assert e.nbytes == 15 * g.element_size() and e.front.numel() >= E.BAND_MIN and e.back.numel() >= E.BAND_MIN
        E.assert_bands_intact(g, "fresh")


def test_band_sizes_and_fills():
    assert E.band_bytes(1) == 4096 and E.band_bytes(5000) == 5000 and E.band_bytes(3 << 20) == 1 << 20
    g = E.guarded((8,), torch.float32, CPU, 0xff)
    assert torch.isnan(g).all()
    back = g._extent.back
    assert len(set(back[:4096].tolist())) > 100, "the bands must not hold a constant"
    h = E.guarded((8,), torch.float32, CPU, 0xff)
    assert not torch.equal(h._extent.back[:4096], back[:4096]), "every buffer gets another stream"
    x = E.embedded(torch.arange(8, dtype=torch.float32), 0xff)
    assert torch.isnan(_window(x, 1, 1)[[0, -1]]).all()
    i = E.embedded(torch.arange(8), 0xff)
    assert _window(i, 1, 1)[[0, -1]].tolist() == [-1, -1]
    u = E.embedded(torch.arange(8, dtype=torch.uint8), 0xff)
    assert _window(u, 1, 1)[[0, -1]].tolist() == [255, 255]
    z = E.embedded(torch.arange(8, dtype=torch.float32), 0x00)
    assert _window(z, 1, 1)[[0, -1]].tolist() == [0, 0]
    io = E.guarded((8,), torch.float32, CPU, torch.arange(8, dtype=torch.float32))
    assert io.tolist() == list(range(8))


def test_same_bits_treats_nan_as_equal_and_signed_zero_as_different():
    nan = torch.full((3,), float("nan"))
    assert E.same_bits(nan, nan.clone()) and not torch.equal(nan, nan.clone())
    assert not E.same_bits(torch.zeros(1), -torch.zeros(1))
    assert not E.same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.int32))


def test_short_size_check_catches_a_call_that_goes_ahead():
    spec = {"x": E.In(_values(4, torch.float32)), "y": E.Out((4,), torch.float32), "w": E.Ws(64)}
    E.run_short(spec, lambda t: -1, CPU, what="refuses")
    E.run_short(spec, lambda t: -2, CPU, what="refuses")
    with pytest.raises(AssertionError, match="returned 0"):
        E.run_short(spec, double_correct, CPU, what="goes ahead")

    def refuses_late(t):
        t["w"][0] = 7
        return -1
    with pytest.raises(AssertionError, match="refused call changed `w`"):
        E.run_short(spec, refuses_late, CPU, what="late")
