"""vqseg_adam_ema_step_f32 through the C ABI, on every path, against tests/optim_cases.py and tests/ema_cases.py:
  * p, m, v bit for bit against `adam_emulate` -- the averaging must not disturb the step;
  * e bit for bit against `ema_emulate` (average: fma(w, p' - e, e); copy: the bits of p'), NaNs by position;
  * every student image bit-equal to the NumPy layout of p', every teacher image to that of e', padding zero;
  * average-only records (g == NULL), records without an average (e == NULL), any order of the item table, copy_all;
  * the old and the new entry point on one table with every e NULL: the same bits;
  * every buffer between sentinel words that must survive; refused calls leave every payload untouched."""
import numpy as np
import pytest
import torch

from tests import ema_cases as E
from tests import optim_cases as C

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def lib():
    from vq_seg_amd import _hip
    return _hip.lib()


def _step(params, emas, hyper=C.HYPER, order="sorted", decay=E.DECAY, copy_all=0, label=""):
    rc = E.ema_launch(params, emas, C.adam_items(params, order, seed=5), hyper, decay, copy_all)
    assert rc == 0, (label, lib().vqseg_last_error())


def _check_record(P, Q, state, e0, copy, label, hyper=C.HYPER, decay=E.DECAY, c1=None):
    """one ordinary record after one launch: p, m, v, e, both image sets, the gradient and every guard -> (p', e')"""
    want = C.check_adam_emulation(P.results(), state, hyper, label)
    assert (C.f32_bits(P.buf["g"].get()) == C.f32_bits(state[1]).reshape(-1)).all(), f"{label}: the gradient was written"
    e_new = None
    if Q.e is not None:
        e_new = E.check_ema(Q.result(), e0, want[0], decay, copy, label)
    for who, imgs, src in (("student", P.img, want[0]), ("teacher", Q.img, e_new)):
        for name, img in C.expected_images(src, P.k, P.cout, P.cin, P.c1, tuple(imgs)).items():
            C.check_image(imgs[name].get(), img, f"{label}: {who} {name}", padding=C.image_padding(name, P.k, P.cout, P.cin))
    assert P.guards_intact() and Q.guards_intact(), f"{label}: a guard word was overwritten"
    return want[0], e_new


# ------------------------------------------------------------------------------------------------ flat records
ALIGNMENTS = {"e_shifted": (None, 1), "aligned": (None, 0), "all_shifted": ({"p": 1, "g": 1, "m": 1, "v": 1}, 1)}


@pytest.mark.parametrize("copy", [0, 1], ids=["average", "copy"])
@pytest.mark.parametrize("n", C.FLAT_NUMELS)
def test_flat_records_in_average_and_copy_mode_at_every_alignment(n, copy):
    """the f32x4 body with its tail (everything aligned) and the scalar body (e alone one float off; everything one float off):
    bit-equal to the emulations and to each other"""
    state, e0 = C.flat_state(n), E.ema_data(900 + n, n)
    runs = {}
    for name, (shift, e_shift) in ALIGNMENTS.items():
        P = C.AdamParam(dev(), state, shift=shift)
        Q = E.EmaParam(dev(), P, e0, copy=copy, shift=e_shift)
        assert (Q.e.ptr % 16 != 0) == bool(e_shift) and all((P.buf[k].ptr % 16 != 0) == bool(shift) for k in "pgmv")
        _step([P], [Q], label=(n, name))
        _check_record(P, Q, state, e0, copy, f"flat {n} {name}")
        runs[name] = P.results() + (Q.result(),)
    for name in ("e_shifted", "all_shifted"):
        for x, y in zip(runs[name], runs["aligned"]):
            assert (C.f32_bits(x) == C.f32_bits(y)).all(), f"flat {n}: {name} differs from the aligned run"


# ------------------------------------------------------------------------------------------------ convolution tiles
def _teacher_sets(cin):
    if cin % 32:
        return [((), None), (("fwd",), None), (("fwd", "tr"), None)]          # no split-3 image exists for these weights
    sets = [((), None), (("fwd",), None)]
    for c1 in C.s3_splits(cin):
        sets += [(("fwd", "s3"), c1), (("fwd", "tr", "s3"), c1)]
    return sets


@pytest.mark.parametrize("student_images", [True, False], ids=["student_all", "student_none"])
@pytest.mark.parametrize("k,cout,cin", [(3, a, b) for a, b in C.K3_SHAPES] + [(1, a, b) for a, b in C.K1_SHAPES])
def test_convolution_tiles_write_both_image_sets_from_one_lds_tile(k, cout, cin, student_images):
    state, e0 = C.tile_state(k, cout, cin), E.ema_data(1300 + 7 * k + 13 * cout + cin, cout * cin * k * k)
    for images, c1 in _teacher_sets(cin):
        mine = (("fwd", "tr", "s3") if cin % 32 == 0 else ("fwd", "tr")) if student_images else ()
        label = f"k{k} {cout}x{cin} student {mine or 'none'} teacher {images or 'none'} c1 {c1}"
        P = C.AdamParam(dev(), state, k=k, cout=cout, cin=cin, c1=c1 or (32 if "s3" in mine else cin), images=mine)
        Q = E.EmaParam(dev(), P, e0, images=images)
        _step([P], [Q], label=label)
        _check_record(P, Q, state, e0, 0, label)
    P = C.AdamParam(dev(), state, k=k, cout=cout, cin=cin, images=("fwd", "tr"))          # a copy record: the teacher's images are the student's
    Q = E.EmaParam(dev(), P, e0, copy=1, images=("fwd", "tr"))
    _step([P], [Q])
    _check_record(P, Q, state, e0, 1, f"k{k} {cout}x{cin} copy")
    for name in ("fwd", "tr"):
        assert (P.img[name].get() == Q.img[name].get()).all()


# ------------------------------------------------------------------------------------------------ average-only records
def _mixed_table(copy=0):
    """ordinary records with and without an average, average-only records (flat and tiled), a record with neither"""
    d = dev()
    specs = [dict(state=C.flat_state(8195)),
             dict(state=C.tile_state(1, 40, 129), k=1, cout=40, cin=129, images=("fwd", "tr")),
             dict(state=C.flat_state(5)),
             dict(state=C.tile_state(3, 40, 33), k=3, cout=40, cin=33, images=("fwd", "tr")),
             dict(state=C.flat_state(1027)),
             dict(state=C.tile_state(3, 64, 64), k=3, cout=64, cin=64, c1=32, images=("fwd", "tr", "s3")),
             dict(state=C.tile_state(1, 64, 256), k=1, cout=64, cin=256, c1=224, images=("s3",)),
             dict(state=C.flat_state(4097)),
             dict(state=C.tile_state(3, 33, 24), k=3, cout=33, cin=24)]
    params = [C.AdamParam(d, **s) for s in specs]
    e0 = [E.ema_data(2000 + i, P.numel) for i, P in enumerate(params)]
    emas = [E.EmaParam(d, params[0], e0[0], copy=copy),
            E.EmaParam(d, params[1], e0[1], copy=copy, images=("fwd", "tr")),
            E.EmaParam(d, params[2], None),                                              # e == NULL beside records with e
            E.EmaParam(d, params[3], None),
            E.EmaParam(d, params[4], e0[4], copy=copy, average_only=True),               # g == NULL: a running statistic
            E.EmaParam(d, params[5], e0[5], copy=copy, images=("fwd", "s3")),
            E.EmaParam(d, params[6], e0[6], copy=copy),
            E.EmaParam(d, params[7], None, average_only=True),                           # neither: nothing to do
            E.EmaParam(d, params[8], e0[8], copy=copy, images=("fwd", "tr"), average_only=True)]
    return specs, params, emas, e0


def _check_table(specs, params, emas, e0, copy, label):
    out = []
    for i, (s, P, Q) in enumerate(zip(specs, params, emas)):
        lab = f"{label} record {i}"
        if Q.average_only:
            assert P.untouched(), f"{lab}: an average-only record's p / g / m / v or student images were written"
            assert P.guards_intact() and Q.guards_intact(), lab
            if Q.e is not None:
                e_new = E.check_ema(Q.result(), e0[i], s["state"][0], E.DECAY, copy or Q.copy, lab)
                for name, img in C.expected_images(e_new, P.k, P.cout, P.cin, P.c1, tuple(Q.img)).items():
                    C.check_image(Q.img[name].get(), img, f"{lab}: teacher {name}", padding=C.image_padding(name, P.k, P.cout, P.cin))
        else:
            _check_record(P, Q, s["state"], e0[i], copy or Q.copy, lab)
        out.append(P.results() + tuple(P.img[n].get() for n in sorted(P.img)) + ((Q.result(),) if Q.e is not None else ())
                   + tuple(Q.img[n].get() for n in sorted(Q.img)))
    return out


def test_average_only_records_leave_p_alone_and_take_null_moments():
    """g == NULL: p read only, m / v NULL, e (and its images) produced -- alone in a table and (below) among ordinary records"""
    for n, shift in ((1027, 0), (4097, 1), (5, 0)):
        state, e0 = C.flat_state(n), E.ema_data(70 + n, n)
        P = C.AdamParam(dev(), state)
        Q = E.EmaParam(dev(), P, e0, average_only=True, shift=shift)
        _step([P], [Q])
        assert P.untouched() and P.guards_intact() and Q.guards_intact()
        E.check_ema(Q.result(), e0, state[0], E.DECAY, 0, f"average-only flat {n}")


@pytest.mark.parametrize("copy_all", [0, 1])
def test_mixed_table_in_any_order(copy_all):
    """records with e == NULL behave as under the old entry point, the others average (copy_all = 1: copy, overriding every
    record's copy = 0); sorted, reversed and shuffled item tables give the same bits"""
    results = {}
    for order in ("sorted", "reversed", "shuffled"):
        specs, params, emas, e0 = _mixed_table()
        assert all(Q.copy == 0 for Q in emas)
        _step(params, emas, order=order, copy_all=copy_all, label=order)
        results[order] = _check_table(specs, params, emas, e0, copy_all, f"table ({order}, copy_all {copy_all})")
    for order in ("reversed", "shuffled"):
        for a, b in zip(results[order], results["sorted"]):
            assert all((x.view(np.uint8) == y.view(np.uint8)).all() for x, y in zip(a, b)), order


def test_per_record_copy_flag():
    specs, params, emas, e0 = _mixed_table(copy=1)
    _step(params, emas)
    _check_table(specs, params, emas, e0, 1, "table (copy records)")


# ------------------------------------------------------------------------------------------------ values
@pytest.mark.parametrize("decay", [E.DECAY, 0.0, 0.999])
def test_special_values_follow_ieee_arithmetic(decay):
    """optim_cases.special_values() state crossed with +-0, subnormal, +-inf and NaN averages: the emulations' bits, NaN by position,
    through the vector and the scalar body"""
    state = C.special_values()
    e0 = E.special_e(state[0].size)
    runs = []
    for e_shift in (0, 1):
        P = C.AdamParam(dev(), state)
        Q = E.EmaParam(dev(), P, e0, shift=e_shift)
        _step([P], [Q], decay=decay)
        _check_record(P, Q, state, e0, 0, f"special values, decay {decay}, {'scalar' if e_shift else 'vector'} body", decay=decay)
        runs.append(Q.result())
    C.check_bits(runs[0], runs[1], "special values e: vector body against scalar body")


# ------------------------------------------------------------------------------------------------ both entry points
def test_every_e_null_is_the_old_entry_point_bit_for_bit():
    def table():
        specs = [dict(state=C.flat_state(8195)), dict(state=C.tile_state(1, 40, 129), k=1, cout=40, cin=129, images=("fwd", "tr")),
                 dict(state=C.flat_state(1023), shift={"m": 1}), dict(state=C.tile_state(3, 40, 33), k=3, cout=40, cin=33, images=("fwd", "tr")),
                 dict(state=C.tile_state(3, 64, 64), k=3, cout=64, cin=64, c1=32, images=("fwd", "tr", "s3")), dict(state=C.tile_state(3, 31, 8), k=3, cout=31, cin=8)]
        return [C.AdamParam(dev(), **s) for s in specs]

    old, new = table(), table()
    assert C.adam_launch(old, C.adam_items(old), C.HYPER) == 0
    _step(new, [E.EmaParam(dev(), P, None) for P in new])
    for i, (a, b) in enumerate(zip(old, new)):
        for name, x, y in zip("pmv", a.results(), b.results()):
            assert (C.f32_bits(x) == C.f32_bits(y)).all(), f"record {i}: {name} differs between the entry points"
        for name in a.img:
            assert (a.img[name].get() == b.img[name].get()).all(), f"record {i}: image {name} differs between the entry points"
        assert b.guards_intact()


# ------------------------------------------------------------------------------------------------ refused calls
def test_refused_calls_leave_every_buffer_untouched():
    L = lib()
    specs, params, emas, e0 = _mixed_table()
    items = C.adam_items(params)
    lr, b1, b2, eps, step = C.HYPER
    refused = [dict(hyper=(lr, b1, b2, eps, 0)), dict(hyper=(lr, 1.0, b2, eps, step)), dict(hyper=(lr, b1, 1.0, eps, step)),
               dict(hyper=(lr, b1, b2, -1e-8, step)), dict(null_params=True), dict(null_ema=True), dict(null_items=True), dict(n_items=0),
               dict(n_items=-3), dict(decay=-0.1), dict(decay=1.0), dict(decay=float("nan"))]
    for kw in refused:
        kw = dict(kw)
        hyper, decay = kw.pop("hyper", C.HYPER), kw.pop("decay", E.DECAY)
        assert E.ema_launch(params, emas, items, hyper, decay, **kw) == -1, (hyper, decay, kw)
        assert L.vqseg_last_error(), (hyper, decay, kw)
    assert all(P.untouched() and P.guards_intact() for P in params) and all(Q.untouched() and Q.guards_intact() for Q in emas)
    _step(params, emas)                                                   # and the same tables are served once the arguments are valid
    _check_table(specs, params, emas, e0, 0, "after the refused calls")
