"""Shared by the photometric tests: the definition of include/vqseg.h (vqseg_photometric_f) restated in numpy -- `photometric64`, all
arithmetic in float64 (THE yardstick: no parity with torchvision or PIL is claimed), and `photometric32`, the same formulas with every
operation rounded to float32 (used only to size the error bar: how far honest float32 arithmetic lands from the float64 result) -- the
test images, and the case table.  What both take from the float32 world, as the kernel does: the input pixels, the parameter row
rounded to float32, and the float32 taps (made in float64 on the host, rounded once)."""
import functools

import numpy as np

from vq_seg_amd import _hip

IDENTITY = (1.0, 1.0, 1.0, 0.0, 0.0, 0.0)


def taps_of(sigma):
    """(R, float32 taps w_-R .. w_R) of a (float32) sigma"""
    t = _hip.photometric_taps(float(np.float32(sigma)))
    return (len(t) - 1) // 2, t


def _gray(r, g, b, T):
    return T(0.299) * r + T(0.587) * g + T(0.114) * b


def _clamp(v, T):
    return np.minimum(np.maximum(v, T(0)), T(1))


def hue_step(r, g, b, hue, T):
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    v, cr = mx, mx - mn
    flat = cr == 0
    s = np.where(flat, T(0), cr / np.where(flat, T(1), mx))
    d = np.where(flat, T(1), cr)
    rc, gc, bc = (mx - r) / d, (mx - g) / d, (mx - b) / d
    h6 = np.where(mx == r, bc - gc, np.where(mx == g, T(2) + rc - bc, T(4) + gc - rc))
    h = h6 / T(6) + T(1)
    h = h - np.floor(h)
    h = h + T(hue)
    h = h - np.floor(h)                                     # (x mod 1 = x - floor(x))
    fi = np.floor(T(6) * h)
    f = T(6) * h - fi
    i = fi.astype(np.int64) % 6
    p_, q, t = _clamp(v * (T(1) - s), T), _clamp(v * (T(1) - f * s), T), _clamp(v * (T(1) - (T(1) - f) * s), T)
    pick = lambda opts: np.choose(i, opts)
    return pick([v, q, p_, p_, t, v]), pick([t, v, v, q, p_, p_]), pick([p_, p_, t, v, v, q])


def blur_step(x, taps, r, T):
    """(3, h, w): rows first, then columns, reflect-101.  float64: the plain sum over i in [-R, R]; float32: the kernel's documented
    order (the two taps of equal weight first, pairs from the outermost inwards), each operation rounded"""
    w = taps.astype(T)
    for axis in (2, 1):
        pad = [(0, 0)] * 3
        pad[axis] = (r, r)
        p = np.pad(x, pad, mode="reflect")
        n = x.shape[axis]
        take = lambda o: np.take(p, np.arange(r + o, r + o + n), axis=axis)
        if T is np.float64:
            x = sum(w[r + o] * take(o) for o in range(-r, r + 1))
        else:
            acc = np.zeros_like(x)
            for k in range(r, 0, -1):
                acc = acc + w[r + k] * (take(-k) + take(k))
            x = acc + w[r] * take(0)
    return x


def _photometric(x, params, T):
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4 and x.shape[1] == 3
    rows = np.asarray(params, dtype=np.float32)
    assert rows.shape == (x.shape[0], 6)
    out = np.empty(x.shape, dtype=T)
    means = np.zeros(x.shape[0], dtype=T)
    for s_ in range(x.shape[0]):
        b, c, sat, hue, gray, sigma = (T(v) for v in rows[s_])
        r, g, bl = (x[s_, k].astype(T) for k in range(3))
        if b != 1:
            r, g, bl = (_clamp(b * p, T) for p in (r, g, bl))
        if c != 1:
            m = means[s_] = _gray(r, g, bl, T).mean(dtype=T) if T is np.float64 else T(_gray(r, g, bl, T).astype(np.float64).mean())
            r, g, bl = (_clamp(c * p + (T(1) - c) * m, T) for p in (r, g, bl))
        if sat != 1:
            gr = _gray(r, g, bl, T)
            r, g, bl = (_clamp(sat * p + (T(1) - sat) * gr, T) for p in (r, g, bl))
        if hue != 0:
            r, g, bl = hue_step(r, g, bl, hue, T)
        if gray != 0:
            r = g = bl = _gray(r, g, bl, T)
        y = np.stack([r, g, bl])
        if sigma != 0:
            rad, taps = taps_of(rows[s_, 5])
            y = blur_step(y, taps, rad, T)
        assert y.dtype == T
        out[s_] = y
    return out, means


def photometric64(x, params, return_means=False):
    out, means = _photometric(x, params, np.float64)
    return (out, means) if return_means else out


def photometric32(x, params):
    return _photometric(x, params, np.float32)[0]


# ---- images ---------------------------------------------------------------------------------------------------------------------------

SPECIALS = ([(v, v, v) for v in (0.25, 0.5, 0.8125)] +                                            # exact grays
            [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)] +                  # primaries and secondaries: ties of max
            [(0, 0, 0), (1, 1, 1)] +                                                               # black, white
            [(0.7, 0.7, 0.2), (0.7, 0.2, 0.7), (0.2, 0.7, 0.7), (0.3, 0.3, 0.9), (0.3, 0.9, 0.3), (0.9, 0.3, 0.3)])     # two equal channels


def images(n, h, w, seed):
    """(n, 3, h, w) float32, uniform in [0, 1], with SPECIALS seeded in at spread-out pixels of every sample"""
    rng = np.random.default_rng([seed, n, h, w])
    x = rng.random((n, 3, h, w)).astype(np.float32)
    at = np.linspace(0, h * w - 1, len(SPECIALS)).astype(np.int64)
    flat = x.reshape(n, 3, h * w)
    for p, rgb in zip(at, SPECIALS):
        flat[:, :, p] = np.asarray(rgb, dtype=np.float32)
    return x


# ---- cases: name -> (n, h, w, rows) ----------------------------------------------------------------------------------------------------

def _row(**kw):
    r = dict(b=1.0, c=1.0, sat=1.0, hue=0.0, gray=0.0, sigma=0.0)
    r.update(kw)
    return (r["b"], r["c"], r["sat"], r["hue"], r["gray"], r["sigma"])


ALL_A, ALL_B = _row(b=1.3, c=0.7, sat=1.4, hue=0.2, sigma=1.5), _row(b=0.6, c=1.4, sat=0.5, hue=-0.4, gray=1.0, sigma=0.7)


def _chunk_rows(n):
    """varied rows for the parameter-chunk case (8 x 8 images: R <= 7, so sigma <= 2 is admissible)"""
    rng = np.random.default_rng(77)
    rows = []
    for s_ in range(n):
        u = rng.random(8)
        rows.append(IDENTITY if s_ % 7 == 3 else
                    (0.5 + u[0], 0.5 + u[1], 0.5 + u[2], u[3] - 0.5, float(u[4] < 0.3), 0.1 + 1.9 * u[5] if u[6] < 0.6 else 0.0))
    return rows


CASES = {}
for _name, _vals in (("b", (0.5, 1.5)), ("c", (0.5, 1.5)), ("sat", (0.5, 1.5)), ("hue", (-0.25, 0.25, 0.5)), ("gray", (1.0,)), ("sigma", (0.1, 0.7, 2.0))):
    for _v in _vals:
        CASES[f"{_name}={_v}"] = (1, 17, 70, [_row(**{_name: _v})])              # each op alone, both ends of its range; partial tiles
CASES["reflect limit 7x9 sigma=2"] = (1, 7, 9, [_row(sigma=2.0)])                 # R = 6 = H - 1
CASES["reflect limit 7x9 all ops"] = (2, 7, 9, [_row(b=1.3, c=0.7, sat=1.4, hue=0.2, sigma=2.0), ALL_B])
CASES["all ops 17x70"] = (2, 17, 70, [ALL_A, ALL_B])                              # partial tiles both ways, a halo across the column seam at x = 64
CASES["all ops 33x130"] = (2, 33, 130, [ALL_A, ALL_B])                            # three tile rows and columns, seams at y = 16, 32 and x = 64, 128
CASES["mean strides 96x160"] = (1, 96, 160, [_row(b=0.8, c=0.6, sat=1.2, hue=-0.1, sigma=1.0)])      # 4 mean workgroups, 15 values per thread
CASES["identity / colour / blur"] = (3, 17, 70, [IDENTITY, _row(b=1.2, c=0.8, sat=1.3, hue=0.1, gray=0.0), _row(sigma=1.2)])
CASES["a sigma per sample"] = (3, 17, 70, [_row(c=1.2, sigma=0.4), _row(sat=0.7, sigma=1.1), _row(hue=0.3, sigma=2.0)])
CASES["parameter chunks n=65"] = (65, 8, 8, _chunk_rows(65))                     # launches of 32 samples: seams at 32 and 64 (and BATCH_ARG_SAMPLES = 64)
CASE_NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (x float32, rows, out64, means64, bar32): computed once, shared, never modified.  bar32 = max |photometric32 - photometric64|"""
    n, h, w, rows = CASES[name]
    x = images(n, h, w, seed=len(name) + h)
    out64, means64 = photometric64(x, rows, return_means=True)
    bar32 = float(np.abs(photometric32(x, rows).astype(np.float64) - out64).max())
    for a in (x, out64, means64):
        a.setflags(write=False)
    return x, rows, out64, means64, bar32
