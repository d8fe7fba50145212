"""Cases, float64 reference, bound and guarded buffers of the EMA tests (csrc/optim.hip: adamw4_multi_kernel<MODE, EMA = true> through
dclip_adamw_multi_ema, swap4_multi_kernel through dclip_swap_multi).  tests/test_ema_gpu.py runs them on the device, tests/test_ema_cpu.py
holds the reference and the bound to an f32 emulation of the kernel's two roundings.

REFERENCE.  Per element, in float64, from the f32 average e before the call, the f32 parameter p' the call wrote (read back) and the
f32 weight w = float32(1 - decay) the C ABI passes:

    e' = e + w (p' - e)

BOUND.  include/dclip.h states the arithmetic: d = p' - e rounded to f32, then e' = fmaf(w, d, e), one rounding; d == 0 gives e itself.
With u = 2^-24 the first rounding moves w d by at most u |w d|, the second the result by at most u |e'|:

    |e' - (e + w (p' - e))| <= u (|w (p' - e)| + |e'|) (1 + 4 u) + S

which is the issue's bound u (2 |w (p' - e)| + |e'|) (1 + 4 u) with the rounding of a separate product taken out, since there is none.
(1 + 4 u) pays for the second-order terms and for |e'| being the reference's; S = 2^-149, one smallest subnormal, pays for a result
that is subnormal (a difference of two f32 is exact when it is subnormal; the fused multiply-add's result is not).  The inputs keep
every result normal all the same: magnitudes between 2^-20 and 2^20, w >= 2^-24 or 0.

EXACT.  w == 0 and p' == e leave e as it is, bit for bit; w == 1 gives e' = e + d with d = p' - e rounded, which is p' whenever the
difference is exact (cases `ulp`, `equal`) and within the bound otherwise."""
import functools

import numpy as np

import adamw_cases as ac

U, S = 2.0 ** -24, 2.0 ** -149
GUARD, GUARD_BITS = ac.GUARD, ac.GUARD_BITS
NAMES = 'pgmve'


def weight(decay):
    """float32(1 - decay), the subtraction in double: what FusedAdamW passes"""
    return float(np.float32(1.0 - float(decay)))


WEIGHTS = (0.0, 2.0 ** -24, weight(0.9999), 0.5, 1.0)
FAMILIES = ('wide', 'far', 'ulp', 'opposite', 'equal')
LENS5 = (4, 8, 1020, 1024, 1028)


def reference(e, p2, w):
    e, p2 = np.asarray(e, dtype=np.float64), np.asarray(p2, dtype=np.float64)
    return e + float(w) * (p2 - e)


def bound(e, p2, w):
    e, p2 = np.asarray(e, dtype=np.float64), np.asarray(p2, dtype=np.float64)
    return U * (np.abs(float(w) * (p2 - e)) + np.abs(reference(e, p2, w))) * (1 + 4 * U) + S


def ratio(got, e, p2, w):
    """largest |got - reference| / bound and where"""
    r = np.abs(np.asarray(got, dtype=np.float64) - reference(e, p2, w)) / bound(e, p2, w)
    r = np.where(np.isnan(r), np.inf, r)
    i = int(np.argmax(r))
    return float(r[i]), i


def _fma(a, b, c):
    """f32 fused multiply-add, correctly rounded: the product of two f32 is exact in float64; the sum is formed in float64 rounded to
    odd (its error term, exact by the two-sum, sets the last bit when it is not zero), which the rounding to f32 then cannot see twice"""
    x, c = a.astype(np.float64) * b.astype(np.float64), c.astype(np.float64)
    s = x + c
    t = s - x
    err = (x - (s - t)) + (c - t)
    even = (s.view(np.uint64) & np.uint64(1)) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def emulate(e, p2, w, fma=True):
    """the kernel in numpy f32: d = p' - e rounded, then one fused multiply-add; or with fma=False a rounded product and a rounded sum,
    which the issue's wider bound covers and this module's does not promise"""
    f = np.float32
    e, p2 = np.ascontiguousarray(e, dtype=f), np.ascontiguousarray(p2, dtype=f)
    with np.errstate(all='ignore'):
        d = p2 - e
        out = _fma(np.full_like(d, f(w)), d, e) if fma else e + f(w) * d
    return np.where(d == 0, e, out)


def _mag(r, n, lo=-20.0, hi=20.0):
    return np.exp2(r.uniform(lo, hi, size=n))


def _signs(r, n):
    return r.randint(0, 2, size=n) * 2.0 - 1.0


@functools.lru_cache(maxsize=None)
def family(name, n, seed=0):
    """-> e, p (f32 [n], read-only): the average before the call and the parameter the call is to write"""
    r = np.random.RandomState(100 * seed + FAMILIES.index(name))
    f = np.float32
    e = (_signs(r, n) * _mag(r, n)).astype(f)
    if name == 'wide':
        p = (_signs(r, n) * _mag(r, n)).astype(f)
    elif name == 'far':                                  # 2^30 and more apart in magnitude, either way round
        e = (_signs(r, n) * np.where(np.arange(n) % 2 == 0, _mag(r, n, 15, 20), _mag(r, n, -20, -15))).astype(f)
        p = (_signs(r, n) * np.where(np.arange(n) % 2 == 0, _mag(r, n, -20, -15), _mag(r, n, 15, 20))).astype(f)
    elif name == 'ulp':                                  # one ulp up or down
        p = np.nextafter(e, np.where(r.randint(0, 2, size=n) == 1, f(np.inf), f(-np.inf)).astype(f))
    elif name == 'opposite':                             # -e exactly in every other element, -e within 1e-3 in the rest
        p = (-e.astype(np.float64) * np.where(np.arange(n) % 2 == 0, 1.0, 1 + 1e-3 * r.randn(n))).astype(f)
    elif name == 'equal':
        p = e.copy()
    else:
        raise KeyError(name)
    assert e.dtype == p.dtype == f and np.isfinite(e).all() and np.isfinite(p).all()
    e.setflags(write=False)
    p.setflags(write=False)
    return e, p


# ---- guarded buffers: GUARD NaN words | range 0 | GUARD words | range 1 | ... | GUARD words, every range on a 16-byte boundary -----------------
def layout(lens):
    assert all(n % 4 == 0 for n in lens)
    spans, at = [], GUARD
    for n in lens:
        spans.append((at, at + n))
        at += n + GUARD
    return spans, at


def guarded(flat, lens):
    """flat: f32 [sum(lens)] -> the guarded buffer (f32, NaN guard words with a payload), spans"""
    spans, total = layout(lens)
    buf = np.full(total, GUARD_BITS, dtype=np.uint32).view(np.float32)
    at = 0
    for (a, b), n in zip(spans, lens):
        buf[a:b] = flat[at:at + n]
        at += n
    return buf, spans


def inside(buf, spans):
    return np.concatenate([buf[a:b] for a, b in spans])


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def lens24():
    """24 ranges of mixed length, one of them so long that the grid-stride loop of a 24-range launch takes three trips, the last one
    ragged -> lens (elements), the stride S in float4, the long range's length in float4"""
    S = ac.stride4(24, 10 ** 7)
    long4 = 2 * S + 77
    assert S == 341 * 256 and ac.stride4(24, long4) == S and 2 * S < long4 < 3 * S and long4 % 256 != 0
    lens4 = [1, 2, 255, 256, 257, 1000, long4, 3, 5, 17, 64, 100, 300, 511, 512, 513, 7, 9, 33, 129, 1023, 1024, 1025, 2049]
    assert len(lens4) == 24
    return [4 * n for n in lens4], S, long4
