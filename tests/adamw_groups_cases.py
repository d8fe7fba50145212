"""Cases, layouts and the tile lookup of the table-driven AdamW tests (csrc/optim.hip: adamw4_table_kernel through dclip_adamw_table,
the host image through dclip_adamw_table_fill; FusedAdamW(groups=...)).  tests/test_adamw_groups_gpu.py runs them on the device,
tests/test_adamw_groups_cpu.py holds the host side and the lookup.

YARDSTICK.  The table entry must leave p, g, m, v, e bit for bit what the existing entries (dclip_adamw_multi, _scaled, _amp, _ema) leave
when they are called range by range with lr_k = float32(lr) * float32(lr_scale_k) and wd_k: no tolerance enters; those entries are
themselves held to float64 by tests/test_adamw_exact_gpu.py, and the grouped result is held to tests/adamw_cases.py's bound once
more, with each range's own hyper-parameters.

KERNEL CONSTANTS the lengths straddle: a lane moves 4 elements (one float4), the workgroup's 256 lanes one TRIP = 1024 elements, 8 trips
make a TILE = 8192 elements (DCLIP_ADAMW_TABLE_TILE), and every range starts a new tile.  LENGTHS: one lane (4), two lanes (8), a partly
filled workgroup (252), exactly one trip (1024), one trip + 4, exactly one tile (8192), one tile + 4, three tiles + 4 (24 580)."""
import functools

import numpy as np

import adamw_cases as ac

LANE, TRIP, TILE = 4, 1024, 8192
LENGTHS = (4, 8, 252, 1024, 1028, 8192, 8196, 24580)
SCALES = (0.0, 0.1, 1.0, 3.0)
WDS = (0.0, 0.01, 0.3)
COUNTS = (1, 7, 25, 70)
GAPS = (4, 64, 0, 12)                                   # frozen elements between neighbouring ranges (0: two ranges that touch)
GUARD, GUARD_BITS = ac.GUARD, ac.GUARD_BITS             # GUARD f32 words = 16 bytes
NAMES = 'pgmve'
RECORD = np.dtype([('tile0', '<i8'), ('begin', '<i8'), ('length', '<i8'), ('lr_scale', '<f4'), ('weight_decay', '<f4')])
assert RECORD.itemsize == 32


@functools.lru_cache(maxsize=None)
def ranges_of(count, lead=8):
    """-> ((begin, length, lr_scale, weight_decay), ...) ascending, total: `count` ranges inside one flat buffer of `total` elements with
    frozen gaps between them (and before the first, after the last).  Lengths, scales and decays cycle with periods 8, 4 and 3, so
    every length meets every pair within 96 ranges and the first 7 already differ pairwise; count = 1 takes the three-tile length."""
    out, at = [], lead
    for k in range(count):
        n = LENGTHS[-1] if count == 1 else LENGTHS[(k * 3 + 5) % len(LENGTHS)]      # (3 and 8 are coprime: all eight lengths, mixed)
        out.append((at, n, SCALES[(k if count > 1 else 3) % len(SCALES)], WDS[((k if count > 1 else 4) // 2) % len(WDS)]))   # (count = 1: 3 and 0.3)
        at += n + GAPS[k % len(GAPS)]
    return tuple(out), at + 4


def lr_of(lr, scale):
    """lr_k as the header states it: ONE f32 product of the two f32 values"""
    return float(np.float32(lr) * np.float32(scale))


def hyper_of(rng, h=ac.HYPER):
    """tests/adamw_cases.py's hyper tuple of one range"""
    lr, b1, b2, eps, _ = h
    return (lr_of(lr, rng[2]), b1, b2, eps, float(np.float32(rng[3])))


# ---- the tile list and the kernel's lookup ---------------------------------------------------------------------------------------------------
def tile0_of(ranges):
    """first tile of every range, + the number of tiles: every range starts a new tile"""
    t = [0]
    for _, n, _, _ in ranges:
        t.append(t[-1] + (n + TILE - 1) // TILE)
    return t


def lookup(tile0, t):
    """adamw4_table_kernel's bisection: the k with tile0[k] <= t < tile0[k + 1], for 0 <= t < tile0[count]"""
    lo, hi = 0, len(tile0) - 1
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if tile0[mid] <= t:
            lo = mid
        else:
            hi = mid
    return lo


def tile_span(ranges, tile0, t):
    """-> (k, first element, elements) workgroup t works on"""
    k = lookup(tile0, t)
    b, n = ranges[k][0], ranges[k][1]
    first = (t - tile0[k]) * TILE
    return k, b + first, min(n - first, TILE)


# ---- guarded buffers: GUARD NaN words | the flat buffer of `total` elements | GUARD NaN words --------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(count, fam='normal', seed=5):
    """-> {name: f32 [total], read-only} for p, g, m, v, e and the family's multiplier (or None): every element of the flat buffer holds
    data, the frozen gaps too, so that a gap written by mistake shows"""
    ranges, total = ranges_of(count)
    p, g, m, v, gs = ac.shared_family(fam, total, seed=seed)
    e = (p + 1e-3 * np.random.RandomState(seed).randn(total)).astype(np.float32)
    e.setflags(write=False)
    return dict(p=p, g=g, m=m, v=v, e=e), gs


def guarded(flat):
    buf = np.full(GUARD + flat.size + GUARD, GUARD_BITS, dtype=np.uint32).view(np.float32)
    buf[GUARD:GUARD + flat.size] = flat
    return buf


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def inside_mask(ranges, total):
    mask = np.zeros(total, dtype=bool)
    for b, n, _, _ in ranges:
        assert not mask[b:b + n].any()
        mask[b:b + n] = True
    return mask
