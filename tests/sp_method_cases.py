"""Adversarial inputs for the stand-alone Spatial Pooler methods (tests/test_hip_sp_methods.py on the device,
tests/test_sp_methods_cpu.py for the host-side twin of the select key): arrays of boosted overlaps laid out so that a
top-k select which loses low mantissa bits, or exponents outside a narrow range, or the difference between a tiny value and
zero, returns a DIFFERENT SET than `oracle.htm_oracle.stable_topk`.

The device breaks ties towards the lower index, so wherever two values are close -- or become equal once information is
lost -- the LARGER one sits at the HIGHER index: "a tie, the lower index wins" is then the wrong answer.

Pure NumPy; nothing here touches a device."""

import numpy as np

from oracle.htm_oracle import stable_topk

SIZES = (63, 257, 1000, 4097)          # below one 256-column block, just above one, several, above 4096 (16 blocks + 1 column)
LOW_BITS = 23                          # mantissa bits a select may believe to be zero (an engine of input_dim 32: 26 key bits)


def k_values(C):
    return sorted({1, min(40, C - 1), C - 1})


CASES = [(C, k) for C in SIZES for k in k_values(C)]


def mask_low(x, bits=LOW_BITS):
    """x with the low `bits` mantissa bits of every double cleared: what a select sees that ignores them."""
    return (np.asarray(x, dtype=np.float64).view(np.uint64) & ~np.uint64((1 << bits) - 1)).view(np.float64)


def _plant_group(x, k, rng):
    """Make the values of ranks k-2 .. k+1 (descending, 0-based: the cut is between ranks k-1 and k) agree in everything but
    their low LOW_BITS mantissa bits, ascending with the index."""
    C = len(x)
    order = np.argsort(-x, kind="stable")
    ranks = np.arange(max(0, k - 2), min(C, k + 2))
    idx = np.sort(order[ranks])
    base = (np.float64(x[order[k - 1]]).view(np.uint64) & ~np.uint64((1 << LOW_BITS) - 1))
    low = np.sort(rng.choice(np.arange(1, 1 << LOW_BITS), size=len(idx), replace=False)).astype(np.uint64)
    x[idx] = (base + low).view(np.float64)
    return x


def full_mantissa(C, k, seed=0):
    """Family 1: RandomState(seed).rand(C) -- 53 random bits each -- with a group of near-equal values across the cut."""
    rng = np.random.RandomState(seed + 1000 * C + k)
    return _plant_group(rng.rand(C), k, rng)


def adjacent_doubles(C, k, seed=0, ramp=False):
    """Family 2: 1 + j * 2^-52 for a seeded permutation of j = 0 .. C-1 (or ascending: the answer is the last k indices)."""
    perm = np.arange(C) if ramp else np.random.RandomState(seed + 1000 * C + k).permutation(C)
    return 1.0 + perm * 2.0 ** -52


def near_tie_products(n_draws=20000, seed=0):
    """(f1, o1, f2, o2) with float32 factors and integer overlaps whose exact float64 products differ, agree above their low
    LOW_BITS mantissa bits and differ by less than 2^-30 of their size: f2 = float32(f1 * o1 / o2) for o1, o2 = 1022, 1023.
    Returns the two product arrays (p1[i], p2[i] a pair), products in [1, 2^17)."""
    rng = np.random.RandomState(seed)
    f1 = (rng.rand(n_draws) * 100.0 + 0.01).astype(np.float32)
    o1, o2 = 1022, 1023
    f2 = (f1.astype(np.float64) * o1 / o2).astype(np.float32)
    p1, p2 = f1.astype(np.float64) * o1, f2.astype(np.float64) * o2          # exact: 24-bit x 10-bit
    ok = (p1 != p2) & (np.abs(p1 - p2) < np.maximum(p1, p2) * 2.0 ** -30) & (mask_low(p1) == mask_low(p2)) & (p1 >= 1) & (p1 < 2 ** 17)
    return p1[ok], p2[ok]


def reference_shaped(C, k, pairs, seed=0):
    """Family 3: every value is float32 x integer.  As many near-tie pairs as fit, one of them split by the cut; whole numbers
    near 2^17 above them and multiples of 2^-12 below 1 (a zero among them) fill the rest."""
    p1, p2 = pairs
    rng = np.random.RandomState(seed + 1000 * C + k)
    n = min(len(p1), (C - 1) // 2)
    pick = rng.choice(len(p1), n, replace=False)
    big, small = np.maximum(p1[pick], p2[pick]), np.minimum(p1[pick], p2[pick])
    order = np.argsort(-big, kind="stable")
    big, small = big[order], small[order]
    assert (small[:-1] > big[1:]).all() if n > 1 else True, "pairs overlap each other"
    j = min(n - 1, (k - 1) // 2)                   # the pair the cut splits: k - 1 values rank above its larger member
    n_high = k - 1 - 2 * j
    n_low = C - n_high - 2 * n
    assert n_high >= 0 and n_low >= 0
    high = 131072.0 - np.arange(n_high)            # > 126975 > every pair (f1 < 100.02, o <= 1023)
    low = np.arange(n_low) * 2.0 ** -12            # < 1
    pos = rng.permutation(C)
    x = np.empty(C)
    x[pos[:n_high]] = high
    x[pos[n_high + 2 * n:]] = low
    pa, pb = pos[n_high:n_high + 2 * n:2], pos[n_high + 1:n_high + 2 * n:2]
    x[np.maximum(pa, pb)] = big                    # the larger member at the higher index
    x[np.minimum(pa, pb)] = small
    return x


TINY = np.array([5e-324, 1e-323, 2.0 ** -1070, 2.0 ** -1022, 2.0 ** -1000, 1e-300, 2.0 ** -500, 2.0 ** -362, 2.0 ** -200, 1e-60,
                 2.0 ** -151, np.nextafter(2.0 ** -150, 0), 2.0 ** -150, 2.0 ** -150, np.nextafter(2.0 ** -150, 1), 2.0 ** -149])


def tiny_values(C, k, extra=0, seed=0):
    """Family 4: exact zeros at the LOWEST indices, then k + extra nonzero values: tiny ones (5e-324 .. 2^-149, ascending with
    the index) and ordinary ones.  extra = 0: the cut falls between the tiny values and the zeros.  extra > 0: the `extra`
    smallest tiny values lose, and they sit below the other nonzero values."""
    rng = np.random.RandomState(seed + 1000 * C + k)
    nnz = min(C, k + extra)
    n_tiny = max(1, min(nnz, max(len(TINY), nnz // 2)))
    tiny = np.sort(TINY[np.arange(n_tiny) % len(TINY)] * (1.0 + (np.arange(n_tiny) // len(TINY)) * 2.0 ** -20))
    tiny[:min(n_tiny, 2)] = TINY[:min(n_tiny, 2)]                          # (a denormal times 1 + 2^-20 is itself)
    ordinary = rng.rand(nnz - n_tiny) * 100.0 + 2.0 ** -20
    x = np.zeros(C)
    x[C - nnz:C - nnz + n_tiny] = tiny
    x[C - nnz + n_tiny:] = ordinary
    return x


def huge_values(C, k, seed=0):
    """Family 5: values up to the largest double among ordinary ones and a few zeros; the huge ones ascend with the index."""
    rng = np.random.RandomState(seed + 1000 * C + k)
    x = rng.rand(C) * 1000.0
    x[rng.choice(C, max(1, C // 16), replace=False)] = 0.0
    n_huge = min(C // 2, 96)
    fixed = np.array([2.0 ** 106, 2.0 ** 107, 2.0 ** 361, np.nextafter(2.0 ** 362, 0), 2.0 ** 362, 2.0 ** 363, 1e300, 2.0 ** 1023,
                      np.finfo(np.float64).max])
    e = rng.randint(107, 1024, size=n_huge)
    huge = np.ldexp(1.0 + rng.rand(n_huge), e - 1)
    huge[:min(n_huge, len(fixed))] = fixed[:min(n_huge, len(fixed))]
    x[np.sort(rng.choice(C, n_huge, replace=False))] = np.sort(huge)
    return x


def signed_zeros(C, k, seed=0):
    """Family 6: -0.0 and +0.0 interleaved at the low indices, fewer than k positive values above them: the cut falls inside the
    zeros, which are all equal -- the lower index goes first, whatever its sign."""
    rng = np.random.RandomState(seed + 1000 * C + k)
    n_pos = k // 2
    x = np.zeros(C)
    x[:C - n_pos:2] = -0.0
    if C - n_pos > 3:
        x[1], x[2] = -0.0, 0.0                    # (not only an alternation)
    x[C - n_pos:] = rng.rand(n_pos) + 2.0 ** -30
    return x


def repeated_value(C, k):
    """Family 7a: one value repeated over up to 600 consecutive columns (three 256-column blocks and part of a fourth where C
    allows), larger and smaller values around them, the cut inside the group."""
    G = min(C - 1, 600)
    g0 = min(200, C - G)
    n_others = C - G
    above = min(n_others, max(0, k - G // 2))
    assert above < k < above + G
    others = np.r_[np.arange(g0), np.arange(g0 + G, C)]
    x = np.full(C, 7.25)
    x[others[:above]] = 8.0 + np.arange(above)
    x[others[above:]] = 0.5 + np.arange(n_others - above) * 2.0 ** -10
    return x


def extreme_span(C, k, seed=0):
    """Family 8: 5e-324 and 1e308 in one array, with everything between."""
    x = huge_values(C, k, seed + 1)
    t = tiny_values(C, k, extra=3, seed=seed + 1)
    x[::2] = t[::2]
    x[0], x[C - 1] = 1e308, 5e-324
    return x


def select_cases(C, k, pairs=None):
    """name -> array, every family at (C, k).  `pairs`: near_tie_products(), computed once by the caller."""
    out = {
        "1-full-mantissa": full_mantissa(C, k),
        "2-adjacent-doubles": adjacent_doubles(C, k),
        "2-adjacent-ramp": adjacent_doubles(C, k, ramp=True),
        "4-tiny-cut-at-zeros": tiny_values(C, k),
        "4-tiny-cut-inside": tiny_values(C, k, extra=3),
        "5-huge": huge_values(C, k),
        "6-signed-zeros": signed_zeros(C, k),
        "7-repeated": repeated_value(C, k),
        "7-all-equal": np.full(C, 3.5),
        "7-all-zero": np.zeros(C),
        "8-extreme-span": extreme_span(C, k),
    }
    if pairs is not None:
        out["3-reference-shaped"] = reference_shaped(C, k, pairs)
    return out


LOW_BIT_FAMILIES = ("1-full-mantissa", "2-adjacent-doubles", "2-adjacent-ramp", "3-reference-shaped")


def loses_without_low_bits(x, k):
    """The family's point: a select blind to the low mantissa bits (ties to the lower index) returns another set."""
    return not np.array_equal(stable_topk(x, k), stable_topk(mask_low(x), k))
