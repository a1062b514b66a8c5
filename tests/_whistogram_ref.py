"""Host referee of rsx_segmented_weighted_histogram (no GPU, no library): the mass of every weight in numpy integers, unsigned (the rule of
rsx_segmented_weighted_select, _wselect_ref.mass_np) and signed, the S x B sums of the masses per (segment, bin) with the bin of
_histogram_ref.bins_of, and — from the layout alone — the path every piece of every tile takes in radix-sort_amd/csrc/rsx_wbins.hpp.

  signed_mass_np      int64 masses: mass_np; signed=True (float kinds): the mass of |w|, negated for a negative weight (NaN of either
                      sign and both zeros: 0; -inf: -2^31)
  whistogram_oracle   S x B int64 sums from bins_of and signed_mass_np, vectorised (exact_sums: integer sums through numpy.bincount, limb by limb)
  whistogram_loop     the same key by key, with Python integers and _histogram_ref.bins_loop
  piece_paths         _histogram_ref.piece_paths with THIS kernel's constants: 2048 bins in LDS, wave-private up to 512, direct pieces below
                      256 keys (_histogram_ref reads its module constants, which are the unweighted kernel's)
  lds_layout          'wave_private' / 'shared' / 'none' for B bins
  big_boundaries_layout  the two-tile layout of tests/test_gpu_whistogram_paths.py for a CU count
  case_weights        the float weights of the GPU tests: negatives, +-0, NaNs, +-inf and one weight at or above 2^weight_exp planted
                      inside the segments; uint32_weights the integer ones; large_case_weights the same for the largest uploads
The sums are compared as int64 words: an unsigned sum below 2^63 reads the same either way.
"""
import numpy as np

import _histogram_ref as H
from _histogram_ref import NO_BIN, TILE, bins_loop, bins_of
from _wselect_ref import kind_of, mass_np  # noqa: F401  (kind_of: for the tests that import this module)

LDS_MAX = 2048               # kWbinsLdsMax
WAVE_PRIVATE_MAX = 512       # kWbinsWavePrivateMax
DIRECT_PIECE = 256           # kBinsDirectPiece (inherited)
EDGES_MAX = 4096             # kWbinsEdgesMax
WHIST_SIGNED = 256


def signed_mass_np(w: np.ndarray, weight_exp: int = 0, signed: bool = False) -> np.ndarray:
    """int64 masses of a uint32 / float32 / float64 weight array, as the call adds them"""
    w = np.asarray(w)
    if w.dtype == np.uint32 or not signed:
        return mass_np(w, weight_exp).astype(np.int64)
    m = mass_np(np.abs(w), weight_exp).astype(np.int64)         # (|NaN| is a NaN: 0)
    return np.where(np.signbit(w), -m, m)


def mass_loop(w: np.ndarray, weight_exp: int = 0, signed: bool = False) -> list:
    """signed_mass_np, weight by weight, from the bits with Python integers: floor(sig * 2^sh) saturated at 2^31"""
    w = np.asarray(w)
    if w.dtype == np.uint32:
        return [int(v) for v in w]
    ebits, mbits = (8, 23) if w.dtype == np.float32 else (11, 52)
    bias = (1 << (ebits - 1)) - 1
    out = []
    for b in (int(v) for v in w.view(np.uint32 if w.dtype == np.float32 else np.uint64)):
        neg = b >> (ebits + mbits)
        e, m = (b >> mbits) & ((1 << ebits) - 1), b & ((1 << mbits) - 1)
        if (neg and not signed) or (e == 0 and m == 0) or (e == (1 << ebits) - 1 and m):
            out.append(0)
            continue
        if e == (1 << ebits) - 1:
            mag = 1 << 31
        else:
            sig = (m | (1 << mbits)) if e else m
            sh = (e if e else 1) - bias - mbits + 31 - int(weight_exp)
            mag = min(sig << sh if sh >= 0 else sig >> -sh, 1 << 31)
        out.append(-mag if neg else mag)
    return out


def whistogram_oracle(keys, weights, off, bins, lo=0, hi=0, shift=0, descending=False, weight_exp=0, signed=False) -> np.ndarray:
    """S x B int64: the sum of the masses of the keys of every segment per bin"""
    B = int(bins) if np.isscalar(bins) else len(bins) - 1
    o = H._offsets(keys.size, off)
    S = o.size - 1
    b = bins_of(keys, bins, lo, hi, shift, descending)
    m = signed_mass_np(weights, weight_exp, signed)
    seg = np.repeat(np.arange(S, dtype=np.int64), np.diff(o))
    live_b, live_m = b[o[0]:o[-1]], m[o[0]:o[-1]]
    ok = live_b != NO_BIN
    return exact_sums(seg[ok] * B + live_b[ok], live_m[ok], S * B).reshape(S, B)


def exact_sums(dest, m, size) -> np.ndarray:
    """int64 sums of the masses m (|m| < 2^32) per destination, exactly: numpy.bincount adds float64 weights, so each 16-bit limb of
    the magnitudes is summed on its own (at most 2^31 addends below 2^16: below 2^47, exact in a double) and the limbs are joined as
    integers"""
    m = np.asarray(m, dtype=np.int64)
    sign = np.where(m < 0, -1.0, 1.0)
    mag = np.abs(m)
    assert mag.size == 0 or int(mag.max()) < 1 << 32
    out = np.zeros(size, dtype=np.int64)
    for limb in range(2):
        part = np.bincount(dest, weights=sign * ((mag >> (16 * limb)) & 0xFFFF).astype(np.float64), minlength=size)
        out += part.astype(np.int64) << (16 * limb)
    return out


def whistogram_loop(keys, weights, off, bins, lo=0, hi=0, shift=0, descending=False, weight_exp=0, signed=False) -> np.ndarray:
    """whistogram_oracle, key by key"""
    B = int(bins) if np.isscalar(bins) else len(bins) - 1
    o = [int(v) for v in H._offsets(keys.size, off)]
    b = bins_loop(keys, bins, lo, hi, shift, descending)
    m = mass_loop(weights, weight_exp, signed)
    sums = [[0] * B for _ in range(len(o) - 1)]
    for s in range(len(o) - 1):
        for i in range(o[s], o[s + 1]):
            if b[i] != NO_BIN:
                sums[s][b[i]] += m[i]
    return np.array(sums, dtype=np.int64).reshape(len(o) - 1, B)


# -- the paths (rsx_wbins.hpp) ---------------------------------------------------------------------------------------------------------------

def piece_paths(n, off, B, cus=256):
    """[(tile, segment, length, path)] of every piece in the order wbins_tile_kernel meets them; the paths are _histogram_ref.piece_paths':
    'direct' (B > 2048 or fewer than 256 keys), 'lds_first', 'lds_same', 'lds_flush'"""
    o = H._offsets(n, off)
    chunk = H.chunk_of(n, cus)
    out = []
    acc, acc_group = None, None
    starts, ends = o[:-1], o[1:]
    for t in range((n + TILE - 1) // TILE):
        group = t // chunk
        if group != acc_group:
            acc, acc_group = None, group
        t0, t1 = t * TILE, (t + 1) * TILE
        first = int(np.searchsorted(ends, t0, side="right"))
        last = int(np.searchsorted(starts, t1, side="left"))
        for s in range(first, last):
            a, e = max(int(starts[s]), t0), min(int(ends[s]), t1)
            if a >= e:
                continue
            if B > LDS_MAX or e - a < DIRECT_PIECE:
                out.append((t, s, e - a, "direct"))
                continue
            out.append((t, s, e - a, "lds_first" if acc is None else "lds_same" if acc == s else "lds_flush"))
            acc = s
    return out


def piece_slots(n, off, B, cus=256):
    """[(tile, segment, length, path, slot)]: as _histogram_ref.piece_slots, from this module's piece_paths"""
    paths = piece_paths(n, off, B, cus)
    o = H._offsets(n, off)
    per_tile = np.bincount([p[0] for p in paths], minlength=1)
    out = []
    for t, s, L, path in paths:
        start = max(int(o[s]), t * TILE)
        out.append((t, s, L, path, None if path == "direct" or per_tile[t] == 1 else (start - t * TILE) // DIRECT_PIECE))
    return out


def big_boundaries_layout(cus=256):
    """(n, off): _histogram_ref.big_boundaries_layout for any CU count: n = (16 cus + 1) tiles + 5, so a workgroup of wbins_tile_kernel
    walks two tiles, with the same offsets relative to the tiles: off[0] and off[S] in mid-tile, a boundary in the middle of a
    workgroup's SECOND tile (tile 3: both pieces long), of its first tile (tile 8), and a short piece at a tile's end (tile 13)"""
    n = (16 * cus + 1) * TILE + 5
    return n, np.array([1000, 3 * TILE + 2000, 8 * TILE + 300, 13 * TILE + 4000, 14 * TILE + 50, n - 3], dtype=np.uint64)


def lds_layout(B):
    """'wave_private' or 'shared' or 'none': the counters of the LDS path for B bins"""
    return "none" if B > LDS_MAX else "wave_private" if B <= WAVE_PRIVATE_MAX else "shared"


# -- inputs --------------------------------------------------------------------------------------------------------------------------------------

WEIGHT_DTYPES = [np.uint32, np.float32, np.float64]
MATRIX_BINS = [1, 64, 513, 2048]
EVEN_SHIFT = {1: 5, 64: 3, 513: 1, 2048: 0}          # integer even form: B << shift values from lo on, inside the keys' span
PATH_BINS = [512, 513, 2048, 2049]                   # the last wave-private and the first shared size, the last LDS and the first direct size


def form_args(dt, form, descending, B, rng):
    """_histogram_ref.form_args with this module's shifts"""
    dt = np.dtype(dt)
    if form == "edges":
        return dict(bins=H.sorted_edges(rng, dt, B, H.SPAN * 3 // 4, descending), lo=0, hi=0, shift=0)
    if dt.kind == "f":
        return dict(bins=B, lo=H.FLOAT_LO, hi=H.FLOAT_HI, shift=0)
    return dict(bins=B, lo=-300 if dt.kind == "i" else 3700, hi=0, shift=EVEN_SHIFT.get(B, 0))


def specials(dt, weight_exp):
    """negatives, +-0, NaNs of both signs, +-inf, a weight of exactly 2^weight_exp and one above it (both saturate)"""
    dt = np.dtype(dt)
    one = np.ldexp(1.0, weight_exp)
    return np.array([-0.25 * one, -one, 0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, one, 3.0 * one, -3.0 * one], dtype=dt)


def case_weights(rng, wdt, n, off, weight_exp=0):
    """n weights of the dtype.  uint32: any word (masses up to 2^32 - 1), with zeros.  Floats: uniform in (-2^e, 2^e) and exact zeros
    everywhere, with specials() planted inside the segments."""
    wdt = np.dtype(wdt)
    if wdt == np.uint32:
        w = rng.integers(0, 1 << 32, n, dtype=np.uint32)
        w[rng.random(n) < 0.1] = 0
        return w
    w = ((rng.random(n) * 2.0 - 1.0) * np.ldexp(1.0, weight_exp)).astype(wdt)
    w[rng.random(n) < 0.1] = 0.0
    return H.scatter_into(rng, w, off, specials(wdt, weight_exp))


def large_case_weights(rng, wdt, n, off, weight_exp=0):
    """case_weights for the uploads of 2^24 elements and more: the same values, the float specials at random positions of
    [off[0], off[S]) that may coincide (scatter_into permutes the whole range to keep them apart)"""
    wdt = np.dtype(wdt)
    if wdt == np.uint32:
        return case_weights(rng, wdt, n, off)
    w = ((rng.random(n) * 2.0 - 1.0) * np.ldexp(1.0, weight_exp)).astype(wdt)
    w[rng.random(n, dtype=np.float32) < 0.1] = 0.0
    o = H._offsets(n, off)
    sp = np.tile(specials(wdt, weight_exp), 4)
    w[rng.integers(int(o[0]), int(o[-1]), sp.size)] = sp
    return w


def dyadic_weights(rng, n, dtype=np.float32):
    """multiples of 2^-20 in [-1, 1]: their float64 sums are exact, and so are their masses at weight_exp 0"""
    return (rng.integers(-(1 << 20), (1 << 20) + 1, n).astype(np.float64) / (1 << 20)).astype(dtype)


# name -> (layout, B, the paths its pieces must take: exactly this set), for THIS kernel's constants
LAYOUTS = {
    "ragged_lds": (H.ragged_layout, 64, {"direct", "lds_first", "lds_flush"}),
    "ragged_lds_2048": (H.ragged_layout, 2048, {"direct", "lds_first", "lds_flush"}),
    "ragged_direct_2049": (H.ragged_layout, 2049, {"direct"}),
    "ragged_direct_4096": (H.ragged_layout, 4096, {"direct"}),
    "ragged_direct_50257": (H.ragged_layout, 50257, {"direct"}),
    "one_segment_three_tiles": (lambda: (H.SKEW_N, None), 256, {"lds_first", "direct"}),
    "one_segment_three_tiles_2048": (lambda: (H.SKEW_N, None), 2048, {"lds_first", "direct"}),
    "one_segment_three_tiles_2049": (lambda: (H.SKEW_N, None), 2049, {"direct"}),
    "big_boundaries": (H.big_boundaries_layout, 256, {"lds_first", "lds_same", "lds_flush", "direct"}),
    "pairs": (H.pairs_layout, 16, {"direct"}),
    "empties": (H.empties_layout, 16, {"lds_first", "lds_flush"}),
    "fifties": (H.fifties_layout, 16, {"direct"}),
}
