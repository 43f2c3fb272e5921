"""Exact reference for the arithmetic of accumulator words (raytracingweekend.jl_amd/csrc/rtw_accum_kernels.hip; include/rtw_hip.h "Progressive
render", "Adaptive sampling"), in plain Python integers, Fractions and single binary64 operations.

An accumulator is 8 uint64 per pixel: (lo, hi) of the signed 64.64 sum of R, G and B, the poison count (word 6) and the signed half
difference in units of 2^-24 (word 7).  Merge, resolve, the adaptive stopping rule and the tile list are exact functions of those words;
this module is the checker's side of each, plus a builder of the export blob so that a test can hand the library any words it likes
(a blob has no checksum).  A helper module, not a conftest.py.

Arrays of words are ``H x W x 8`` uint64, ``words[i, j]`` = row i, column j -- what ``read_pixels`` returns; the device and the blob
keep pixel (i, j) at ``(j * H + i) * 8``."""
from fractions import Fraction
import random
import struct

import numpy as np

M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
TILE = 8


# ---- integers <-> words -------------------------------------------------------------------------------------------------------------
def split128(S):
    """a Python integer (any sign) -> (lo, hi) of its value mod 2^128"""
    S &= M128
    return S & M64, S >> 64


def signed128(lo, hi):
    v = int(lo) | (int(hi) << 64)
    return v - (1 << 128) if v >> 127 else v


def signed64(w):
    v = int(w)
    return v - (1 << 64) if v >> 63 else v


def make_words(width, height):
    return np.zeros((height, width, 8), np.uint64)


def set_pixel(words, i, j, rgb=(0, 0, 0), h=0, poison=0):
    """pixel (i, j): the three channel sums as integers in units of 2^-64, the half difference in units of 2^-24, the poison count"""
    for c, S in enumerate(rgb):
        words[i, j, 2 * c], words[i, j, 2 * c + 1] = split128(int(S))
    words[i, j, 6], words[i, j, 7] = int(poison) & M64, int(h) & M64


def fx(x):
    """a value that is a multiple of 2^-64 (a binary64 number, an int or a Fraction) -> the integer the words hold for it"""
    q = Fraction(x) * (1 << 64)
    assert q.denominator == 1, x
    return int(q)


def words_of_sums(sums, width, height):
    """``len(sums) <= 3 W H`` integers, spread over the pixels in the device's order (column by column) and their channels"""
    w = make_words(width, height)
    assert len(sums) <= 3 * width * height
    for k, S in enumerate(sums):
        pix, c = divmod(k, 3)
        j, i = divmod(pix, height)
        w[i, j, 2 * c], w[i, j, 2 * c + 1] = split128(int(S))
    return w


def device_order(a, per_pixel):
    """``H x W x per_pixel`` -> flat, pixel (i, j) at ``(j * H + i) * per_pixel``"""
    return np.ascontiguousarray(np.asarray(a).transpose(1, 0, 2)).reshape(-1)


def from_device_order(flat, width, height, per_pixel):
    return np.asarray(flat).reshape(width, height, per_pixel).transpose(1, 0, 2)


# ---- the export blob (rtw_accum.hip BlobHeader / rtw_accum.hpp AccumBind) -------------------------------------------------------------------------
#   char magic[8]; uint32 version, header_bytes; int32 width, height, bound, n_ranges;                     32 bytes
#   AccumBind: int32 is_f64, spp, chunk_spp, n_chunks, max_depth, numerics; uint64 seed, scene_hash;       40 bytes
#              unsigned char cam[sizeof(rtw_camera_f64)] (22 doubles; Float32: the first half, the rest 0) 176 bytes
#   n_ranges x (int32 begin, int32 end); width * height * 8 uint64, little endian
HEADER_BYTES = 248
CAM_BYTES = 176


def n_chunks_of(spp, chunk_spp):
    return (spp + chunk_spp - 1) // chunk_spp


def blob(width, height, words=None, *, is_f64=False, spp=1, chunk_spp=1, n_chunks=None, max_depth=16, numerics=0, seed=1, scene_hash=0,
         cam=b"", ranges=(), bound=None, version=1):
    """a blob as rtw_accum_export writes it.  ``ranges`` empty and ``bound`` None: an unbound accumulator (the binding is zeroed)."""
    ranges = [(int(b), int(e)) for b, e in ranges]
    if bound is None:
        bound = 1 if ranges else 0
    head = b"RTWACCUM" + struct.pack("<IIiiii", version, HEADER_BYTES, width, height, bound, len(ranges))
    if bound:
        cam = bytes(cam)
        assert len(cam) <= CAM_BYTES
        head += struct.pack("<iiiiiiQQ", int(bool(is_f64)), spp, chunk_spp, n_chunks_of(spp, chunk_spp) if n_chunks is None else n_chunks,
                            max_depth, numerics, seed, scene_hash) + cam + bytes(CAM_BYTES - len(cam))
    else:
        head += bytes(HEADER_BYTES - len(head))
    assert len(head) == HEADER_BYTES
    body = b"".join(struct.pack("<ii", b, e) for b, e in ranges)
    if words is None:
        words = make_words(width, height)
    words = np.asarray(words)
    assert words.shape == (height, width, 8) and words.dtype == np.uint64
    return np.frombuffer(head + body + device_order(words, 8).astype("<u8").tobytes(), np.uint8).copy()


def samples_held(ranges, spp, chunk_spp):
    """the samples of the chunk ranges [begin, end): chunks of ``chunk_spp`` samples, the last one short when spp is no multiple"""
    return sum(min(spp, e * chunk_spp) - min(spp, b * chunk_spp) for b, e in ranges)


def coalesce(ranges):
    out = []
    for b, e in sorted(ranges):
        if out and out[-1][1] == b:
            out[-1] = (out[-1][0], e)
        else:
            out.append((b, e))
    return out


# ---- resolve ------------------------------------------------------------------------------------------------------------------------
def sum_to_double(S):
    """the signed 64.64 sum as a binary64 number, one correctly rounded step (ties to even)"""
    return float(Fraction(int(S), 1 << 64))


def resolve(words, samples, gamma, T):
    """``H x W x 3`` of type T: sum -> binary64 (one rounding) -> / samples -> sqrt if gamma -> rounded to T; NaN where word 6 != 0.
    ``samples``: one divisor, or ``H x W`` of them."""
    words = np.asarray(words)
    H, W = words.shape[:2]
    v = np.empty((H, W, 3), np.float64)
    for i in range(H):
        for j in range(W):
            w = words[i, j]
            for c in range(3):
                v[i, j, c] = sum_to_double(signed128(w[2 * c], w[2 * c + 1]))
    v[words[..., 6] != 0] = np.nan
    div = np.broadcast_to(np.asarray(samples, np.float64).reshape((-1, 1, 1) if np.ndim(samples) == 0 else (H, W, 1)), v.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        v = v / div
        if gamma:
            v = np.sqrt(v)
        return v.astype(T)


def same_bits(a, b):
    """bit equality of two float arrays; NaNs are compared by position (the payload of a NaN is not part of the contract)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return bool(np.array_equal(na, nb) and np.array_equal(np.ascontiguousarray(a).view(u)[~na], np.ascontiguousarray(b).view(u)[~nb]))


def tile_divisors(chunks, width, height, spp, chunk_spp):
    """``H x W``: min(spp, C_t * chunk_spp) of each pixel's tile (``chunks``: C_t in tile order t = tj * tiles_i + ti)"""
    tiles_i = (height + TILE - 1) // TILE
    out = np.empty((height, width), np.int64)
    for i in range(height):
        for j in range(width):
            out[i, j] = min(spp, int(chunks[(j // TILE) * tiles_i + i // TILE]) * chunk_spp)
    return out


# ---- merge --------------------------------------------------------------------------------------------------------------------------
def merge(a, b):
    """dst += src: every channel mod 2^128, words 6 and 7 each mod 2^64 on their own -- no carry leaves a channel or a word"""
    a, b = np.asarray(a), np.asarray(b)
    out = np.empty_like(a)
    H, W = a.shape[:2]
    for i in range(H):
        for j in range(W):
            for c in range(3):
                S = (signed128(a[i, j, 2 * c], a[i, j, 2 * c + 1]) + signed128(b[i, j, 2 * c], b[i, j, 2 * c + 1])) & M128
                out[i, j, 2 * c], out[i, j, 2 * c + 1] = S & M64, S >> 64
            for k in (6, 7):
                out[i, j, k] = (int(a[i, j, k]) + int(b[i, j, k])) & M64
    return out


# ---- the sums a resolve has to get right ---------------------------------------------------------------------------------------------
def tie(M, s):
    """a sum that lies exactly half way between two binary64 numbers: a 53-bit significand M, the tie bit, ten zeros, shifted by s"""
    assert M >> 52 == 1
    return ((M << 11) | 0x400) << s


# even, even, odd (all ones), odd; and an even one that is itself half way between two binary32 numbers (the upper of them odd): the
# sticky bit of T + 1 then decides the Float32 result as well, through the second rounding
TIE_SIGNIFICANDS = [1 << 52, (1 << 52) + 0x5a5a5a5a5a5a4, (1 << 53) - 1, (1 << 52) + 0x3c3c3c3c3c3c3, (1 << 52) | (1 << 28)]


def resolve_classes(seed=7, n_random=300):
    """the list of 128-bit sums of the resolve tests: every class below and the negative of each value"""
    pos = [0, 1, 1 << 64]
    for b in range(127):                                            # every shift count of the normalisation
        pos += [1 << b, (1 << b) - 1, (1 << b) + 1]
    for M in TIE_SIGNIFICANDS:                                      # exact ties and their neighbours: the tie bit (bit s + 10) lies in lo
        for s in range(64):                                         # for s < 54 and in hi from there on; after the normalisation it is
            t = tie(M, s)                                           # bit 10 of hi, and what tells T + 1 from T lies in lo alone
            pos += [t, t + 1, t - 1]
    pos += [((1 << 64) - 1) << s for s in (0, 1, 31, 62, 63)]       # 64 ones: all-ones significand that rounds up into the next binade
    pos += [(1 << 127) - 1]
    rnd = random.Random(seed)
    for _ in range(n_random):
        pos.append(rnd.getrandbits(rnd.randint(1, 127)))
    out = []
    for S in pos:
        out += [S, -S]
    out += [-(1 << 127)]
    out += [signed128(1, M64), signed128(0, M64), signed128(0, (1 << 64) - 5), signed128(0, 1 << 63)]      # the negation's carry
    return out


# ---- the stopping rule: rtw_amd.adaptive.reference_decisions restated with ONE deliberate deviation at a time --------------------------
VARIANTS = ("pairwise", "butterfly", "reverse", "rgb_right", "exact_y", "clamp_tile", "strict", "floor_right", "npix_unpoisoned",
            "poison_counted", "h_truncated")


def _tree(x, strides):
    x = list(x)
    for d in strides:
        x = [x[l] + x[l ^ d] for l in range(64)]
    return x[0]


def _sum64(x, variant):
    if variant == "pairwise":                                       # neighbours first
        return _tree(x, (1, 2, 4, 8, 16, 32))
    if variant == "butterfly":                                      # halves first
        return _tree(x, (32, 16, 8, 4, 2, 1))
    s = 0.0
    for v in (reversed(x) if variant == "reverse" else x):
        s = s + v
    return s


def decisions(words, width, height, n, tol, floor, variant=None):
    """``converged[t]`` like ``reference_decisions`` (variant None: the rule as written), or the rule with one deviation:
    pairwise / butterfly / reverse -- D and Y summed in another order;  rgb_right -- R + (G + B);  exact_y -- the three channels added
    exactly and rounded once;  clamp_tile -- the tile's Y clamped at 0 instead of each pixel's;  strict -- D < tol M;
    floor_right -- floor * (n * npix);  npix_unpoisoned -- poisoned pixels not counted in npix;  poison_counted -- poisoned pixels
    not skipped;  h_truncated -- |H| -> binary64 rounded towards zero"""
    assert variant is None or variant in VARIANTS
    H, W = int(height), int(width)
    words = np.asarray(words)
    assert words.shape == (H, W, 8)
    tiles_i, tiles_j = (H + 7) // 8, (W + 7) // 8
    tol, floor, n = float(tol), float(floor), float(n)
    conv = []
    for tj in range(tiles_j):
        for ti in range(tiles_i):
            d, y = [0.0] * 64, [0.0] * 64
            npix = 0
            for l in range(64):
                i, j = ti * 8 + (l & 7), tj * 8 + (l >> 3)
                if i >= H or j >= W:
                    continue
                w = words[i, j]
                bad = int(w[6]) != 0
                if not (bad and variant == "npix_unpoisoned"):
                    npix += 1
                if bad and variant != "poison_counted":
                    continue
                m = abs(signed64(w[7]))
                if variant == "h_truncated" and m.bit_length() > 53:
                    m = (m >> (m.bit_length() - 53)) << (m.bit_length() - 53)
                d[l] = float(m) * 2.0 ** -24
                S = [signed128(w[2 * c], w[2 * c + 1]) for c in range(3)]
                r, g, b = (sum_to_double(s) for s in S)
                if variant == "rgb_right":
                    yp = r + (g + b)
                elif variant == "exact_y":
                    yp = float(Fraction(sum(S), 1 << 64))
                else:
                    yp = (r + g) + b
                y[l] = yp if variant == "clamp_tile" else max(yp, 0.0)
            D, Y = _sum64(d, variant), _sum64(y, variant)
            if variant == "clamp_tile":
                Y = max(Y, 0.0)
            dark = floor * (n * float(npix)) if variant == "floor_right" else (floor * n) * float(npix)
            M = max(Y, dark)
            conv.append(D < tol * M if variant == "strict" else D <= tol * M)
    return np.array(conv, dtype=bool)


# ---- hand-made frames for the stopping rule -------------------------------------------------------------------------------------------
def U(v):
    """an integer radiance sum in the words' units of 2^-64"""
    return int(v) << 64


def _case(name, width, height, words, tol, floor=0.0, c=2, cs=1, chunks=None, tile=0, opposite=()):
    n_tiles = ((height + 7) // 8) * ((width + 7) // 8)
    return dict(name=name, width=width, height=height, words=words, tol=float(tol), floor=float(floor), c=c, cs=cs,
                chunks=np.full(n_tiles, c, np.int64) if chunks is None else np.asarray(chunks, np.int64), tile=tile, opposite=tuple(opposite))


RAGGED_NPIX = [64, 40, 24, 15]                   # the tiles of 13 rows x 11 columns, t = tj * 2 + ti


def _ragged(extra):
    w = make_words(11, 13)
    for t, npix in enumerate(RAGGED_NPIX):
        set_pixel(w, 8 * (t & 1), 8 * (t >> 1), h=(npix << 24) + extra)
    return w


def stopping_cases():
    """Frames on which the rule as written and ONE named deviation from it (``opposite``) decide tile ``tile`` differently; the case's
    docstring-like name says what it pins.  Every number below is a power of two or a short sum of them, so every step can be followed
    by hand: d_p = |H_p| 2^-24, y_p = max((R + G) + B, 0), D and Y summed from lane 0 upwards, M = max(Y, (floor n) npix), converged
    iff D <= tol M."""
    cases = []
    # D in lane order: 2^38 + 2^-15 is a tie that falls back to 2^38, 63 times; any order that adds two small terms first gets above it
    w = make_words(8, 8)
    for l in range(64):
        set_pixel(w, l & 7, l >> 3, h=(1 << 9) * (-1 if l & 1 else 1))
    set_pixel(w, 0, 0, rgb=(U(1 << 38), 0, 0), h=1 << 62)
    cases.append(_case("D_in_lane_order", 8, 8, w, 1.0, opposite=("pairwise", "butterfly", "reverse", "strict")))
    # Y in lane order: 2^53 + 1 falls back to 2^53, 63 times.  tol M = 2^33 < D = 2^33 + 2^-19 <= 2^-20 (2^53 + 62)
    w = make_words(8, 8)
    for l in range(64):
        set_pixel(w, l & 7, l >> 3, rgb=(U(1), 0, 0))
    set_pixel(w, 0, 0, rgb=(U(1 << 53), 0, 0), h=(1 << 57) + 32)
    cases.append(_case("Y_in_lane_order", 8, 8, w, 2.0 ** -20, opposite=("pairwise", "butterfly", "reverse")))
    # (R + G) + B = 2^53, R + (G + B) = 2^53 + 2; D = 2^33 + 2^-19 lies above the one product and on the other
    w = make_words(1, 1)
    set_pixel(w, 0, 0, rgb=(U(1 << 53), U(1), U(1)), h=(1 << 57) + 32)
    cases.append(_case("R_plus_G_first", 1, 1, w, 2.0 ** -20, opposite=("rgb_right", "exact_y")))
    # every channel is rounded to binary64 before the sum: R = 2^53 + 1 -> 2^53, G = 1 - 2^-64 -> 1, their sum -> 2^53; exactly: 2^53 + 2
    w = make_words(1, 1)
    set_pixel(w, 0, 0, rgb=(U((1 << 53) + 1), U(1) - 1, 0), h=(1 << 57) + 32)
    cases.append(_case("channels_rounded_before_the_sum", 1, 1, w, 2.0 ** -20, opposite=("exact_y",)))
    # the clamp is per pixel: y = 10 and y = -4 -> Y = 10, not 6; D = 8
    w = make_words(8, 8)
    set_pixel(w, 0, 0, rgb=(U(10), 0, 0), h=8 << 24)
    set_pixel(w, 1, 0, rgb=(-U(4), 0, 0))
    cases.append(_case("clamp_per_pixel", 8, 8, w, 1.0, opposite=("clamp_tile",)))
    # a poisoned pixel adds nothing to D and Y ...
    w = make_words(8, 8)
    set_pixel(w, 0, 0, rgb=(U(10), 0, 0), h=8 << 24)
    set_pixel(w, 2, 3, rgb=(U(5), 0, 0), h=1 << 40, poison=1)
    cases.append(_case("poisoned_pixel_skipped", 8, 8, w, 1.0, opposite=("poison_counted",)))
    # ... but counts in npix: D = 63.5 against (1 * 1) * 64
    w = make_words(8, 8)
    set_pixel(w, 0, 0, h=127 << 23)
    set_pixel(w, 2, 3, poison=3)
    cases.append(_case("poisoned_pixel_in_npix", 8, 8, w, 1.0, floor=1.0, c=1, opposite=("npix_unpoisoned",)))
    # (floor n) npix = (1.3 * 3) * 15 = 58.50000000000001, not 1.3 * 45 = 58.5: D = 2^23 * 58.50000000000001 exactly, in the 5 x 3 corner tile
    dark = (1.3 * 3.0) * 15.0
    assert dark != 1.3 * (3.0 * 15.0)
    h = Fraction(dark) * (1 << 47)
    assert h.denominator == 1 and h < 1 << 53
    w = make_words(11, 13)
    set_pixel(w, 8, 8, h=-int(h))
    cases.append(_case("floor_times_n_first", 11, 13, w, 2.0 ** 23, floor=1.3, c=3, tile=3, opposite=("floor_right", "strict")))
    # equality is converged; the next tolerance below is not
    w = make_words(8, 8)
    set_pixel(w, 0, 0, rgb=(U(100), U(100), U(200)), h=100 << 24)
    cases.append(_case("equality_converges", 8, 8, w, 0.25, opposite=("strict",)))
    cases.append(_case("below_equality", 8, 8, w, float(np.nextafter(0.25, 0.0))))
    # |H| -> binary64 is rounded to nearest: 2^63 - 1 -> 2^63, D = 2^39 > Y = 2^39 - 2^-14; and H = -2^63 itself, D = Y = 2^39
    w = make_words(8, 8)
    set_pixel(w, 0, 0, rgb=((1 << 103) - (1 << 50), 0, 0), h=-((1 << 63) - 1))
    cases.append(_case("H_most_negative_plus_one", 8, 8, w, 1.0, opposite=("h_truncated",)))
    w = make_words(8, 8)
    set_pixel(w, 0, 0, rgb=(U(1 << 39), 0, 0), h=-(1 << 63))
    cases.append(_case("H_most_negative", 8, 8, w, 1.0, opposite=("strict",)))
    # |H| = 2^53 + 1 is a tie that falls to 2^53 (D = 2^29 = Y); 2^53 + 3 is one that goes up to 2^53 + 4
    # (D = 2^29 + 2^-22 > Y = 2^29 + 2^-23, which is what 2^53 + 2 would give)
    w = make_words(8, 8)
    set_pixel(w, 7, 7, rgb=(0, U(1 << 29), 0), h=-((1 << 53) + 1))
    cases.append(_case("H_above_2p53_tie", 8, 8, w, 1.0, opposite=("strict",)))
    w = make_words(8, 8)
    set_pixel(w, 7, 7, rgb=(0, U(1 << 29) + (1 << 41), 0), h=(1 << 53) + 3)
    cases.append(_case("H_above_2p53_up", 8, 8, w, 1.0, opposite=("h_truncated",)))
    # ragged frames: every tile against its OWN npix, at equality and one unit of H above it
    cases.append(_case("ragged_at_equality", 11, 13, _ragged(0), 1.0, floor=1.0, c=1))
    cases.append(_case("ragged_above_equality", 11, 13, _ragged(1), 1.0, floor=1.0, c=1))
    w = make_words(1, 1)
    set_pixel(w, 0, 0, h=4 << 24)
    cases.append(_case("one_pixel_at_equality", 1, 1, w, 1.0, floor=0.5, c=4, cs=2))
    w = make_words(1, 1)
    set_pixel(w, 0, 0, h=(4 << 24) + 1)
    cases.append(_case("one_pixel_above_equality", 1, 1, w, 1.0, floor=0.5, c=4, cs=2))
    # a tile at another chunk count is not looked at, however noisy
    cases.append(_case("other_chunk_counts", 11, 13, _ragged(1 << 50), 1.0, floor=1.0, c=4, chunks=[4, 6, 2, 4]))
    return cases


def random_words(width, height, seed):
    """words of every kind at once: sums of both signs with bits below binary64's, half differences of both signs, a few poisoned pixels"""
    rnd = random.Random(seed)
    w = make_words(width, height)
    for i in range(height):
        for j in range(width):
            rgb = [rnd.getrandbits(rnd.randint(60, 84)) * (-1 if rnd.random() < 0.1 else 1) for _ in range(3)]
            h = rnd.getrandbits(rnd.randint(30, 44)) * rnd.choice((-1, 1))
            set_pixel(w, i, j, rgb=rgb, h=h, poison=1 if rnd.random() < 0.03 else 0)
    return w
