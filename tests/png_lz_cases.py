"""Inputs of the LZ77 device encoder's tests (tests/test_png_lz.py on the restatement, tests/test_png_lz_device.py on the kernels): small
blocks whose tokens are written out by hand, and blocks built to reach every distance and length symbol.  TEST INFRASTRUCTURE."""
import numpy as np

import png_lz_np as Z
import png_np as P


def _b(text):
    return np.frombuffer(text.encode("latin-1") if isinstance(text, str) else bytes(text), np.uint8)


def unique_bytes(n, first=0):
    """n bytes in which no three consecutive bytes occur twice and no two neighbours are equal: the pairs (k % 125, 128 + k // 125) of a
    counter k from `first` on.  A low byte (< 125) and a high byte (>= 128) alternate, so a window is low-high-low or high-low-high and
    holds one whole pair, which names k.  Up to 32000 bytes; the values 125, 126 and 127 never occur."""
    k = np.arange(first, first + (n + 1) // 2)
    assert first + len(k) <= 16000
    return np.stack([k % 125, 128 + k // 125], axis=1).astype(np.uint8).reshape(-1)[:n]


# ---- tokens written out by hand: (name, bytes, stride, [("lit", byte) | ("match", length, distance)]) ---------------------------------------

def _lits(text):
    return [("lit", c) for c in _b(text).tolist()]


def far_three(distance):
    """abc, `distance` - 3 bytes of unique_bytes, abc, Q: the second abc is 3 bytes at `distance`"""
    return np.concatenate([_b("abc"), unique_bytes(distance - 3), _b("abcQ")])


HAND_CASES = (
    ("abcabcabcabc", _b("abcabcabcabc"), 0, _lits("abc") + [("match", 9, 3)]),
    # an overlapping match, d < M: the pair repeats into itself
    ("overlap", _b("xyxyxyxyxyxyxyxyxyxy!"), 0, _lits("xy") + [("match", 18, 2), ("lit", 33)]),
    # 300 zeros in rows of 100: at 259 the run (d = 1, which is prev's distance too) and the row above (d = 100) both reach the end
    ("tie_run_row", np.zeros(300, np.uint8), 100, [("lit", 0), ("match", 258, 1), ("match", 41, 1)]),
    # abc 100 times in rows of 6: at 261 prev (d = 3) and the row above (d = 6) both reach the end
    ("tie_prev_row", _b("abc" * 100), 6, _lits("abc") + [("match", 258, 3), ("match", 39, 3)]),
    # at 20 the last abc is 3 back and matches 3 bytes; the row above (d = 10) matches 7.  (At 17 abc is 7 back; at 27 hij is 20 back.)
    ("row_beats_prev", _b("abcdefghij" "abcdefgabc" "abcdefghij"), 10,
     _lits("abcdefghij") + [("match", 7, 10), ("match", 3, 7), ("match", 7, 10), ("match", 3, 20)]),
    # at 10 the row above (d = 7) matches nothing; prev (d = 10) matches abcd
    ("prev_beats_row", _b("abcdefg" "xyzabcd"), 7, _lits("abcdefgxyz") + [("match", 4, 10)]),
    # the match is cut by the block end
    ("cut_by_end", _b("abcabcab"), 0, _lits("abc") + [("match", 5, 3)]),
    # the last two positions have no prev, and nothing of length 3 fits: literals, with and without a row above
    ("last_two", _b("abcdab"), 0, _lits("abcdab")),
    ("last_two_row", _b("abcdab"), 4, _lits("abcdab")),
    ("far_4096", far_three(4096), 0, None),   # checked at position 4096 alone: ("match", 3, 4096)
    ("far_4097", far_three(4097), 0, None),   # ("lit", 'a') at 4097
)


def expected(case):
    """The hand-written tokens as png_lz_np.block_tokens spells them, with positions"""
    out, p = [], 0
    for t in case[3]:
        if t[0] == "lit":
            out.append(("lit", p, t[1]))
            p += 1
        else:
            out.append(("match", p, t[1], t[2]))
            p += t[1]
    return out


PREFIX = 4200   # a multiple of every stride of HAND_CASES


def prefixed(case):
    """(name, bytes, stride) of a hand-written case behind PREFIX bytes of a value none of them holds: the run costs a few bytes, so the
    block is a Huffman block and its bytes show the tokens; the case's own tokens are the same, PREFIX further on"""
    return "pre_" + case[0], np.concatenate([np.full(PREFIX, 200, np.uint8), case[1]]), case[2]


def across_blocks():
    """A block that ends in uvwxyz and a second block uvwxyzuvwxyz: its first six bytes have nothing to match in their own block"""
    first = np.resize(unique_bytes(32000), P.BLOCK)
    first[-6:] = _b("uvwxyz")
    return np.concatenate([first, _b("uvwxyzuvwxyz")])


# ---- coverage -----------------------------------------------------------------------------------------------------------------------------

# one length of every length symbol 257..285, and the top of a few ranges
ALL_LENGTHS = tuple(P.LENGTH_BASE) + (10, 18, 34, 66, 130, 257)
# The largest distance a taken match can have: a match at i needs i - D >= 0 and three bytes, so D <= i <= 32765, and at 32765 only three
# bytes are left, which are not taken at D > 4096: D <= 32764.  32767, and the top of symbol 29's range, cannot occur.
MAX_DISTANCE = P.BLOCK - 4
NEAR_DISTANCES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17, 24, 25, 32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 192, 193, 256, 257, 384, 385, 512)
FAR_SYMBOLS = tuple(range(18, 30))
FAR_FIRST, FAR_LAST = 513, 24577   # the low ends of symbols 18 and 29


def near_block():
    """Distances up to 512, symbols 0..17 at both ends of their ranges: for each, D fresh bytes, then L bytes that repeat them (a match
    that overlaps itself when L > D), then a byte that occurs nowhere else.  -> (bytes, [(L, D)])"""
    parts, want, k = [], [], 0
    for j, d in enumerate(NEAR_DISTANCES):
        length = ALL_LENGTHS[j % len(ALL_LENGTHS)]
        fresh = unique_bytes(d + (d & 1), k)[:d]
        k += (d + 1) // 2
        parts += [fresh, np.resize(fresh, length), np.array([125 + j % 3], np.uint8)]
        want.append((length, d))
    return np.concatenate(parts), want


def far_block():
    """A full block: unique bytes, then copies of disjoint pieces of them at distances of every symbol 18..29, each followed by a byte
    that occurs nowhere else; the last four bytes copy the first four: the largest distance there is.  -> (bytes, [(L, D)])"""
    lengths = [n for n in ALL_LENGTHS if n >= 4]
    jobs = [(None, FAR_FIRST)] + [(s, None) for s in FAR_SYMBOLS] + [(None, FAR_LAST)]
    jobs = [(lengths[(3 * j) % len(lengths)], s, d) for j, (s, d) in enumerate(jobs)]
    area = sum(n + 1 for n, _, _ in jobs) + 4
    start = P.BLOCK - area
    blk = np.zeros(P.BLOCK, np.uint8)
    blk[:start] = unique_bytes(start)
    used, want, p = [(0, 8)], [], start    # source intervals taken; the first bytes belong to the last match
    for j, (length, sym, dist) in enumerate(jobs):
        lo, hi = (dist, dist) if dist else (Z.DIST_BASE[sym], min(Z.DIST_BASE[sym] + (1 << Z.DIST_EXTRA[sym]) - 1, MAX_DISTANCE))
        for d in range(hi, lo - 1, -1):
            a, b = p - d, p - d + length + 1
            if a >= 0 and b <= start and all(b <= u or a >= v for u, v in used):
                break
        else:
            raise AssertionError(("no free source", j, length, sym, dist))
        used.append((a, b))
        blk[p:p + length] = blk[a:a + length]
        blk[p + length] = 125 + j % 3
        want.append((length, d))
        p += length + 1
    assert p == P.BLOCK - 4
    blk[p:] = blk[:4]
    want.append((4, MAX_DISTANCE))
    return blk, want


def coverage_cases():
    """(name, bytes, stride) of the blocks that together reach every symbol; test_png_lz.py asserts that they do"""
    rng = np.random.default_rng(77)
    return (("near", near_block()[0], 0), ("far", far_block()[0], 0), ("no_match", unique_bytes(4000), 0),
            ("one_distance", _b("abcabcabcabc" * 30), 0), ("stored", rng.integers(0, 256, 3000, dtype=np.uint8), 0))


def deflate_cases():
    """Every (name, bytes, stride) the deflate entry is asked for: the hand-written blocks, the block pair, the coverage blocks, and the
    sizes around a block with and without a stride"""
    rng = np.random.default_rng(78)
    out = [(c[0], c[1], c[2]) for c in HAND_CASES] + [prefixed(c) for c in HAND_CASES] + [("across_blocks", across_blocks(), 0)] + list(coverage_cases())
    for n in (1, 2, 3, 4, 32767, 32768, 32769, 65537):
        smooth = (np.cumsum(rng.integers(0, 3, n)) // 7 % 256).astype(np.uint8)   # long runs and repeats
        rows = np.resize(rng.integers(0, 4, 97, dtype=np.uint8), n)               # rows of 97 bytes of four values that repeat the row above, but for
        rows[rng.integers(0, n, n // 40)] ^= 1                                    # a changed byte in every 40: the nearest equal three
        out += [("n%d" % n, smooth, 0), ("n%d_rows" % n, rows, 97), ("n%d_rows_stride0" % n, rows, 0)]   # bytes are often elsewhere
    return out
