"""Test helper: raw DEFLATE streams written bit by bit from RFC 1951, for the shapes that zlib's own compressor never emits (deep codes, mixed
block types at odd bit offsets, empty blocks, matches into earlier blocks, degenerate distance alphabets, header run-length codes that
cross from the literal into the distance lengths, every length / distance symbol at both ends of its extra bits), and structured invalid
streams.  Pure Python, independent of the decoders under test; everything is seeded.  catalogue() and invalid_catalogue() are what the
tests use; every catalogue stream is checked against zlib's inflater by the tests before any decoder sees it."""
import functools
import random
from collections import namedtuple

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CLORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST_LENS = [5] * 30


class BitWriter:
    """LSB-first bit stream (RFC 1951 3.1.1): values go in least significant bit first, Huffman codes most significant bit first"""
    def __init__(self):
        self.buf = bytearray(); self.acc = 0; self.n = 0

    def bits(self, value, count):
        assert 0 <= value < (1 << count)
        self.acc |= value << self.n; self.n += count
        while self.n >= 8:
            self.buf.append(self.acc & 0xFF); self.acc >>= 8; self.n -= 8

    def code(self, code, length):
        rev = 0
        for b in range(length): rev |= ((code >> b) & 1) << (length - 1 - b)
        self.bits(rev, length)

    def align(self):
        if self.n: self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.buf += data

    def bit_length(self):
        return len(self.buf) * 8 + self.n

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")


def canonical_codes(lens):
    """code of every symbol from its length (0 = no code), RFC 1951 3.2.2"""
    count = [0] * 16
    for l in lens: count[l] += 1
    count[0] = 0
    nxt = [0] * 17
    code = 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = [0] * len(lens)
    for s, l in enumerate(lens):
        if l: codes[s] = nxt[l]; nxt[l] += 1
    return codes


def kraft(lens):
    """sum of 2^-len in units of 2^-15: 32768 for a complete code"""
    return sum(1 << (15 - l) for l in lens if l)


def complete_lengths(n, max_depth, rng=None):
    """n code lengths of a complete prefix code no deeper than max_depth, ascending.  rng None: always the deepest leaf that may still be split
    is split (depth 15 is reached with 16 symbols); otherwise a random leaf."""
    assert 2 <= n <= (1 << max_depth)
    leaves = [1, 1]
    while len(leaves) < n:
        cand = [i for i, d in enumerate(leaves) if d < max_depth]
        i = max(cand, key=lambda k: leaves[k]) if rng is None else rng.choice(cand)
        d = leaves.pop(i)
        leaves += [d + 1, d + 1]
    leaves.sort()
    assert kraft(leaves) == 32768
    return leaves


def alphabet(size, short, deep, max_depth, rng=None, pad=0):
    """Code lengths of an alphabet of `size` symbols: a complete code over the symbols of `short` (they get the shortest codes, in that order),
    `pad` further symbols nothing uses, and the symbols of `deep` (they get the longest codes: what the tokens use reaches max_depth)."""
    used = list(short) + list(deep)
    assert len(set(used)) == len(used)
    free = [s for s in range(size) if s not in set(used)]
    order = list(short) + free[:pad] + list(deep)
    lens = [0] * size
    for s, l in zip(order, complete_lengths(len(order), max_depth, rng)): lens[s] = l
    return lens


def length_symbol(length):
    s = max(i for i in range(29) if LEN_BASE[i] <= length)
    return s


def distance_symbol(dist):
    return max(i for i in range(30) if DIST_BASE[i] <= dist)


def apply_tokens(tokens, out):
    """appends what the tokens decode to; a token is a literal byte or (length, distance[, length symbol])"""
    for t in tokens:
        if isinstance(t, int): out.append(t); continue
        length, dist = t[0], t[1]
        assert 3 <= length <= 258 and 1 <= dist <= 32768 and dist <= len(out), t
        for _ in range(length): out.append(out[-dist])
    return out


def symbols_used(tokens):
    """(literal/length symbols, distance symbols) of a token list, end-of-block included"""
    ll, dd = {256}, set()
    for t in tokens:
        if isinstance(t, int): ll.add(t)
        else: ll.add(257 + (t[2] if len(t) > 2 else length_symbol(t[0]))); dd.add(distance_symbol(t[1]))
    return ll, dd


def write_tokens(w, tokens, lit_lens, dist_lens):
    lc, dc = canonical_codes(lit_lens), canonical_codes(dist_lens)
    for t in tokens:
        if isinstance(t, int):
            assert lit_lens[t]; w.code(lc[t], lit_lens[t]); continue
        ls = t[2] if len(t) > 2 else length_symbol(t[0])
        assert lit_lens[257 + ls] and 0 <= t[0] - LEN_BASE[ls] < (1 << LEN_EXTRA[ls]), t
        w.code(lc[257 + ls], lit_lens[257 + ls]); w.bits(t[0] - LEN_BASE[ls], LEN_EXTRA[ls])
        ds = distance_symbol(t[1])
        assert dist_lens[ds]
        w.code(dc[ds], dist_lens[ds]); w.bits(t[1] - DIST_BASE[ds], DIST_EXTRA[ds])
    assert lit_lens[256]; w.code(lc[256], lit_lens[256])


def run_length_code(lens, use_repeat_codes):
    """the code-length symbols (symbol, extra value) of a dynamic header over the CONCATENATED literal and distance lengths: a run does not
    stop where the distance lengths begin"""
    if not use_repeat_codes: return [(l, 0) for l in lens]
    syms, i = [], 0
    while i < len(lens):
        j = i
        while j < len(lens) and lens[j] == lens[i]: j += 1
        run, v = j - i, lens[i]
        if v == 0:
            while run >= 11: r = min(run, 138); syms.append((18, r - 11)); run -= r
            if run >= 3: syms.append((17, run - 3)); run = 0
            syms += [(0, 0)] * run
        else:
            syms.append((v, 0)); run -= 1
            while run >= 3: r = min(run, 6); syms.append((16, r - 3)); run -= r
            syms += [(v, 0)] * run
        i = j
    return syms


CL_EXTRA = {16: 2, 17: 3, 18: 7}


def run_crosses(syms, hlit):
    """whether one repeat code of a header's code-length symbols covers both the last literal/length lengths and the first distance lengths"""
    at = 0
    for s, x in syms:
        n = 1 if s < 16 else x + (11 if s == 18 else 3)
        if s >= 16 and at < hlit < at + n: return True
        at += n
    return False


def write_dynamic_header(w, lit_lens, dist_lens, use_repeat_codes=True, full_hclen=False, cl_syms=None, cl_deep=False):
    """HLIT, HDIST, HCLEN, the code-length code and the code lengths.  Nothing about lit_lens / dist_lens is checked: the invalid streams come
    through here too.  cl_syms replaces the run-length coding of the lengths; cl_deep gives the code-length code 7-bit members."""
    assert 257 <= len(lit_lens) <= 288 and 1 <= len(dist_lens) <= 32
    syms = run_length_code(list(lit_lens) + list(dist_lens), use_repeat_codes) if cl_syms is None else cl_syms
    freq = [0] * 19
    for s, _ in syms: freq[s] += 1
    used = sorted((s for s in range(19) if freq[s]), key=lambda s: -freq[s])
    if len(used) == 1: used.append(1 if used[0] != 1 else 2)   # a one-code code-length code is incomplete: zlib refuses it
    k = len(used)
    if cl_deep and k >= 8: cl = complete_lengths(k, 7)
    else:
        m = (k - 1).bit_length()
        cl = [m - 1] * ((1 << m) - k) + [m] * (2 * k - (1 << m))
    cl_lens = [0] * 19
    for s, l in zip(used, cl): cl_lens[s] = l
    assert kraft(cl_lens) == 32768 and max(cl_lens) <= 7
    hclen = 19 if full_hclen else max(4, max(i + 1 for i in range(19) if cl_lens[CLORDER[i]]))
    w.bits(len(lit_lens) - 257, 5); w.bits(len(dist_lens) - 1, 5); w.bits(hclen - 4, 4)
    for i in range(hclen): w.bits(cl_lens[CLORDER[i]], 3)
    cc = canonical_codes(cl_lens)
    for s, x in syms:
        w.code(cc[s], cl_lens[s])
        if s >= 16: w.bits(x, CL_EXTRA[s])
    return syms


class Stream:
    """one raw DEFLATE stream under construction: blocks are appended where the last one ended, bit-exact; .out is what it decodes to"""
    def __init__(self):
        self.w = BitWriter(); self.out = bytearray(); self.header_syms = []

    def stored(self, data, final=False):
        assert len(data) <= 0xFFFF
        self.w.bits(int(final), 1); self.w.bits(0, 2); self.w.align()
        self.w.bits(len(data), 16); self.w.bits(len(data) ^ 0xFFFF, 16); self.w.raw(data)
        self.out += data
        return self

    def fixed(self, tokens, final=False):
        self.w.bits(int(final), 1); self.w.bits(1, 2)
        write_tokens(self.w, tokens, FIXED_LIT_LENS, FIXED_DIST_LENS)
        apply_tokens(tokens, self.out)
        return self

    def dynamic(self, tokens, lit_lens, dist_lens, final=False, use_repeat_codes=True, full_hclen=False, cl_deep=False):
        self.w.bits(int(final), 1); self.w.bits(2, 2)
        self.header_syms += write_dynamic_header(self.w, lit_lens, dist_lens, use_repeat_codes, full_hclen, cl_deep=cl_deep)
        write_tokens(self.w, tokens, lit_lens, dist_lens)
        apply_tokens(tokens, self.out)
        return self

    def getvalue(self):
        return self.w.getvalue()


def trimmed(lens, least):
    """the alphabet cut behind its last coded symbol, as HLIT / HDIST allow"""
    n = max([i + 1 for i, l in enumerate(lens) if l] + [least])
    return list(lens[:n])


def auto_alphabets(tokens, rng, lit_depth=15, dist_depth=15, random_tree=True, lit_pad=0, dist_pad=0):
    """alphabets for a token list: complete codes over what the tokens use (and pads), shuffled so that used symbols sit at every depth"""
    ll, dd = symbols_used(tokens)
    ll, dd = sorted(ll), sorted(dd)
    rng.shuffle(ll); rng.shuffle(dd)
    while len(ll) + lit_pad < 2: lit_pad += 1
    lit = alphabet(286, ll, [], lit_depth, rng if random_tree else None, lit_pad)
    if len(dd) == 0: dist = [0]
    elif len(dd) == 1 and dist_pad == 0: dist = [0] * 30; dist[dd[0]] = 1
    else: dist = alphabet(30, dd, [], dist_depth, rng if random_tree else None, dist_pad)
    return trimmed(lit, 257), trimmed(dist, 1)


# name, the stream, what it inflates to, and whether its literal/length alphabet is a single code (the one class the host fast decoder may decline)
Case = namedtuple("Case", "name comp out single_ll_code")
Invalid = namedtuple("Invalid", "name comp isize zlib_raises core_rc")
# the return codes of uvc_inflate_core.h (the device call reports the same number in its message)
EINPUT, EOUTPUT, ECODE, ESHORT, EDIST = -1, -2, -3, -4, -5


def _length_ends():
    """every length symbol at the lowest and the highest value of its extra bits; 258 also as symbol 284 with all extra bits set"""
    v = []
    for s in range(29):
        v.append((LEN_BASE[s], s))
        if LEN_EXTRA[s]: v.append((LEN_BASE[s] + (1 << LEN_EXTRA[s]) - 1, s))
    assert v[-2] == (258, 27)
    return v


def _all_symbol_tokens(rng, n_literals, max_dist_symbol):
    letters = b"ACGTN!I"
    tokens = [letters[min(int(rng.expovariate(0.7)), 6)] for _ in range(n_literals)]
    lens = _length_ends(); k = 0
    for ds in range(max_dist_symbol + 1):
        for dist in sorted({DIST_BASE[ds], DIST_BASE[ds] + (1 << DIST_EXTRA[ds]) - 1}):
            length, ls = lens[k % len(lens)]; k += 1
            tokens.append((length, dist, ls))
            if k % 3 == 0: tokens += [letters[rng.randrange(7)] for _ in range(k % 5)]   # back-to-back matches and matches behind literals
    while k < len(lens):   # (the small streams have fewer distances than there are length values)
        length, ls = lens[k]; k += 1
        tokens.append((length, 1 + k % 9, ls))
    return tokens


def _deep_alphabets(tokens, lit_depth, dist_depth):
    """the literals get the short codes, the length symbols and end-of-block the deepest; the distance symbols fill their code to dist_depth"""
    ll, dd = symbols_used(tokens)
    freq = {}
    for t in tokens:
        if isinstance(t, int): freq[t] = freq.get(t, 0) + 1
    short = sorted(freq, key=lambda s: -freq[s])
    deep = sorted(s for s in ll if s >= 256)
    pad = max(0, lit_depth + 1 - len(short) - len(deep))
    lit = alphabet(286, short, deep, lit_depth, None, pad)
    dd = sorted(dd)
    dist = alphabet(30, dd[:len(dd) // 2], dd[len(dd) // 2:], dist_depth, None, max(0, dist_depth + 1 - len(dd)))
    assert max(lit[s] for s in ll) == lit_depth and max(dist[s] for s in dd) == dist_depth   # members of full depth that the tokens use
    return trimmed(lit, 257), trimmed(dist, 1)


def _overlap_tokens():
    t = list(b"overlaps!")
    for dist in range(1, 10):
        for length in (3, 8, 63, 64, 65, 128, 129, 258): t.append((length, dist))
    for L in (3, 4, 64, 65, 66, 258):
        t += [(L, L), (L, L - 1), (L, L + 1), (L, 1)]
    t += [(64, 64), (64, 64), (64, 3), (3, 64), (65, 2), (64, 65), (258, 258), (258, 257)]   # each reads what the one before wrote
    return t


@functools.lru_cache(maxsize=None)
def catalogue():
    rng = random.Random(1951)
    cases = []

    def add(name, s, single=False):
        cases.append(Case(name, s.getvalue(), bytes(s.out), single))

    # --- all symbols, deep codes
    tokens = _all_symbol_tokens(rng, 33000, 29)
    lit, dist = _deep_alphabets(tokens, 15, 15)
    add("all_symbols_depth15", Stream().dynamic(tokens, lit, dist, final=True, cl_deep=True))
    add("all_symbols_depth15_plain_header", Stream().dynamic(tokens, lit, dist, final=True, use_repeat_codes=False, full_hclen=True))
    rlit, rdist = auto_alphabets(tokens, rng, 15, 15, random_tree=True, lit_pad=40)
    add("all_symbols_random_tree", Stream().dynamic(tokens, rlit, rdist, final=True))
    small = _all_symbol_tokens(rng, 3000, 22)
    for depth in (9, 10, 11, 12):   # one on each side of every fast-table width
        lit, dist = _deep_alphabets(small, depth, depth - 2)
        add("small_depth_%d_%d" % (depth, depth - 2), Stream().dynamic(small, lit, dist, final=True))
    lit, dist = complete_lengths(286, 15, rng), complete_lengths(30, 15, rng)
    rng.shuffle(lit); rng.shuffle(dist)
    tokens = [rng.randrange(256) for _ in range(2000)] + [(LEN_BASE[s], DIST_BASE[s % 20], s) for s in range(29)] + [rng.randrange(256) for _ in range(100)]
    add("hlit286_hdist30_all_coded", Stream().dynamic(tokens, lit, dist, final=True))

    # --- mixed blocks in one stream
    s = Stream()
    s.fixed(list(b"fixed block first ") + [(5, 6), (12, 3)])
    assert (s.w.bit_length() + 3) % 8 != 0
    s.stored(bytes(rng.randrange(256) for _ in range(301)))          # the header ends inside a byte: the stored bytes start after pad bits
    s.stored(b"")
    t = [65, (258, 1), (40, 300), (3, 635), (100, 17), 66, 67, (258, 1), (7, 320), 68]   # into the stored and the fixed bytes before
    lit, dist = auto_alphabets(t, rng)
    s.dynamic(t, lit, dist)
    s.fixed([])
    s.stored(b"xyz")
    s.fixed(list(b"again") + [(30, 5), (4, 400)])
    t = [rng.randrange(97, 123) for _ in range(200)] + [(64, 64), (64, 1), (9, 700)] + [rng.randrange(97, 123) for _ in range(50)]
    lit, dist = auto_alphabets(t, rng, 12, 6, lit_pad=30, dist_pad=8)
    s.dynamic(t, lit, dist, cl_deep=True)
    s.stored(b"", final=True)
    add("mixed_block_types", s)
    add("stored_then_empty_fixed", Stream().stored(b"stored data, then the end").fixed([], final=True))
    add("only_empty_stored", Stream().stored(b"", final=True))
    add("only_empty_fixed", Stream().fixed([], final=True))
    add("stored_ff00", Stream().stored(bytes(rng.randrange(256) for _ in range(0xff00)), final=True))

    # --- overlapped copies on both sides of the 64-lane and 8-byte strides
    t = _overlap_tokens()
    lit, dist = auto_alphabets(t, rng, 11, 9, lit_pad=20, dist_pad=3)
    add("overlaps_dynamic", Stream().dynamic(t, lit, dist, final=True))
    add("overlaps_fixed", Stream().fixed(t, final=True))

    # --- header shapes
    t = list(b"one distance code") + [(10, 5), 33, (4, 6), (258, 5), 34, (3, 5)]
    lit, dist = auto_alphabets(t, rng)
    assert [l for l in dist if l] == [1]
    add("one_distance_code", Stream().dynamic(t, lit, dist, final=True))
    t = list(b"no distance code at all: literals only")
    lit, dist = auto_alphabets(t, rng)
    assert dist == [0]
    add("no_distance_code", Stream().dynamic(t, lit, dist, final=True))
    lit, dist = auto_alphabets([90], rng)
    assert sorted(l for l in lit if l) == [1, 1]
    add("one_literal_dynamic", Stream().dynamic([90], lit, dist, final=True))
    t = list(b"aaaa") + [(258, 1), (257, 2), (258, 3), (250, 4), 97]          # four 2-bit codes in each alphabet: one repeat covers symbol 285 and the distances
    lit = [0] * 286; lit[97] = lit[256] = lit[284] = lit[285] = 2
    s = Stream().dynamic(t, lit, [2, 2, 2, 2], final=True)
    assert (16, 2) in s.header_syms and run_crosses(s.header_syms, 286)
    add("repeat_16_crosses_into_the_distance_lengths", s)
    t = list(b"abba") + [(258, 1), (258, 2), (258, 3), (258, 4), 97]          # the repeat begins at the first distance length and copies symbol 285's
    lit = [0] * 286; lit[97] = lit[98] = lit[256] = lit[285] = 2
    s = Stream().dynamic(t, lit, [2, 2, 2, 2], final=True)
    assert s.header_syms[-2:] == [(2, 0), (16, 1)]
    add("repeat_16_starts_at_the_distance_lengths", s)
    t = list(b"zero run") + [(3, 8), (4, 5), 33, (5, 16)]                         # HLIT 286 with nothing coded behind symbol 259, no distance below 5
    lit, dist = auto_alphabets(t, rng)
    s = Stream().dynamic(t, lit + [0] * (286 - len(lit)), dist, final=True)
    assert dist[:4] == [0] * 4 and any(c == 18 for c, _ in s.header_syms) and run_crosses(s.header_syms, 286)
    add("repeat_18_crosses_into_the_distance_lengths", s)
    eob_only = [0] * 256 + [1]
    add("stored_then_eob_only_dynamic", Stream().stored(b"behind me: a block of nothing").dynamic([], eob_only, [0], final=True), single=True)

    # --- ends: the compressed size runs across the 8-byte and 4-byte tail loads; a match that ends exactly at ISIZE, with and without pad bits
    for n in range(12):
        add("fixed_%d_literals" % n, Stream().fixed([48 + i for i in range(n)], final=True))
    for n in range(1, 6):
        padded = set()
        for first in (65, 200):   # literals below 144 have 8-bit codes, the others 9: one of the two streams ends on a byte boundary
            s = Stream().fixed([first] + [66 + i for i in range(n - 1)] + [(258, n)], final=True)
            pad = s.w.bit_length() % 8 != 0
            padded.add(pad)
            add("fixed_%d_literals_match_to_isize_%s" % (n, "pad" if pad else "nopad"), s)
        assert padded == {False, True}
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def _fixed_code(w, sym):
    w.code(canonical_codes(FIXED_LIT_LENS)[sym], FIXED_LIT_LENS[sym])


@functools.lru_cache(maxsize=None)
def invalid_catalogue():
    """Structured invalid streams: each breaks one rule and nothing else, and where it reaches outside its output it does so by a few bytes.
    zlib_raises is False only where the stream itself is legal and it is the output size (ISIZE) that it misses.  core_rc is the error
    that names the broken rule in uvc_inflate_core.h: a stream refused for another reason has not tested its rule."""
    cases = []

    def add(name, s, isize, core_rc, zlib_raises=True):
        cases.append(Invalid(name, s.getvalue(), isize, zlib_raises, core_rc))

    def fixed_start(lits):
        s = Stream(); s.w.bits(1, 1); s.w.bits(1, 2)
        for c in lits: _fixed_code(s.w, c)
        return s
    s = fixed_start(b"abcd"); _fixed_code(s.w, 286); s.w.bits(0, 5); _fixed_code(s.w, 256)
    add("length_symbol_286", s, 7, ECODE)
    s = fixed_start(b"abcd"); _fixed_code(s.w, 287); s.w.bits(0, 5); _fixed_code(s.w, 256)
    add("length_symbol_287", s, 7, ECODE)
    for ds in (30, 31):
        s = fixed_start(b"abcd"); _fixed_code(s.w, 257); s.w.code(ds, 5); _fixed_code(s.w, 256)
        add("distance_symbol_%d" % ds, s, 7, ECODE)
    s = fixed_start(b"ab"); _fixed_code(s.w, 257); s.w.code(2, 5); _fixed_code(s.w, 256)                 # (3, 3) behind two bytes
    add("distance_before_the_start", s, 5, EDIST)
    s = fixed_start(b""); _fixed_code(s.w, 257); s.w.code(0, 5); _fixed_code(s.w, 256)                   # a match as the first symbol
    add("match_first", s, 3, EDIST)
    add("match_past_isize", Stream().fixed(list(b"abcd") + [(10, 1)], final=True), 12, EOUTPUT, zlib_raises=False)   # 14 bytes
    add("literal_past_isize", Stream().fixed(list(b"abcdef"), final=True), 5, EOUTPUT, zlib_raises=False)
    add("stream_short_of_isize", Stream().fixed(list(b"abcdef"), final=True), 8, ESHORT, zlib_raises=False)
    s = Stream(); s.w.bits(1, 1); s.w.bits(0, 2); s.w.align(); s.w.bits(4, 16); s.w.bits(4 ^ 0xFFFE, 16); s.w.raw(b"abcd")
    add("stored_len_nlen_mismatch", s, 4, ECODE)
    s = Stream().fixed(list(b"ab")); s.w.bits(1, 1); s.w.bits(0, 2); s.w.align(); s.w.bits(9, 16); s.w.bits(9 ^ 0xFFFF, 16); s.w.raw(b"abcd")
    add("stored_longer_than_the_input", s, 11, EINPUT)
    s = Stream().fixed(list(b"ab")); s.w.bits(1, 1); s.w.bits(3, 2); s.w.bits(0, 13)
    add("block_type_3", s, 2, ECODE)
    add("no_final_block_stored", Stream().stored(b"abcdefgh"), 8, EINPUT)
    add("no_final_block_fixed", Stream().fixed(list(b"abcdefgh")), 8, EINPUT)

    def dyn(lit_lens, dist_lens, cl_syms=None, tail=True):
        s = Stream(); s.w.bits(1, 1); s.w.bits(2, 2)
        write_dynamic_header(s.w, lit_lens, dist_lens, cl_syms=cl_syms)
        if tail: s.w.bits(0, 32)
        return s
    lit = [0] * 257; lit[97] = lit[98] = lit[256] = 1
    add("oversubscribed_literal_code", dyn(lit, [0]), 4, ECODE)
    lit = [0] * 257; lit[97] = 1; lit[98] = lit[256] = 2
    add("oversubscribed_distance_code", dyn(lit, [1, 1, 1]), 4, ECODE)
    add("repeat_16_first", dyn([0] * 257, [0], cl_syms=[(16, 0), (1, 0), (1, 0), (18, 127), (18, 102), (1, 0), (0, 0)]), 4, ECODE)   # (258 lengths if the 16 stood for three)
    # 257 + 1 lengths: 97 zeros, two ones, then runs of zeros that end 5 past the last length
    add("repeat_overruns_the_lengths", dyn([0] * 257, [0], cl_syms=[(18, 97 - 11), (1, 0), (1, 0), (18, 127), (18, 26 - 11)]), 4, ECODE)
    lit = [0] * 257; lit[97] = lit[98] = 1
    add("no_end_of_block_length", dyn(lit, [0]), 4, ECODE)
    # an incomplete literal/length code (a 00, end-of-block 01; 10 and 11 are nobody's) is the core's to accept (lenient_catalogue); a
    # stream that then USES a code nobody has is invalid, and must end at that code whatever ISIZE says
    s = Stream(); s.w.bits(1, 1); s.w.bits(2, 2)
    write_dynamic_header(s.w, _incomplete_lit_lens(), [0])
    for _ in range(3): s.w.code(0, 2)
    s.w.code(3, 2); s.w.code(1, 2)
    add("unassigned_code_of_an_incomplete_code", s, 3, ECODE)
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def _incomplete_lit_lens():
    lit = [0] * 257; lit[97] = lit[256] = 2
    return lit


@functools.lru_cache(maxsize=None)
def lenient_catalogue():
    """(name, stream, output) of the two things the project's decoders take and zlib's inflater does not: an incomplete literal/length code
    (two symbols, both of length 2), and whole bytes behind the final block"""
    s = Stream().dynamic([97, 97, 97], _incomplete_lit_lens(), [0], final=True)
    t = Stream().fixed(list(b"trailing") + [(20, 8)], final=True)
    return (("incomplete_literal_code", s.getvalue(), bytes(s.out)), ("bytes_behind_the_final_block", t.getvalue() + b"\x00\x7f\xff", bytes(t.out)))
