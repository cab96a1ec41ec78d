"""Deterministic MP3 streams that put the Huffman / scalefactor decode (k_dec_huffman and its host twins) at its bit-stream edges, and a
bit-position model of how the reference reads them (decoder/Frame.py:357-559).

Every stream is one to three MPEG-1 Layer III frames without bit reservoir (main_data_begin = 0), written field by field: the reference's
parser, the oracle, the host parser and every device path read the same bytes.  Two things come out of this module:

  streams()        name -> Stream: the bytes, and what the BUILDER wrote where (per unit: start bit, start bit of every pair and quadruple
                   it wrote, max_bit)
  model(data)      a plain walk over the bytes of a stream with the reference's cursor rules -> per unit the start bit of EVERY pair and
                   quadruple the reference reads (also of those it reads from bits that belong to something else), the decoded lines, and
                   from them: which units k_dec_huffman must flag with which MP3S_HS_* bit, and at which frame the reference refuses the stream

The expected flags follow from the model and never from the code under test:

  MP3S_HS_BAD_REGION  a long-window unit whose region0_count + 1 or region0_count + region1_count + 2 exceeds 22 (the reference indexes
                      its 23-entry band table: IndexError)
  MP3S_HS_BIG_VALUES  big_values > 288 (the reference writes behind its 576 lines: IndexError)
  MP3S_HS_OVERRUN     the kernel's documented rule: some big-value pair of the unit STARTS at a bit greater than max_bit (the reference's cursor,
                      Frame.py:469-518; pairs of books 0, 4 and 14 take no bits but have a start like any other).  A pair that starts at or
                      before max_bit and runs past it is decoded and not flagged.  A unit with one of the two bits above is not decoded at all
                      and so reports no overrun.
  MP3S_HS_HINT        part2_3_length above the caller's bound (only when the test passes a bound that does not hold)

The reference refuses a stream at the first frame that holds a BAD_REGION or BIG_VALUES unit, and no other.
"""
import hashlib
import itertools

import numpy as np

from frame_synth import Bits, put_pair, put_quad, books, SFB_LONG, SLEN, LINBITS, XMAX, BITRATES, RATES

HS_BAD_REGION, HS_BIG_VALUES, HS_HINT, HS_OVERRUN = 1, 2, 4, 8
BIG_BOOKS = [1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 24]        # the distinct big-value code books
YLEN = {1: 2, 2: 3, 3: 3, 5: 4, 6: 4, 7: 6, 8: 6, 9: 6, 10: 8, 11: 8, 12: 8}
VALUE_MAX = 15 + 8191
LONGEST = (23, VALUE_MAX, -VALUE_MAX)                                   # the big-value pair of the most bits: 8 of code word, two escapes of 13, two signs


def ylen(t):
    return YLEN.get(t, 16)


def hlen(t, x, y):
    return int(books()[t][1][min(x, 15) * ylen(t) + min(y, 15)])


def pair_bits(t, x, y):
    """bits of one big-value pair: code word, linbits, signs"""
    if t in (0, 4, 14):
        return 0
    ax, ay = abs(x), abs(y)
    return hlen(t, ax, ay) + (LINBITS[t] if ax >= 15 and LINBITS[t] else 0) + (LINBITS[t] if ay >= 15 and LINBITS[t] else 0) + (ax > 0) + (ay > 0)


def longest_code(t):
    """(x, y) of the longest code word of book t (the first of them in table order)"""
    hl = books()[t][1]
    n = ylen(t)
    i = int(np.argmax(hl[:n * n] if t > 12 else hl))
    return i // n, i % n


def part2_fields(u, gr, scfsi):
    """the widths of the scalefactor fields of a unit in the order the reference reads them (Frame.py:365-441)"""
    s0, s1 = SLEN[u["sfc"]]
    if u["ws"] and u["bt"] == 2:
        return [s0] * (17 if u["mixed"] else 18) + [s1] * 18
    if gr == 0:
        return [s0] * 11 + [s1] * 10
    return [s0 if s < 11 else s1 for s in range(21) if not scfsi[0 if s < 6 else (1 if s < 11 else (2 if s < 16 else 3))]]


def regions(u, sr):
    """(region0, region1, bad) in lines"""
    if u["ws"] and u["bt"] == 2:
        return 36, 576, False
    r0c, r1c = (7, 13) if u["ws"] else (u["r0c"], u["r1c"])
    i0, i1 = r0c + 1, r0c + r1c + 2
    if i0 > 22 or i1 > 22:
        return SFB_LONG[sr][min(i0, 22)], 576, True
    return SFB_LONG[sr][i0], SFB_LONG[sr][i1], False


def book_at(u, sr, line):
    r0, r1, _ = regions(u, sr)
    return u["ts"][0] if line < r0 else (u["ts"][1] if line < r1 else u["ts"][2])


_DEFAULT = dict(sfc=0, ws=0, bt=0, mixed=0, ts=(0, 0, 0), r0c=0, r1c=0, c1=0, gg=150, pre=0, sfs=0, sbg=(0, 0, 0), sf="ones", pairs=(),
                quads=(), tail="", bv=None, p23=None)


def U(**kw):
    """a unit: its side-info fields and what is written into its bits -- scalefactor fields (sf: "ones" = every field all ones, or an
    integer k: field i holds (5 * i + k) masked to its width), big-value `pairs` with the books the side info selects, count1 `quads`,
    and a `tail` of raw bits.  bv / p23 default to what was written; other values make the malformed cases."""
    d = dict(_DEFAULT)
    assert set(kw) <= set(d), kw
    d.update(kw)
    return d


class Stream:
    def __init__(self, name, frames, sr=0, mono=False, cut=None, bitrate=None, pcm=False):
        """frames: [dict(units=[[gr0ch0, gr0ch1], [gr1ch0, gr1ch1]], scfsi=[[4], [4]], fill=byte)]; cut: bytes of the LAST frame's main data
        that the file still holds; pcm: the fixture also records the reference's PCM digests of this stream"""
        self.name, self.sr, self.mono, self.pcm, self.cut = name, sr, mono, pcm, cut
        nch = 1 if mono else 2
        side_len = 17 if mono else 32
        out = bytearray()
        self.units = []                   # per frame [gr][ch] -> dict(start, max_bit, pair_bits, quad_bits, part2_end)
        for fi, fr in enumerate(frames):
            scfsi = fr.get("scfsi", [[0] * 4] * 2)
            md, start, rec = Bits(), 0, [[None, None], [None, None]]
            for gr in range(2):
                for ch in range(nch):
                    u = fr["units"][gr][ch]
                    own = Bits()
                    for i, w in enumerate(part2_fields(u, gr, scfsi[ch])):
                        own.put((1 << w) - 1 if u["sf"] == "ones" else (5 * i + u["sf"]) & ((1 << w) - 1), w)
                    part2 = len(own)
                    pb, qb = [], []
                    for p, (x, y) in enumerate(u["pairs"]):
                        t = book_at(u, sr, 2 * p)
                        pb.append(len(own))
                        if t in (0, 4, 14):
                            assert x == 0 and y == 0
                        else:
                            assert max(abs(x), abs(y)) <= XMAX[t] + (((1 << LINBITS[t]) - 1) if LINBITS[t] else 0), (name, t, x, y)
                            put_pair(own, t, x, y)
                    for q in u["quads"]:
                        qb.append(len(own))
                        put_quad(own, u["c1"], q)
                    for c in u["tail"]:
                        own.put(int(c), 1)
                    if len(own):
                        assert len(md) <= start, (name, fi, gr, ch, "the unit in front wrote into this one")
                        md.put(0, start - len(md))
                    at = len(md)
                    md.b += own.b
                    p23 = len(own) if u["p23"] is None else u["p23"]
                    assert 0 <= p23 <= 4095, (name, p23)
                    rec[gr][ch] = dict(start=start, max_bit=start + p23, part2_end=at + part2, pair_bits=[at + b for b in pb],
                                       quad_bits=[at + b for b in qb], p23=p23, bv=len(u["pairs"]) if u["bv"] is None else u["bv"], at=at, written=len(own.b))
                    start += p23
            md.put(0, max(0, start - len(md)))
            need = (len(md) + 7) // 8
            if bitrate is None:
                bi = next(b for b in range(1, 15) if 144 * BITRATES[b] * 1000 // RATES[sr] - 4 - side_len >= max(need, 24))
            else:
                bi = bitrate
            fsize = 144 * BITRATES[bi] * 1000 // RATES[sr]
            cap = fsize - 4 - side_len
            assert need <= cap, (name, need, cap)
            si = Bits()
            si.put(0, 9)
            si.put(0, 5 if mono else 3)
            for ch in range(nch):
                for b in range(4):
                    si.put(scfsi[ch][b], 1)
            for gr in range(2):
                for ch in range(nch):
                    u, r = fr["units"][gr][ch], rec[gr][ch]
                    si.put(r["p23"], 12); si.put(r["bv"], 9); si.put(u["gg"], 8); si.put(u["sfc"], 4); si.put(u["ws"], 1)
                    if u["ws"]:
                        si.put(u["bt"], 2); si.put(u["mixed"], 1); si.put(u["ts"][0], 5); si.put(u["ts"][1], 5)
                        for w in range(3):
                            si.put(u["sbg"][w], 3)
                    else:
                        for r3 in range(3):
                            si.put(u["ts"][r3], 5)
                        si.put(u["r0c"], 4); si.put(u["r1c"], 3)
                    si.put(u["pre"], 1); si.put(u["sfs"], 1); si.put(u["c1"], 1)
            assert len(si) == side_len * 8
            body = md.bytes()
            body += bytes([fr.get("fill", 0)]) * (cap - len(body))
            if cut is not None and fi == len(frames) - 1:
                body = body[:cut]
            out += bytes([0xFF, 0xFB, (bi << 4) | (sr << 2), (3 if mono else 0) << 6]) + si.bytes() + body
            self.units.append(rec)
        self.data = bytes(out)
        self.n_frames, self.nch = len(frames), nch


# ------------------------------------------------------------------------------------------------------- the model
_DEC = {}


def _decode_tables(t):
    """book -> {code word as a bit string: (x, y)}, lengths present; from the ISO code books (tests/golden/g1_tables.npz)"""
    if t not in _DEC:
        hc, hl = books()[t]
        n = 16 if t == 32 else ylen(t) ** 2
        d = {format(int(hc[i]), "0%db" % int(hl[i])): i for i in range(n) if hl[i]}
        assert len(d) == n
        _DEC[t] = (d, sorted({len(k) for k in d}))
    return _DEC[t]


def _lookup(t, s, bit):
    d, lens = _decode_tables(t)
    for n in lens:
        i = d.get(s[bit:bit + n])
        if i is not None:
            return i, n
    return None, 0        # no entry matches: the reference leaves the pair zero and the cursor in place


def parse_frames(data):
    """the stream's frames as the reference walks them (MP3_Parser.py:68-80): [(sr, nch, scfsi, units[gr][ch], main data bit string)]"""
    out, pos = [], 0
    while len(data) > pos + 4:
        h = data[pos:pos + 4]
        assert h[0] == 0xFF and h[1] == 0xFB
        sr, mono = (h[2] >> 2) & 3, (h[3] >> 6) == 3
        fsize = 144 * BITRATES[h[2] >> 4] * 1000 // RATES[sr] + ((h[2] >> 1) & 1)
        nch, side_len = (1, 17) if mono else (2, 32)
        buf = data[pos:pos + fsize]
        assert len(buf) >= 4 + side_len
        sb = "".join(format(b, "08b") for b in buf[4:4 + side_len])
        o = [0]

        def get(n):
            v = int(sb[o[0]:o[0] + n], 2)
            o[0] += n
            return v
        assert get(9) == 0
        get(5 if mono else 3)
        scfsi = [[get(1) for _ in range(4)] for _ in range(nch)]
        units = [[None, None], [None, None]]
        for gr in range(2):
            for ch in range(nch):
                u = dict(p23=get(12), bv=get(9), gg=get(8), sfc=get(4), ws=get(1), bt=0, mixed=0, r0c=0, r1c=0, sbg=(0, 0, 0))
                if u["ws"]:
                    u["bt"], u["mixed"] = get(2), get(1)
                    u["ts"] = (get(5), get(5), 0)
                    u["sbg"] = (get(3), get(3), get(3))
                else:
                    u["ts"] = (get(5), get(5), get(5))
                    u["r0c"], u["r1c"] = get(4), get(3)
                u["pre"], u["sfs"], u["c1"] = get(1), get(1), get(1)
                units[gr][ch] = u
        md = buf[4 + side_len:fsize]
        out.append((sr, nch, scfsi, units, "".join(format(b, "08b") for b in md) + "0" * 8400, len(md)))
        pos += fsize
    return out


def walk_unit(u, sr, gr, scfsi, s, start):
    """one unit with the reference's cursor: -> dict(start, max_bit, part2_end, pair_bits, quad_bits, lines[576], flags, sf: the fields read)"""
    bit, max_bit = start, start + u["p23"]
    sf = []
    for w in part2_fields(u, gr, scfsi):
        sf.append(int(s[bit:bit + w], 2) if w else 0)
        bit += w
    r = dict(start=start, max_bit=max_bit, part2_end=bit, pair_bits=[], quad_bits=[], lines=np.zeros(576, dtype=np.int16), sf=sf, nomatch=0)
    _, _, bad = regions(u, sr)
    r["flags"] = (HS_BAD_REGION if bad else 0) | (HS_BIG_VALUES if u["bv"] > 288 else 0)
    if r["flags"]:
        return r
    line = 0
    for p in range(u["bv"]):
        t = book_at(u, sr, line)
        r["pair_bits"].append(bit)
        if bit > max_bit:
            r["flags"] |= HS_OVERRUN
        if t not in (0, 4, 14):
            tt = 16 if 16 <= t < 24 else (24 if t >= 24 else t)
            i, n = _lookup(tt, s, bit)
            if i is None:
                r["nomatch"] += 1
            else:
                bit += n
                for k, v in enumerate((i // ylen(tt), i % ylen(tt))):
                    if LINBITS[t] and v == 15:
                        v += int(s[bit:bit + LINBITS[t]], 2)
                        bit += LINBITS[t]
                    if v:
                        v = -v if s[bit] == "1" else v
                        bit += 1
                    r["lines"][line + k] = v
        line += 2
    r["pairs_end"] = bit
    while bit < max_bit and line + 4 < 576:           # D1
        r["quad_bits"].append(bit)
        if u["c1"]:
            v = [1 - int(c) for c in s[bit:bit + 4]]
            bit += 4
        else:
            i, n = _lookup(32, s, bit)
            bit += n
            v = [(i >> 3) & 1, (i >> 2) & 1, (i >> 1) & 1, i & 1] if i is not None else [0, 0, 0, 0]
        for k in range(4):
            if v[k]:
                v[k] = -1 if s[bit] == "1" else 1
                bit += 1
        r["lines"][line:line + 4] = v
        line += 4
    r["end_bit"], r["end_line"] = bit, line
    return r


_MODEL = {}


def model(data):
    """-> dict(units: per frame [gr][ch] walk_unit results, flags: OR over the stream, frame_flags, refused_at: frame or -1,
    lines int16 [frames][2][2][576], md_len per frame)"""
    key = hashlib.blake2b(data, digest_size=16).digest()
    if key in _MODEL:
        return _MODEL[key]
    frames = parse_frames(data)
    n = len(frames)
    out = dict(units=[], frame_flags=[], refused_at=-1, lines=np.zeros((n, 2, 2, 576), dtype=np.int16), md_len=[f[5] for f in frames],
               nch=frames[0][1], sr=frames[0][0], max_p23=0)
    for f, (sr, nch, scfsi, units, s, _) in enumerate(frames):
        rec, start, ff = [[None, None], [None, None]], 0, 0
        for gr in range(2):
            for ch in range(nch):
                r = walk_unit(units[gr][ch], sr, gr, scfsi[ch], s, start)
                r["side"], r["scfsi"] = units[gr][ch], scfsi[ch]
                rec[gr][ch] = r
                out["lines"][f, gr, ch] = r["lines"]
                ff |= r["flags"]
                out["max_p23"] = max(out["max_p23"], units[gr][ch]["p23"])
                start = r["max_bit"]
        out["units"].append(rec)
        out["frame_flags"].append(ff)
        if ff & (HS_BAD_REGION | HS_BIG_VALUES) and out["refused_at"] < 0:
            out["refused_at"] = f
    out["flags"] = int(np.bitwise_or.reduce(out["frame_flags"]))
    _MODEL[key] = out
    return out


def frame_digests(pcm):
    """a 64-bit blake2b of every frame's float64 PCM bytes"""
    return np.array([int.from_bytes(hashlib.blake2b(np.ascontiguousarray(pcm[i:i + 1152]).tobytes(), digest_size=8).digest(), "little")
                     for i in range(0, len(pcm), 1152)], dtype=np.uint64)


def input_digest(data):
    return int.from_bytes(hashlib.blake2b(data, digest_size=8).digest(), "little")


# ------------------------------------------------------------------------------------------------------- case builders
def signed(vals):
    """every sign combination of a tuple of magnitudes"""
    return [tuple(-v if (m >> k) & 1 else v for k, v in enumerate(vals)) for m in range(1 << len(vals))
            if all(v or not (m >> k) & 1 for k, v in enumerate(vals))]


def filler(k=0):
    """a small well-formed unit whose bits are not zero"""
    return U(ts=(1, 1, 1), pairs=[(1, -1), (-1, 1), (0, 1), (1, 1)], quads=[(1, -1, 1, -1), (0, 1, 0, -1)], sf=k, sfc=5)


def empty():
    return U()


def frame(units, mono=False, **kw):
    """units: up to four, in the order of the bits; the rest are empty"""
    units = list(units) + [empty() for _ in range((2 if mono else 4) - len(units))]
    d = dict(units=[[units[0], None], [units[1], None]] if mono else [[units[0], units[1]], [units[2], units[3]]])
    d.update(kw)
    return d


def pack_units(t, pairs, max_bits=1900, **kw):
    """units of book t (all three regions) that hold `pairs` back to back: at most 288 pairs and max_bits bits each"""
    out, cur, bits = [], [], 0
    for x, y in pairs:
        b = pair_bits(t, x, y)
        if len(cur) == 288 or bits + b > max_bits:
            out.append(U(ts=(t, t, t), pairs=cur, **kw))
            cur, bits = [], 0
        cur.append((x, y))
        bits += b
    out.append(U(ts=(t, t, t), pairs=cur, **kw))
    return out


def streams_of_units(prefix, units, per_frame=4, frames_per_stream=3, **kw):
    """units laid out four to a frame, three frames to a stream"""
    out = []
    per = per_frame * frames_per_stream
    for i in range(0, len(units), per):
        chunk = units[i:i + per]
        frames = [frame(chunk[j:j + per_frame], mono=kw.get("mono", False)) for j in range(0, len(chunk), per_frame)]
        out.append(Stream("%s/%d" % (prefix, i // per) if len(units) > per else prefix, frames, **kw))
    return out


def all_pairs(t):
    n = XMAX[t] + 1
    return [p for x in range(n) for y in range(n) for p in signed((x, y))]


ESC_BOOKS = list(range(16, 32))


def escape_values(t):
    return sorted({0, 1, 14, 15, 16, 15 + (1 << LINBITS[t]) - 1})


def pad_quads(n):
    """n one-bit count1 quadruples of book A: zeros, each the code word '1' (lengthen a unit by n bits)"""
    return [(0, 0, 0, 0)] * n


def family_code_words():
    out = []
    for t in BIG_BOOKS:
        out += streams_of_units("codes/book%d" % t, pack_units(t, all_pairs(t)), pcm=t in (7, 24))
    # the widest books again at two other alignments of the first code word: the scalefactor bits in front are 10 and 21 bits
    for t in (13, 15, 16, 24):
        for sfc, nbits in ((1, 10), (5, 21)):
            out += streams_of_units("codes/book%d_part2_%d" % (t, nbits), pack_units(t, all_pairs(t), sfc=sfc, sf=3))
    for c1 in (0, 1):
        quads = [q for i in range(16) for q in signed(((i >> 3) & 1, (i >> 2) & 1, (i >> 1) & 1, i & 1))]
        out.append(Stream("codes/count1_%s" % "AB"[c1], [frame([U(c1=c1, quads=quads), filler(), U(c1=c1, quads=quads[::-1], sfc=9, sf=1)])], pcm=c1 == 0))
    return out


def family_escapes():
    out = []
    for t in ESC_BOOKS:
        vals = escape_values(t)
        pairs = [p for x in vals for y in vals for p in signed((x, y))]
        out += streams_of_units("escapes/book%d" % t, pack_units(t, pairs), pcm=t == 31)
    # the longest code word of the book, then the largest escapes in both signs and both positions, first code word at every bit alignment
    for t in (23, 24, 31):
        top = 15 + (1 << LINBITS[t]) - 1
        seq = [longest_code(t), (top, -top), (-top, top), (top, 0), (0, -top)]
        units, at = [], 0
        for a in range(32):
            if len(units) % 4 == 0:                               # the first unit of a frame starts at bit 0: a unit of `a` bits in front
                units.append(U(quads=pad_quads(a)))
                at = a
            assert at % 32 == a
            n = sum(pair_bits(t, x, y) for x, y in seq)
            padq = (a + 1 - at - n) % 32                          # the next test unit starts one bit further on
            units.append(U(ts=(t, t, t), pairs=seq, quads=pad_quads(padq)))
            at += n + padq
        out += streams_of_units("escapes/align_book%d" % t, units)
    return out


def family_no_bits_books():
    """books 0, 4 and 14 in each of the three regions: no bits, zeros (D2); the neighbours are real books"""
    out = []
    for t in (0, 4, 14):
        units = []
        for region in range(3):
            ts = [7, 7, 7]
            ts[region] = t
            # regions: lines 0..3, 4..7, 8.. (region0_count = region1_count = 0)
            pairs = [(0, 0) if p // 2 == region or (region == 2 and p >= 4) else (3, -2) for p in range(8)]
            units.append(U(ts=tuple(ts), pairs=pairs, quads=[(1, 0, 0, -1)]))
        out.append(Stream("nobits/book%d" % t, [frame(units + [filler()])]))
    return out


def family_regions(sr=0, mono=False, tag=""):
    out = []

    def mframe(units, **kw):
        return frame(units, mono=mono, **kw)
    sfb = SFB_LONG[sr]
    mk = dict(sr=sr, mono=mono)
    # region0_count / region1_count at and beyond the band table: i1 = 22 (line 576), i0 = 22 (not reachable with 4 bits: 16 is the largest),
    # i1 = 23 and the maximum (15, 7) = 24
    for r0c, r1c in ((15, 5), (13, 7), (14, 7), (15, 6), (15, 7)):
        for bv in (0, 3):
            u = U(ts=(1, 2, 3), r0c=r0c, r1c=r1c, pairs=[(1, -1)] * bv)
            out.append(Stream("regions%s/r0c%d_r1c%d_bv%d" % (tag, r0c, r1c, bv), [mframe([filler(), u]), mframe([filler(1)])], **mk))
    # big_values before, on and one pair past either bound; neighbouring books of different index width and linbits (13: none, 24: 4, 31: 13, 1: a 1-bit book)
    for r0c, r1c, ts in ((2, 1, (1, 13, 31)), (5, 3, (24, 1, 16)), (0, 0, (31, 2, 24))):
        r0, r1 = sfb[r0c + 1] // 2, sfb[r0c + r1c + 2] // 2
        for bv in sorted({r0 - 1, r0, r0 + 1, r1 - 1, r1, r1 + 1}):
            vals = {1: (1, -1), 2: (2, -1), 13: (-15, 14), 16: (16, -15), 24: (-30, 15), 31: (8206, -17)}
            u0 = U(ts=ts, r0c=r0c, r1c=r1c)
            pairs = [vals[book_at(u0, sr, 2 * p)] for p in range(bv)]
            u = U(ts=ts, r0c=r0c, r1c=r1c, pairs=pairs, quads=[(1, 1, -1, 0)], sfc=6, sf=2)
            out.append(Stream("regions%s/books%d_%d_%d_bv%d" % ((tag,) + ts + (bv,)), [mframe([u, filler()] if not mono else [u])], **mk))
    # short windows: the bounds are 36 and 576 whatever the counts; a start block has (7, 13)
    for bt, mixed in ((2, 0), (2, 1), (1, 0), (3, 1)):
        r0 = 18 if bt == 2 else sfb[8] // 2
        for bv in (r0 - 1, r0, r0 + 1):
            u0 = U(ws=1, bt=bt, mixed=mixed, ts=(15, 24, 0))
            pairs = [(15, -3) if book_at(u0, sr, 2 * p) == 15 else (-30, 1) for p in range(bv)]
            u = U(ws=1, bt=bt, mixed=mixed, ts=(15, 24, 0), pairs=pairs, quads=[(0, 1, 0, 1)], sfc=8, sbg=(1, 2, 3))
            out.append(Stream("regions%s/bt%d_mixed%d_bv%d" % (tag, bt, mixed, bv), [mframe([filler(), u])], **mk))
    return out


def family_big_values(sr=0, mono=False, tag=""):
    out = []

    def mframe(units, **kw):
        return frame(units, mono=mono, **kw)
    mk = dict(sr=sr, mono=mono)
    for bv in (0, 287, 288, 289, 511):
        u = U(bv=bv, quads=[(1, -1, 0, 0)], r0c=7, r1c=3)
        out.append(Stream("big_values%s/book0_%d" % (tag, bv), [mframe([filler(), u]), mframe([filler(2)])], **mk))
    for bv in (287, 288):
        u = U(ts=(1, 2, 1), r0c=7, r1c=3, pairs=[(1, -1) if p % 3 else (0, 0) for p in range(bv)], quads=[(1, -1, 0, 0)])
        out.append(Stream("big_values%s/real_%d" % (tag, bv), [mframe([u, filler()] if not mono else [u])], **mk))
    u = U(ts=(1, 2, 1), r0c=7, r1c=3, pairs=[(1, 1)] * 288, bv=289)
    out.append(Stream("big_values%s/real_289" % tag, [mframe([u])], **mk))
    return out


def family_count1_end():
    out = []
    ones = [(1, -1, 1, -1)] * 4
    for c1 in (0, 1):
        # more count1 bits than lines: quadruples start at lines 566..574, D1 stops them in front of 572
        for bv in (283, 284, 285, 286, 287):
            u = U(ts=(1, 1, 1), r0c=3, r1c=3, c1=c1, pairs=[(0, 0)] * (bv - 1) + [(1, 1)], quads=ones)
            out.append(Stream("count1/end_c1%d_bv%d" % (c1, bv), [frame([u, filler()])]))
        # quadruples all the way: the last one starts at line 568
        q = [((i >> 1) & 1, 0, -(i & 1), 0) for i in range(143)] + [(1, 1, 1, 1), (-1, -1, -1, -1)]
        out.append(Stream("count1/all_the_way_c1%d" % c1, [frame([filler(), U(c1=c1, quads=q)])], pcm=c1 == 1))
        # slack of 1..12 bits inside part2_3_length, in all four positions of a frame; behind the last unit: the frame's fill bytes
        for slack in range(1, 13):
            pos = (slack - 1) % 4
            body = U(c1=c1, ts=(5, 5, 5), pairs=[(3, -3), (1, 0)], quads=[(0, 1, 1, 0)])
            nbits = pair_bits(5, 3, 3) + pair_bits(5, 1, 0) + (4 if c1 else int(books()[32][1][6])) + 2
            body["p23"] = nbits + slack
            units = [filler(k) for k in range(pos)] + [body]
            units += [U(ts=(1, 1, 1), pairs=[(1, -1)] * 6, sfc=0)] if pos < 3 else []
            out.append(Stream("count1/slack%d_c1%d_unit%d" % (slack, c1, pos), [frame(units, fill=0xA7 if slack % 2 else 0xFF)]))
    return out


def family_against_part2_3_length():
    out = []
    t, big = LONGEST[0], LONGEST[1:]
    nbig = pair_bits(t, *big)
    lead = [(1, -1), (15, 0), (-14, 14)]
    nlead = sum(pair_bits(t, x, y) for x, y in lead)
    nxt = U(ts=(1, 1, 1), bv=4, p23=40)                                # reads what lies there: the overhang of the unit in front, then zeros
    # the last pair ends at max_bit, straddles it by 1 bit and by all but its first bit; starts at max_bit; starts at max_bit + 1
    for name, p23 in (("ends_at", nlead + nbig), ("straddles_1", nlead + nbig - 1), ("straddles_all_but_1", nlead + 1), ("starts_at", nlead),
                      ("starts_behind", nlead - 1)):
        u = U(ts=(t, t, t), pairs=lead + [big], p23=p23)
        out.append(Stream("p23/" + name, [frame([filler(), u, dict(nxt, p23=nbig + 30), filler(3)], fill=0x5C)], pcm=name in ("straddles_1", "starts_at")))
        out.append(Stream("p23/" + name + "_last_unit", [frame([filler(), filler(1), filler(2), u], fill=0xE3)]))
    out.append(Stream("p23/zero_with_big_values", [frame([filler(), U(ts=(7, 7, 7), bv=3, p23=0), U(ts=(7, 7, 7), pairs=[(5, -5), (0, 1), (2, 2)])])]))
    out += family_part2()
    return out


def family_part2(sr=0, mono=False, tag=""):
    """a scalefactor part longer than part2_3_length, without and with big values (those start behind max_bit: flagged), long and short.
    The unit's own bits are longer than its part2_3_length: what follows starts inside them, so it writes nothing of its own."""
    out = []
    for sfc in (15, 4):
        for bv in (0, 2):
            for short in (0, 1):
                u = U(sfc=sfc, ws=short, bt=2 * short, ts=(8, 8, 0) if short else (8, 8, 8), pairs=[(5, -1), (-2, 3)][:bv], p23=7, sf=4)
                units = ([] if mono else [filler()]) + [u, U(ts=(2, 2, 2), bv=2, p23=170)] + ([] if mono else [filler(5)])
                out.append(Stream("part2%s/longer_sfc%d_bv%d_short%d" % (tag, sfc, bv, short), [frame(units, mono=mono), frame([filler(1)], mono=mono)], sr=sr, mono=mono))
    return out


def family_staging(sr=0, mono=False, tag=""):
    """a unit of part2_3_length = 4095 that starts at bit offset 31 (mod 32) and whose last pair, the longest the books allow, starts at
    max_bit - 1: the staging clamp to W and HUF_WORDS_MAX are the limiting quantities"""
    out = []
    t, big = LONGEST[0], LONGEST[1:]
    for p23 in (4095, 4094, 4064, 4002, 4001):        # (4001: the longest unit whose staging is not clamped to HUF_WORDS_MAX)
        # region 0 (lines 0..23 at every rate) holds twelve pairs of book 1 that make the length come out: (0, 0), (0, 1) and (1, -1)
        l0, l1, l2 = pair_bits(1, 0, 0), pair_bits(1, 0, 1), pair_bits(1, 1, -1)
        body, nbits, k = [], 0, 0
        while True:
            x, y = ((15 + (977 * k) % 8192) * (-1) ** k, (k * 7) % 16 * (-1) ** (k // 2))
            if nbits + pair_bits(t, x, y) > p23 - 1 - 12 * l0 - 6:
                break
            body.append((x, y))
            nbits += pair_bits(t, x, y)
            k += 1
        rest = p23 - 1 - nbits                                        # the last pair starts at max_bit - 1
        a, b = next((a, b) for a in range(13) for b in range(13 - a) if a * l1 + b * l2 + (12 - a - b) * l0 == rest)
        pairs = [(0, 1)] * a + [(1, -1)] * b + [(0, 0)] * (12 - a - b) + body + [big]
        assert len(pairs) <= 288
        u = U(ts=(1, t, t), r0c=5, r1c=0, pairs=pairs, p23=p23)
        first = U(quads=pad_quads(31))                                # 31 bits in front: the worst unit starts at bit 31
        units = [first, u]
        nxt = [U(ts=(1, 1, 1), bv=3, p23=60), filler(7)] if not mono else []
        out.append(Stream("staging%s/p23_%d" % (tag, p23), [frame(units + nxt, mono=mono, fill=0x96), frame([filler()], mono=mono)], sr=sr, mono=mono,
                          bitrate=14, pcm=p23 == 4095 and not tag))
    return out


def family_end_of_data():
    """the file ends inside the last frame's main data: inside a scalefactor, a code word, either escape, in front of either sign bit,
    inside count1; bits past the end read as 0.  The file ends on a byte, so the units in front are lengthened until the place is one."""
    out = []
    t = 23
    pairs = [(8206, -8206), (-8000, 15), (3, 3)]
    n2, code = 11 * 4 + 10 * 3, hlen(16, 15, 15)
    marks = {"in_scalefactor": 38, "in_code_word": n2 + 3, "in_x_linbits": n2 + code + 6, "at_x_sign": n2 + code + 13, "in_y_linbits": n2 + code + 14 + 6,
             "at_y_sign": n2 + code + 27, "in_count1": n2 + sum(pair_bits(t, x, y) for x, y in pairs) + 7}
    for name, at in marks.items():
        for k in range(8):
            lead = [filler(), dict(filler(1), quads=filler()["quads"] + pad_quads(k))]
            u = U(ts=(t, t, t), sfc=15, sf=6, pairs=pairs, quads=[(1, 1, 1, 1)] * 3)
            probe = Stream("probe", [frame(lead + [u])])
            if (probe.units[0][1][0]["start"] + at) % 8 == 0:
                break
        cut = (probe.units[0][1][0]["start"] + at) // 8
        out.append(Stream("end_of_data/" + name, [frame([filler(4)]), frame(lead + [u, filler(2)], fill=0xFF)], cut=cut, pcm=name == "in_x_linbits"))
    out.append(Stream("end_of_data/no_main_data", [frame([filler()]), frame([filler(1), U(ts=(t, t, t), sfc=15, sf=6, pairs=pairs)])], cut=0))
    return out


def family_scalefactors():
    out = []
    body = dict(ts=(2, 2, 2), pairs=[(2, -1), (1, 1)], quads=[(1, 0, 0, 1)])
    sbody = dict(ts=(2, 2, 0), pairs=[(2, -1), (1, 1)], quads=[(1, 0, 0, 1)])
    # every scalefac_compress with all-ones fields in long, short and mixed granules
    for sfc in range(16):
        units = [U(sfc=sfc, **body), U(sfc=sfc, ws=1, bt=2, sbg=(1, 0, 2), **sbody), U(sfc=sfc, ws=1, bt=2, mixed=1, **sbody), U(sfc=sfc, **body)]
        out.append(Stream("scalefactors/compress%d" % sfc, [frame(units)], pcm=sfc == 15))
    # all 16 scfsi patterns per channel in granule 1 behind a long granule 0
    for pat in range(16):
        a = [(pat >> k) & 1 for k in range(4)]
        b = [(pat >> (3 - k)) & 1 ^ 1 for k in range(4)]
        units = [U(sfc=13, sf=pat, **body), U(sfc=10, sf=pat + 3, **body), U(sfc=7, sf=1, **body), U(sfc=15, sf=2, **body)]
        out.append(Stream("scalefactors/scfsi%d" % pat, [frame(units, scfsi=[a, b])], pcm=pat == 5))
    # scfsi behind a short and behind a mixed granule 0 in the second and third frame: the values come from the frame before
    for kind, mixed in (("short", 0), ("mixed", 1)):
        f0 = frame([U(sfc=15, sf=1, **body), U(sfc=13, sf=2, **body), U(sfc=15, sf=3, **body), U(sfc=12, sf=4, **body)])
        f1 = frame([U(sfc=15, sf=5, ws=1, bt=2, mixed=mixed, **sbody), U(sfc=9, sf=6, ws=1, bt=2, mixed=mixed, **sbody), U(sfc=14, sf=7, **body), U(sfc=11, sf=8, **body)],
                   scfsi=[[1, 0, 1, 1], [1, 1, 0, 1]])
        f2 = frame([U(sfc=14, sf=9, ws=1, bt=2, mixed=mixed, **sbody), U(sfc=15, sf=10, ws=1, bt=2, mixed=1 - mixed, **sbody), U(sfc=13, sf=11, **body), U(sfc=15, sf=12, **body)],
                   scfsi=[[1, 1, 1, 1], [0, 1, 1, 0]])
        out.append(Stream("scalefactors/scfsi_behind_" + kind, [f0, f1, f2], pcm=True))
    # a start and a stop block with the mixed flag (requantised with the short scalefactors from band 8 on), behind short granules that wrote them
    f0 = frame([U(sfc=15, sf=1, ws=1, bt=2, **sbody), U(sfc=13, sf=2, ws=1, bt=2, mixed=1, **sbody), U(sfc=15, sf=3, ws=1, bt=2, **sbody), U(sfc=12, sf=4, ws=1, bt=2, **sbody)])
    f1 = frame([U(sfc=15, sf=5, ws=1, bt=1, mixed=1, **sbody), U(sfc=9, sf=6, ws=1, bt=3, mixed=1, **sbody), U(sfc=14, sf=7, ws=1, bt=3, mixed=1, **sbody),
                U(sfc=11, sf=8, ws=1, bt=1, mixed=1, **sbody)], scfsi=[[0, 1, 0, 0], [0, 0, 0, 0]])
    out.append(Stream("scalefactors/start_stop_mixed", [f0, f1], pcm=True))
    return out


_STREAMS = None


def streams():
    """name -> Stream, in a fixed order"""
    global _STREAMS
    if _STREAMS is None:
        lst = family_code_words() + family_escapes() + family_no_bits_books() + family_regions() + family_big_values() + family_count1_end()
        lst += family_against_part2_3_length() + family_staging() + family_end_of_data() + family_scalefactors()
        # the big_values limits, region bounds, part2 and staging worst case in mono and at the other sampling rates (other band tables)
        lst += family_big_values(sr=1, mono=True, tag="_mono48") + family_regions(sr=1, mono=True, tag="_mono48") + family_part2(sr=1, mono=True, tag="_mono48")
        lst += family_staging(sr=1, mono=True, tag="_mono48")
        for sr, tag in ((1, "_48"), (2, "_32")):
            lst += family_big_values(sr=sr, tag=tag) + family_regions(sr=sr, tag=tag) + family_part2(sr=sr, tag=tag) + family_staging(sr=sr, tag=tag)
        _STREAMS = {s.name: s for s in lst}
        assert len(_STREAMS) == len(lst)
    return _STREAMS


# (book, window) pairs -- window 0: 32 zero bits, 1: 32 one bits -- that no entry of the reference's code book matches (the reference then leaves
# the pair zero and the cursor in place).  The fixture's generator probes the reference's tables and asserts that this list is what it finds:
# the books are complete prefix codes, so there is none, and no stream has to be added for the case.
PROBE_NOMATCH = []


# What the case set comes to, by the model: the tests assert these numbers, so a change of the builders or of the model that moves a unit
# into or out of the flagged set shows up as a change of this table.  Keys 1, 2, 8: units flagged with MP3S_HS_BAD_REGION, _BIG_VALUES, _OVERRUN.
# Per builder: family_regions writes three bad region pairs with big_values 0 and 3 (6 units) and family_big_values 289, 511 with book 0 and
# 289 with a real book (3 units), each four times (stereo at three rates, mono); every such unit has a stream of its own, which the
# reference refuses.  Overruns (19 = 3 + 4 * 4): p23/starts_behind twice, p23/zero_with_big_values, and per family_part2 (four times, as above) the four streams with big values.
STATED = {"streams": 386, "frames": 544, "units": 2000, "refused_streams": 36, "flagged_streams": 55, HS_BAD_REGION: 24, HS_BIG_VALUES: 12, HS_OVERRUN: 19}
