"""The Huffman / scalefactor decode (k_dec_huffman, csrc/k_huffman.hpp, and its host twins) at its bit-stream edges: every code word of
every book, the escapes up to 8206, books that read no bits, the region bounds, the big_values limits, the end of count1 (D1), big values
against part2_3_length, the staging worst case, the end of the main data, and every way scalefactors are read or inherited
(tests/huffman_edges.py builds the streams and holds the bit-position model).

CPU half: the builders reproduce the fixture's inputs (tests/golden/g16_huffman_edges.npz, the upstream reference's own decode, made by
tests/golden/gen_huffman_edges_golden.py), the case set reaches what it is meant to reach, and the model, the oracle, the host parser and
the one-frame host decode equal the fixture.  GPU half: the kernel alone, under every launch shape, with other neighbours in the wave, behind
the device parser, and end to end.  Every comparison is bit-exact; which frames the kernel flags is fixed by the model, never measured."""
import os

import numpy as np
import pytest

import huffman_edges as H

LANES = (32, 8, 16, 62, 64)


@pytest.fixture(scope="module")
def S():
    return H.streams()


@pytest.fixture(scope="module")
def fix(golden_dir):
    g = np.load(os.path.join(golden_dir, "g16_huffman_edges.npz"))
    names = [str(s) for s in g["names"]]
    start = np.concatenate([[0], np.cumsum(g["n_frames"])])
    pstart = np.concatenate([[0], np.cumsum(g["pcm_frames"])])
    out = {"names": names, "in_digest": dict(zip(names, g["in_digest"].tolist())), "probe_nomatch": g["probe_nomatch"],
           "raises": dict(zip(names, [str(s) for s in g["raises"]])), "raises_at": dict(zip(names, g["raises_at"].tolist())),
           "pcm": {str(n): g["pcm_digest"][pstart[i]:pstart[i + 1]] for i, n in enumerate(g["pcm_names"])}}
    for k in ("is", "scale_fac_l", "scale_fac_s"):
        a = g[k]
        a.setflags(write=False)
        out[k] = {n: a[start[i]:start[i + 1]] for i, n in enumerate(names)}
    return out


def kernel_masks(units, nch):
    """the scalefactor entries the requantiser reads of a frame's units, as the kernel leaves them (own bits, scfsi copies, inherited
    entries): -> bool [2][2][22], bool [2][2][3][13]"""
    ml, ms = np.zeros((2, 2, 22), dtype=bool), np.zeros((2, 2, 3, 13), dtype=bool)
    for gr in range(2):
        for ch in range(nch):
            u = units[gr][ch]["side"]
            if u["ws"] and u["bt"] == 2:
                ms[gr, ch, :, :12] = True
                if u["mixed"]:
                    ml[gr, ch, :8] = True
            else:
                ml[gr, ch, :21] = True
                if u["ws"] and u["mixed"]:
                    ms[gr, ch, :, 8:12] = True
    return ml, ms


def own_masks(units, nch):
    """the entries a frame determines by itself: what its units read from their own bits, and what scfsi copies from a granule 0 that read it"""
    ml, ms = np.zeros((2, 2, 22), dtype=bool), np.zeros((2, 2, 3, 13), dtype=bool)
    for gr in range(2):
        for ch in range(nch):
            u, scfsi = units[gr][ch]["side"], units[gr][ch]["scfsi"]
            if u["ws"] and u["bt"] == 2:
                ms[gr, ch, :, 3 if u["mixed"] else 0:12] = True
                if u["mixed"]:
                    ml[gr, ch, :8] = True
            elif gr == 0:
                ml[gr, ch, :21] = True
            else:
                for s in range(21):
                    band = 0 if s < 6 else (1 if s < 11 else (2 if s < 16 else 3))
                    ml[gr, ch, s] = not scfsi[band] or ml[0, ch, s]
    return ml, ms


def compare_frame(tag, isv, si, f_is, f_l, f_s, masks, nch):
    assert np.array_equal(isv[:, :nch], f_is[:, :nch]), (tag, "spectra", np.argwhere(isv[:, :nch] != f_is[:, :nch])[:4].tolist())
    ml, ms = masks
    assert np.array_equal(si["scale_fac_l"][ml], f_l[ml]), (tag, "scale_fac_l")
    assert np.array_equal(si["scale_fac_s"][ms], f_s[ms]), (tag, "scale_fac_s")


def side_fields_equal(tag, si, units, nch):
    """every other field of mp3s_granule_si against the side info the model parsed"""
    for gr in range(2):
        for ch in range(nch):
            u, g = units[gr][ch]["side"], si[gr, ch]
            got = (int(g["global_gain"]), int(g["scalefac_scale"]), int(g["block_type"]), int(g["mixed_block_flag"]), int(g["preflag"]), tuple(int(v) for v in g["sub_block_gain"]))
            assert got == (u["gg"], u["sfs"], u["bt"], u["mixed"], u["pre"], tuple(u["sbg"])), (tag, gr, ch)


def expected_status(m, bound=4095):
    """the OR of MP3S_HS_* over a stream by the model, for a caller's bound on part2_3_length: a unit above the bound is reported with
    MP3S_HS_HINT and not decoded (no overrun is seen in it)"""
    st = 0
    for rec in m["units"]:
        for gr in range(2):
            for ch in range(m["nch"]):
                r = rec[gr][ch]
                st |= (r["flags"] & ~H.HS_OVERRUN) | H.HS_HINT if r["side"]["p23"] > bound else r["flags"]
    return st


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_builders_reproduce_the_fixture_inputs(S, fix):
    assert list(S) == fix["names"]
    for n, s in S.items():
        assert H.input_digest(s.data) == fix["in_digest"][n], n
    assert sorted(map(tuple, fix["probe_nomatch"].tolist())) == sorted(H.PROBE_NOMATCH)


def test_model_equals_the_reference(S, fix):
    """the bit-position model reads every stream as the reference does: same lines in every frame the reference decoded, and it names
    the streams the reference refuses, with the frame"""
    refused = 0
    for n, s in S.items():
        m = H.model(s.data)
        k = len(fix["is"][n])
        assert fix["raises_at"][n] == m["refused_at"], n
        assert k == (s.n_frames if m["refused_at"] < 0 else m["refused_at"]), n
        assert np.array_equal(m["lines"][:k, :, :s.nch], fix["is"][n][:, :, :s.nch]), n
        if m["refused_at"] >= 0:
            assert fix["raises"][n] == "IndexError", n
            refused += 1
        for f in range(k):                                     # the scalefactor fields a unit reads from its own bits
            for gr in range(2):
                for ch in range(s.nch):
                    r = m["units"][f][gr][ch]
                    u = r["side"]
                    if u["ws"] and u["bt"] == 2:
                        sf = list(r["sf"])
                        if u["mixed"]:
                            assert fix["scale_fac_l"][n][f, gr, ch, :8].tolist() == sf[:8], n
                            del sf[:8]
                            got = fix["scale_fac_s"][n][f, gr, ch, :, 3:12].T.reshape(-1).tolist()
                        else:
                            got = fix["scale_fac_s"][n][f, gr, ch, :, :12].T.reshape(-1).tolist()
                        assert got == sf, (n, f, gr, ch)
                    elif gr == 0:
                        assert fix["scale_fac_l"][n][f, gr, ch, :21].tolist() == r["sf"], (n, f, gr, ch)
    assert refused == H.STATED["refused_streams"]


def test_flagged_units_are_what_the_builder_states(S):
    """the set of units the kernel must flag is a condition: its size per bit is stated in huffman_edges.py"""
    count = {"streams": len(S), "frames": 0, "units": 0, "refused_streams": 0, "flagged_streams": 0, H.HS_BAD_REGION: 0, H.HS_BIG_VALUES: 0, H.HS_OVERRUN: 0}
    for n, s in S.items():
        m = H.model(s.data)
        count["frames"] += s.n_frames
        count["units"] += 2 * s.nch * s.n_frames
        count["refused_streams"] += m["refused_at"] >= 0
        count["flagged_streams"] += m["flags"] != 0
        for rec in m["units"]:
            for gr in range(2):
                for ch in range(s.nch):
                    for b in (H.HS_BAD_REGION, H.HS_BIG_VALUES, H.HS_OVERRUN):
                        count[b] += bool(rec[gr][ch]["flags"] & b)
        assert expected_status(m) == m["flags"]
    print(count)
    assert count == H.STATED


def test_builder_positions_equal_the_model(S):
    """where a well-formed unit was written is where the reference's cursor reads it: unit start, max_bit, every pair and quadruple"""
    checked = 0
    for n, s in S.items():
        m = H.model(s.data)
        for f in range(s.n_frames):
            for gr in range(2):
                for ch in range(s.nch):
                    b, r = s.units[f][gr][ch], m["units"][f][gr][ch]
                    assert (b["start"], b["max_bit"]) == (r["start"], r["max_bit"]), n
                    if r["flags"] or b["written"] == 0 or b["at"] != b["start"] or b["bv"] != len(b["pair_bits"]) or (s.cut is not None and f == s.n_frames - 1):
                        continue
                    assert b["part2_end"] == r["part2_end"] and b["pair_bits"] == r["pair_bits"], (n, f, gr, ch)
                    k = min(len(b["quad_bits"]), len(r["quad_bits"]))
                    assert b["quad_bits"][:k] == r["quad_bits"][:k], (n, f, gr, ch)
                    checked += 1
    assert checked > 800


def census(S):
    c = dict(pairs=set(), quads=set(), values=set(), straddle=set(), starts=set(), bv=set(), align={}, d1=set(), last_quad=set(), slack=set(), nobits=set(),
             cut=set(), part2=set(), scfsi=set(), regions=set())
    for n, s in S.items():
        m = H.model(s.data)
        for f in range(s.n_frames):
            for gr in range(2):
                for ch in range(s.nch):
                    r, b = m["units"][f][gr][ch], s.units[f][gr][ch]
                    u = r["side"]
                    c["bv"].add((u["bv"], any(u["ts"])))
                    c["part2"].add((u["sfc"], "short" if u["ws"] and u["bt"] == 2 and not u["mixed"] else ("mixed" if u["ws"] and u["bt"] == 2 else "long")))
                    if gr == 1 and not (u["ws"] and u["bt"] == 2):
                        g0 = m["units"][f][0][ch]["side"]
                        c["scfsi"].add((tuple(r["scfsi"]), "short" if g0["ws"] and g0["bt"] == 2 and not g0["mixed"] else ("mixed" if g0["ws"] and g0["bt"] == 2 else "long"), f))
                    if not (u["ws"] and u["bt"] == 2):
                        r0c, r1c = (7, 13) if u["ws"] else (u["r0c"], u["r1c"])
                        c["regions"].add((r0c + 1, r0c + r1c + 2, s.sr, s.nch))
                    if r["flags"] & (H.HS_BAD_REGION | H.HS_BIG_VALUES):
                        continue
                    ends = r["pair_bits"][1:] + [r["pairs_end"]] if r["pair_bits"] else []
                    for p, (at, end) in enumerate(zip(r["pair_bits"], ends)):
                        t = H.book_at(u, s.sr, 2 * p)
                        x, y = int(r["lines"][2 * p]), int(r["lines"][2 * p + 1])
                        if t in (0, 4, 14):
                            c["nobits"].add((t, 0 if 2 * p < H.regions(u, s.sr)[0] else (1 if 2 * p < H.regions(u, s.sr)[1] else 2)))
                            continue
                        if at < r["max_bit"] or end <= r["max_bit"]:
                            c["pairs"].add((t, x, y))
                            c["align"].setdefault((t, abs(x), abs(y)), set()).add(at % 32)
                        for k, v in enumerate((x, y)):
                            if abs(v) == H.VALUE_MAX:
                                c["values"].add((k, v))
                        if p == len(ends) - 1:
                            c["starts"].add(at - r["max_bit"])
                            if at <= r["max_bit"] < end:
                                c["straddle"].add((end - r["max_bit"], end - at))
                    for q, at in enumerate(r["quad_bits"]):
                        line = 2 * u["bv"] + 4 * q
                        c["quads"].add((u["c1"],) + tuple(int(v) for v in r["lines"][line:line + 4]))
                    if r["quad_bits"]:
                        c["last_quad"].add((u["c1"], 2 * u["bv"] + 4 * (len(r["quad_bits"]) - 1), r["end_bit"] - r["max_bit"]))
                    if r["end_bit"] < r["max_bit"]:                  # bits were left: D1 ended count1
                        c["d1"].add((u["c1"], u["bv"], r["end_line"]))
                    if b["written"] and b["p23"] > b["written"] and b["at"] == b["start"]:
                        c["slack"].add((b["p23"] - b["written"], gr * 2 + ch, u["c1"]))
        if s.cut is not None:                                # what the file's end falls into: which part of which unit of the last frame
            end = 8 * m["md_len"][-1]
            for gr in range(2):
                for ch in range(s.nch):
                    b = s.units[-1][gr][ch]                      # (the builder's positions: what is cut no longer decodes to what was written)
                    if b["start"] < end < b["at"] + b["written"] and b["pair_bits"] and b["quad_bits"]:
                        p0, code, lb = b["pair_bits"][0], H.hlen(16, 15, 15), 13
                        edges = [("scalefactor", b["part2_end"]), ("code_word", p0 + code), ("x_linbits", p0 + code + lb), ("x_sign", p0 + code + lb + 1),
                                 ("y_linbits", p0 + code + 2 * lb + 1), ("y_sign", p0 + code + 2 * lb + 2), ("pairs", b["quad_bits"][0]), ("count1", b["at"] + b["written"])]
                        c["cut"].add(next(k for k, e in edges if end < e))           # the field whose first missing bit is the file's end
            if end == 0:
                c["cut"].add("empty")
    return c


@pytest.fixture(scope="module")
def cen(S):
    return census(S)


def test_census_every_code_word(cen):
    for t in H.BIG_BOOKS + H.ESC_BOOKS:
        base = 16 if 16 <= t < 24 else (24 if t >= 24 else t)
        if t in H.BIG_BOOKS:
            want = {(t, x, y) for x, y in H.all_pairs(t)}
            assert want <= cen["pairs"], (t, sorted(want - cen["pairs"])[:5])
        if t in H.ESC_BOOKS:
            vals = H.escape_values(t)
            want = {(t, x, y) for a in vals for b in vals for x, y in H.signed((a, b))}
            assert want <= cen["pairs"], (t, sorted(want - cen["pairs"])[:5])
        assert base in H.BIG_BOOKS
    for c1 in (0, 1):
        want = {(c1,) + q for i in range(16) for q in H.signed(((i >> 3) & 1, (i >> 2) & 1, (i >> 1) & 1, i & 1))}
        assert len(want) == 81 and want <= cen["quads"], c1
    assert cen["nobits"] == {(t, r) for t in (0, 4, 14) for r in range(3)}


def test_census_extreme_values_and_alignments(cen):
    assert cen["values"] == {(0, 8206), (0, -8206), (1, 8206), (1, -8206)}
    for t in (23, 24, 31):
        x, y = H.longest_code(t)
        top = 15 + (1 << H.LINBITS[t]) - 1
        assert cen["align"][(t, x, y)] >= set(range(32)), t                    # the longest code word at every alignment
        assert cen["align"][(t, top, top)] >= set(range(32)), t                # and both escapes behind it
    for t in (13, 15, 16, 24):                                                 # the widest books at three alignments of their first code word
        x, y = H.all_pairs(t)[0]
        assert len(cen["align"][(t, abs(x), abs(y))]) >= 3, t


def test_census_limits(cen):
    longest = H.pair_bits(*H.LONGEST)
    assert longest == 36 == max(H.pair_bits(t, x if x < 15 else 15 + (1 << H.LINBITS[t]) - 1, y if y < 15 else 15 + (1 << H.LINBITS[t]) - 1)
                                for t in H.ESC_BOOKS for x in range(16) for y in range(16))
    # the last pair against max_bit: ends on it, straddles it by one bit and by all but its first bit (the pair of the most bits that the
    # books allow has 36: 19-bit code words exist, but not for (15, 15)), starts on it, starts one bit behind it (flagged)
    assert {(1, longest), (longest - 1, longest)} <= cen["straddle"]
    assert {-longest, 0, 1} <= cen["starts"]
    for books_used in (False, True):
        assert {0, 287, 288} <= {bv for bv, used in cen["bv"] if used == books_used}
    assert {289, 511} <= {bv for bv, _ in cen["bv"]}
    for c1 in (0, 1):
        # big_values 283..287 with count1 bits to spare: D1 stops in front of line 572 + 4
        # (283: quadruples at 566 and 570, none at 574; 284: one at 568, none at 572; 285: one at 570; 286 and 287: none at 572 / 574)
        assert {(c1, 283, 574), (c1, 284, 572), (c1, 285, 574), (c1, 286, 572), (c1, 287, 574)} <= cen["d1"], c1
        assert any(k[0] == c1 and k[1] == 568 for k in cen["last_quad"])       # quadruples all the way
        assert any(k[0] == c1 and k[2] == 0 for k in cen["last_quad"])         # the last quadruple ends on max_bit
        assert {(s, (s - 1) % 4, c1) for s in range(1, 13)} <= cen["slack"]
    assert {(sfc, kind) for sfc in range(16) for kind in ("long", "short", "mixed")} <= cen["part2"]
    pats = {k[0] for k in cen["scfsi"] if k[1] == "long"}
    assert len(pats) == 16
    assert {("short", 1), ("short", 2), ("mixed", 1), ("mixed", 2)} <= {(k[1], k[2]) for k in cen["scfsi"] if any(k[0])}
    for sr, nch in ((0, 2), (1, 2), (2, 2), (1, 1)):
        assert {(16, 22), (14, 22), (15, 23), (16, 23), (16, 24)} <= {k[:2] for k in cen["regions"] if k[2:] == (sr, nch)}
    assert cen["cut"] == {"scalefactor", "code_word", "x_linbits", "x_sign", "y_linbits", "y_sign", "count1", "empty"}


def test_staging_worst_case_is_in_the_set(S):
    """a unit of 4095 bits that starts at bit 31 (mod 32) and whose last pair, the longest there is, starts one bit in front of max_bit"""
    for tag, nch in (("", 2), ("_48", 2), ("_32", 2), ("_mono48", 1)):
        m = H.model(S["staging%s/p23_4095" % tag].data)
        r = m["units"][0][0][1] if nch == 2 else m["units"][0][1][0]
        assert r["start"] % 32 == 31 and r["side"]["p23"] == 4095 and m["max_p23"] == 4095
        assert r["pair_bits"][-1] == r["max_bit"] - 1 and r["pairs_end"] == r["max_bit"] + 35 and r["flags"] == 0
        assert int(r["lines"][2 * len(r["pair_bits"]) - 2]) == 8206


def test_oracle_equals_the_reference(orc, S, fix):
    for n, s in S.items():
        r = orc.decode(s.data)
        if fix["raises_at"][n] >= 0:
            assert r["rc"] != 0, n
            continue
        assert r["rc"] == 0 and r["n_frames"] == s.n_frames and r["channels"] == s.nch, n
        assert np.array_equal(r["is"][:, :, :s.nch], fix["is"][n][:, :, :s.nch]), n
        assert np.array_equal(r["frames"]["scale_fac_l"][:, :, :s.nch], fix["scale_fac_l"][n][:, :, :s.nch]), n
        assert np.array_equal(r["frames"]["scale_fac_s"][:, :, :s.nch], fix["scale_fac_s"][n][:, :, :s.nch]), n
        if n in fix["pcm"]:
            assert np.array_equal(H.frame_digests(r["pcm"][:s.n_frames * 1152]), fix["pcm"][n]), n


def test_host_parser_equals_the_reference(mlib, S, fix):
    for n, s in S.items():
        if fix["raises_at"][n] >= 0:
            with pytest.raises(mlib.Mp3sError) as e:
                mlib.parse_stream(s.data)
            assert e.value.code == mlib.E_MALFORMED, n
            continue
        p = mlib.parse_stream(s.data)
        assert p["n_frames"] == s.n_frames and p["channels"] == s.nch, n
        assert np.array_equal(p["is"][:, :, :s.nch], fix["is"][n][:, :, :s.nch]), n
        assert np.array_equal(p["si"]["scale_fac_l"][:, :, :s.nch], fix["scale_fac_l"][n][:, :, :s.nch]), n
        assert np.array_equal(p["si"]["scale_fac_s"][:, :, :s.nch], fix["scale_fac_s"][n][:, :, :s.nch]), n


def test_one_frame_host_decode_equals_the_reference(mlib, S, fix):
    """mp3s_debug_parse_scanned_frame, the path the frames take that the kernel flags, on every frame of every accepted stream: the
    spectra, and every scalefactor the frame determines by itself"""
    L = mlib.lib()
    for n, s in S.items():
        if fix["raises_at"][n] >= 0:
            continue
        sc = mlib.scan_stream(s.data)
        m = H.model(s.data)
        assert sc["n_frames"] == s.n_frames and sc["max_part2_3_length"] == m["max_p23"], n
        side, blob = np.ascontiguousarray(sc["side"]), np.ascontiguousarray(sc["blob"])
        for f in range(s.n_frames):
            isv = np.zeros((2, 2, 576), dtype=np.int16)
            si = np.zeros((2, 2), dtype=mlib.GRANULE_SI_DTYPE)
            mlib.check(L.mp3s_debug_parse_scanned_frame(side[f:f + 1].ctypes.data, blob.ctypes.data, isv.ctypes.data, si.ctypes.data))
            compare_frame((n, f), isv, si, fix["is"][n][f], fix["scale_fac_l"][n][f], fix["scale_fac_s"][n][f], own_masks(m["units"][f], s.nch), s.nch)
            side_fields_equal((n, f), si, m["units"][f], s.nch)


# ---------------------------------------------------------------------------------------------------------------- GPU
def batch_of(mlib, S, names):
    """the scanned streams as one batch: blob and side records concatenated, md_off moved, reserved = the stream's first frame"""
    blobs, sides, first, at, nf = [], [], {}, 0, 0
    for n in names:
        sc = mlib.scan_stream(S[n].data)
        side = sc["side"].copy()
        side["md_off"] += at
        side["reserved"] = nf
        blob = sc["blob"].tobytes()
        blob += bytes(8 + (-len(blob) - 8) % 4)
        blobs.append(blob)
        sides.append(side)
        first[n] = nf
        at += len(blob)
        nf += len(side)
    return np.frombuffer(b"".join(blobs) + bytes(16), dtype=np.uint8), np.concatenate(sides), first


def run_kernel(ctx, mlib, blob, side, nch, bound):
    L = mlib.lib()
    n = len(side)
    d_blob, d_side = ctx.to_device(blob), ctx.to_device(side)
    d_is, d_si, d_st = ctx.alloc(n * 2304 * 2), ctx.alloc(n * 4 * 72), ctx.alloc(4)
    try:
        ctx.upload(d_is, np.full(n * 2304, 0x5a5a, dtype=np.int16))
        mlib.check(L.mp3s_huffman_decode_dev(ctx.handle, d_blob, d_side, n, nch, int(bound), d_is, d_si, d_st))
        ctx.sync()
        return (int(ctx.download(d_st, np.int32, (1,))[0]), ctx.download(d_is, np.int16, (n, 2, 2, 576)), ctx.download(d_si, mlib.GRANULE_SI_DTYPE, (n, 2, 2)))
    finally:
        for q in (d_blob, d_side, d_is, d_si, d_st):
            ctx.free(q)


def clean_names(S, nch):
    return [n for n, s in S.items() if s.nch == nch and H.model(s.data)["flags"] == 0]


def check_rows(S, fix, names, first, isv, si, nch):
    for n in names:
        m = H.model(S[n].data)
        assert not isv[first[n]:first[n] + S[n].n_frames, :, nch:].any(), n
        for f in range(S[n].n_frames):
            g = first[n] + f
            compare_frame((n, f), isv[g], si[g], fix["is"][n][f], fix["scale_fac_l"][n][f], fix["scale_fac_s"][n][f], kernel_masks(m["units"][f], nch), nch)
            side_fields_equal((n, f), si[g], m["units"][f], nch)


@pytest.mark.gpu
def test_kernel_alone_on_the_clean_batch(ctx, mlib, S, fix):
    for nch in (2, 1):
        names = clean_names(S, nch)
        # the whole batch, then without its longest units: each bound is met exactly by a unit of the batch (4095, 4002: staging clamped to
        # HUF_WORDS_MAX; 4001: the longest that is not; 2000: a bound among the everyday ones)
        for limit in (4095, 4002, 4001, 2000):
            part = [n for n in names if H.model(S[n].data)["max_p23"] <= limit]
            blob, side, first = batch_of(mlib, S, part)
            bound = max(H.model(S[n].data)["max_p23"] for n in part)
            assert bound == limit or limit == 2000
            for b in (bound, 0) if limit == 4095 else (bound,):
                st, isv, si = run_kernel(ctx, mlib, blob, side, nch, b)
                assert st == 0, (nch, b, st)
                check_rows(S, fix, part, first, isv, si, nch)
            assert run_kernel(ctx, mlib, blob, side, nch, bound - 1)[0] == H.HS_HINT


@pytest.mark.gpu
def test_kernel_flags_exactly_what_the_model_flags(ctx, mlib, S, fix):
    """one call per stream that must be flagged: the status word is the model's OR of bits, no bit more and none fewer; the frames the model
    does not flag equal the fixture (behind the frame at which the reference gives up: the model, which equals the fixture everywhere else)"""
    flagged = [n for n, s in S.items() if H.model(s.data)["flags"]]
    assert len(flagged) == H.STATED["flagged_streams"]
    for n in flagged:
        s, m = S[n], H.model(S[n].data)
        blob, side, _ = batch_of(mlib, S, [n])
        bounds = [m["max_p23"], 0] + ([m["max_p23"] - 1] if m["max_p23"] >= 2 else [])
        for b in bounds:
            st, isv, si = run_kernel(ctx, mlib, blob, side, s.nch, b)
            assert st == expected_status(m, b if b else 4095), (n, b, st)
            if b == bounds[-1] and len(bounds) == 3:
                assert st & H.HS_HINT
                continue
            for f in range(s.n_frames):
                if m["frame_flags"][f]:
                    continue
                if f < len(fix["is"][n]):
                    compare_frame((n, f), isv[f], si[f], fix["is"][n][f], fix["scale_fac_l"][n][f], fix["scale_fac_s"][n][f], kernel_masks(m["units"][f], s.nch), s.nch)
                else:
                    assert np.array_equal(isv[f, :, :s.nch], m["lines"][f, :, :s.nch]), (n, f)
                side_fields_equal((n, f), si[f], m["units"][f], s.nch)


@pytest.mark.gpu
def test_kernel_under_every_launch_shape(ctx, mlib, S, fix):
    old = ctx.get_option("huf_lanes")
    try:
        for nch in (2, 1):
            names = clean_names(S, nch)
            blob, side, first = batch_of(mlib, S, names)
            for lanes in LANES:
                ctx.set_option("huf_lanes", lanes)
                st, isv, si = run_kernel(ctx, mlib, blob, side, nch, 4095)
                assert st == 0, (nch, lanes, st)
                check_rows(S, fix, names, first, isv, si, nch)
            # (shapes that the staging of 4095-bit units does not fit fall back to a narrower one: again with short units only)
            names = [n for n in names if H.model(S[n].data)["max_p23"] <= 900]
            blob, side, first = batch_of(mlib, S, names)
            bound = max(H.model(S[n].data)["max_p23"] for n in names)
            for lanes in LANES:
                ctx.set_option("huf_lanes", lanes)
                st, isv, si = run_kernel(ctx, mlib, blob, side, nch, bound)
                assert st == 0, (nch, lanes, st)
                check_rows(S, fix, names, first, isv, si, nch)
    finally:
        ctx.set_option("huf_lanes", old)


@pytest.mark.gpu
def test_kernel_with_other_neighbours(ctx, mlib, S, fix):
    """the clean batch in reversed and in interleaved stream order: units that end at different multiples of 16 pairs share a wave in another
    way (the tile loop's early end and the zero fill behind it), every stream's rows stay what they are"""
    for nch in (2, 1):
        names = clean_names(S, nch)
        half = (len(names) + 1) // 2
        inter = [n for pair in zip(names[:half], names[half:] + [None]) for n in pair if n is not None]
        assert sorted(inter) == sorted(names)
        for order in (names[::-1], inter):
            blob, side, first = batch_of(mlib, S, order)
            st, isv, si = run_kernel(ctx, mlib, blob, side, nch, 0)
            assert st == 0
            check_rows(S, fix, order, first, isv, si, nch)


@pytest.mark.gpu
def test_device_parse_then_kernel(ctx, mlib, S, fix):
    """walk -> device parse -> Huffman kernel on the clean streams the walk takes"""
    L = mlib.lib()
    taken = 0
    for nch in (2, 1):
        for n in clean_names(S, nch):
            data = S[n].data
            w = mlib.walk_stream(data)
            if not w["regular"] or not w["n_frames"]:
                continue
            m = H.model(data)
            nf = w["n_frames"]
            assert nf == S[n].n_frames and w["max_part2_3_length"] == m["max_p23"], n
            d_img = ctx.to_device(np.frombuffer(data + bytes(16), dtype=np.uint8))
            d_refs, d_streams = ctx.to_device(w["refs"]), ctx.to_device(w["stream"])
            d_side, d_hdr, d_blob = ctx.alloc(nf * 104), ctx.alloc(nf * 8), ctx.alloc(w["blob_len"] + 16)
            d_st = ctx.to_device(np.zeros(4, dtype=np.int32))
            d_is, d_si, d_hst = ctx.alloc(nf * 2304 * 2), ctx.alloc(nf * 4 * 72), ctx.alloc(16)
            try:
                mlib.check(L.mp3s_parse_frames_dev(ctx.handle, d_img, 0, d_refs, d_streams, nf, 0, d_side, d_hdr, d_blob, None, d_st))
                mlib.check(L.mp3s_huffman_decode_dev(ctx.handle, d_blob, d_side, nf, nch, w["max_part2_3_length"], d_is, d_si, d_hst))
                ctx.sync()
                assert int(ctx.download(d_hst, np.int32, (1,))[0]) == 0, n
                isv, si = ctx.download(d_is, np.int16, (nf, 2, 2, 576)), ctx.download(d_si, mlib.GRANULE_SI_DTYPE, (nf, 2, 2))
            finally:
                for q in (d_img, d_refs, d_streams, d_side, d_hdr, d_blob, d_st, d_is, d_si, d_hst):
                    ctx.free(q)
            check_rows(S, fix, [n], {n: 0}, isv, si, nch)
            taken += 1
    assert taken > 200


@pytest.fixture(scope="module")
def singles(ctx, mlib, S):
    """every stream decoded alone on the device (float64 PCM), or the error it raises; shared by the end-to-end tests"""
    out = {}
    for n, s in S.items():
        try:
            r = ctx.decode_stream(s.data, mlib.MP3S_PCM_F64)
            out[n] = (r["pcm"].tobytes(), r["n_frames"], r["channels"])
        except mlib.Mp3sError as e:
            out[n] = e
    return out


@pytest.mark.gpu
def test_end_to_end_equals_the_oracle_and_the_reference(mlib, orc, S, fix, singles):
    for n, s in S.items():
        got = singles[n]
        if fix["raises_at"][n] >= 0:
            assert isinstance(got, mlib.Mp3sError) and got.code == mlib.E_MALFORMED, n
            continue
        assert not isinstance(got, Exception), (n, got)
        o = orc.decode(s.data)
        assert o["rc"] == 0 and got[0] == o["pcm"].tobytes() and got[1:] == (o["n_frames"], o["channels"]), n
        if n in fix["pcm"]:
            pcm = np.frombuffer(got[0], dtype=np.float64).reshape(-1, s.nch)
            assert np.array_equal(H.frame_digests(pcm[:s.n_frames * 1152]), fix["pcm"][n]), n
    assert len(fix["pcm"]) >= 12


@pytest.mark.gpu
def test_end_to_end_as_one_batch(ctx, mlib, S, singles):
    """the whole list as one decode_streams batch: every member gets the result, or the status, it gets alone"""
    names = list(S)
    out = ctx.decode_streams([S[n].data for n in names], mlib.MP3S_PCM_F64, per_file=True)
    assert len(out) == len(names)
    for n, r in zip(names, out):
        alone = singles[n]
        if isinstance(alone, Exception):
            assert isinstance(r, mlib.Mp3sError) and r.code == alone.code, n
        else:
            assert not isinstance(r, Exception), (n, r)
            assert (r["pcm"].tobytes(), r["n_frames"], r["channels"]) == alone, n
