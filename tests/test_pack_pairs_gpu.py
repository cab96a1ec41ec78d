"""k_enc_pack on hand-made units (mp3s_pack_frames_dev) against the host formatter (mp3s_format_stream): every kind of pair,
book, count1 region, region bound, stuffing and error the packer's arithmetic tells apart, in batches of 2 and 3 frames.

The units are built in numpy; `check_coverage` asserts on the arrays that every case of the list is there before anything is
launched.  The generator and the formatter need no GPU: `test_pack_pairs_generator_cpu` runs them alone."""
import numpy as np
import pytest

MAXV = 8191 + 15                       # the largest magnitude the rate loop emits: linbits 13
PALETTE = (0, 1, -1, 14, -14, 15, -15, 16, -16, MAXV, -MAXV)


def _tables(mlib):
    t = mlib.debug_tables()
    return {"sfb": np.array(t["sfb_long"]), "h13": np.array(t["hlen13"]).astype(int), "h15": np.array(t["hlen15"]).astype(int),
            "h16": np.array(t["hlen16"]).astype(int), "h24": np.array(t["hlen24"]).astype(int),
            "c1a": np.array(t["hlen_c1a"]).astype(int), "lin": np.array(t["linbits"]).astype(int)}


def _hlen(T, book):
    return T["h13"] if book == 13 else T["h15"] if book == 15 else T["h16"] if book < 24 else T["h24"]


def _region_starts(T, sri, r0c, r1c):
    return int(T["sfb"][sri][r0c + 1]), int(T["sfb"][sri][r0c + r1c + 2])


def unit_bits(T, sri, ix, s):
    """the code bits of a unit, counted the way the format defines them (ISO 11172-3 2.4.2.7)"""
    r1s, r2s = _region_starts(T, sri, s["r0c"], s["r1c"])
    bits = 0
    for p in range(s["bv"]):
        book = s["ts"][(2 * p >= r1s) + (2 * p >= r2s)]
        if not book:
            continue
        x, y = abs(int(ix[2 * p])), abs(int(ix[2 * p + 1]))
        lb = int(T["lin"][book]) if book > 15 else 0
        assert max(x, y) <= (15 + (1 << lb) - 1 if lb else 15), (book, x, y)
        bits += int(_hlen(T, book)[min(x, 15) * 16 + min(y, 15)]) + (x != 0) + (y != 0) + lb * ((x > 14) + (y > 14))
    for q in range(s["c1"]):
        v = [abs(int(a)) for a in ix[2 * s["bv"] + 4 * q: 2 * s["bv"] + 4 * q + 4]]
        assert max(v) <= 1
        bits += (int(T["c1a"][v[0] + 2 * v[1] + 4 * v[2] + 8 * v[3]]) if s["c1sel"] == 0 else 4) + sum(v)
    return bits


def make_unit(T, sri, s, seed):
    """ix[576] of a unit from its description: big-value pairs cycle through every (x, y) of the book's palette, every
    `every`-th pair (the others are (0, 0)); count1 values cycle through 0 / +1 / -1; nothing behind count1"""
    rng = np.random.RandomState(seed)
    ix = np.zeros(576, dtype=np.int16)
    r1s, r2s = _region_starts(T, sri, s["r0c"], s["r1c"])
    n_used = {}
    for p in range(s["bv"]):
        book = s["ts"][(2 * p >= r1s) + (2 * p >= r2s)]
        if s.get("all_max"):
            ix[2 * p], ix[2 * p + 1] = (MAXV, -MAXV) if p & 1 else (-MAXV, MAXV)
            continue
        if p % s.get("every", 1):
            continue
        if book == 0:
            pal = (0, 3, -7, 20, -MAXV)                      # a region without a book: its values are not coded
        else:
            lb = int(T["lin"][book]) if book > 15 else 0
            top = 15 + (1 << lb) - 1 if lb else 15
            pal = tuple(v for v in PALETTE if abs(v) <= top)
        combos = [(a, b) for a in pal for b in pal]
        k = n_used.get(book, 0)
        n_used[book] = k + 1
        ix[2 * p], ix[2 * p + 1] = combos[(k * 7 + seed) % len(combos)] if k >= len(pal) * 2 else ((pal[k // 2], 0) if k % 2 == 0 else (0, pal[k // 2]))
    c = rng.randint(-1, 2, size=4 * s["c1"]).astype(np.int16)
    if s["c1"]:
        c[-4:] = (1, 0, 0, -1)                              # the last quadruple is not empty
        c[:8] = (1, -1, -1, 1, 0, 1, 1, 0)[:len(c[:8])]
    ix[2 * s["bv"]: 2 * s["bv"] + 4 * s["c1"]] = c
    return ix


def U(bv, c1, ts, r0c, r1c, c1sel=0, **kw):
    d = {"bv": bv, "c1": c1, "ts": tuple(ts), "r0c": r0c, "r1c": r1c, "c1sel": c1sel}
    d.update(kw)
    return d


ZERO = U(0, 0, (0, 0, 0), 0, 0)
# (rate, kbit/s, frames of four units in unit order (frame, channel, granule)); "fill": the unit takes what the frame has left, exactly
CALLS = [
    (44100, 128, [
        [U(37, 9, (13, 15, 24), 4, 1, 0, every=2), U(0, 20, (0, 0, 0), 0, 0, 1), ZERO, U(288, 0, (13, 13, 15), 6, 7, 0, every=9)],
        [U(23, 3, (0, 17, 0), 0, 2, 0), U(4, 142, (15, 1, 1), 5, 0, 0), U(61, 0, (15, 15, 23), 2, 3, 1, every=3), U(12, 5, (31, 13, 13), 6, 7, 1)],
        [U(9, 0, (16, 16, 16), 0, 0, 0), U(41, 31, (13, 20, 28), 1, 0, 1, every=4), U(5, 1, (15, 15, 15), 3, 3, 0), ZERO]]),
    (32000, 320, [
        [U(100, 0, (31, 31, 31), 6, 7, 0, all_max=True), U(90, 40, (31, 23, 13), 6, 7, 1), U(288, 0, (24, 15, 13), 6, 7, 0, every=2), U(45, 99, (19, 26, 0), 0, 7, 0)],
        [U(3, 2, (13, 13, 13), 0, 0, 0), ZERO, U(0, 1, (0, 0, 0), 0, 0, 1), U(2, 0, (15, 0, 0), 0, 0, 0)]]),                       # tiny units: the stuffing spills at 4095
    (48000, 64, [
        [U(20, 6, (13, 15, 16), 0, 1, 0, every=2), U(33, 4, (24, 13, 15), 2, 1, 1, every=3), U(15, 30, (15, 13, 13), 5, 5, 0), "fill"],   # no stuffing at all
        [U(8, 140, (13, 0, 0), 6, 7, 1), ZERO, U(1, 0, (13, 13, 13), 0, 0, 0), U(10, 2, (21, 29, 15), 0, 0, 0)],
        [ZERO, ZERO, ZERO, ZERO]]),
]


def frame_capacity(slots, pad):
    mean_bits = (8 * (slots + pad) - 288) // 2
    return 2 * mean_bits + (mean_bits & 1)


def build_call(mlib, T, rate, kbps, frames):
    """-> dict of what the device call and the formatter take.  The formatter derives the padding from the frame number, so
    the frames of the call are the ones around the stream's first unpadded frame (where the rate has one), behind
    all-zero frames."""
    sri = {44100: 0, 48000: 1, 32000: 2}[rate]
    slots = (kbps * 1000 * 1152 // 8) // rate
    n = len(frames)
    _, pad_all = mlib.rate_frames(rate, kbps, 2, 64)
    first = max(int(np.argmin(pad_all)) - 1, 0) if pad_all.min() != pad_all.max() else 0
    total = first + n + 1                                   # one all-zero frame behind: the formatter drops an unfinished last dword
    ix = np.zeros((total * 4, 576), dtype=np.int16)
    gr = np.zeros(total * 4, dtype=mlib.GR_OUT_DTYPE)
    specs = [dict(ZERO) for _ in range(total * 4)]
    for fi, fr in enumerate(frames):
        f = first + fi
        cap, used = frame_capacity(slots, int(pad_all[f])), 0
        for k, s in enumerate(fr):
            u = f * 4 + k
            if s == "fill":
                rem = cap - used
                c00, c10 = int(T["h13"][0]), int(T["h13"][16]) + 1
                assert c00 == 1
                n10 = max(0, -(-(rem - 288) // (c10 - 1)))
                n00 = rem - n10 * c10
                assert n00 >= 0 and n10 + n00 <= 288, (rem, n10, n00)
                s = U(n10 + n00, 0, (13, 13, 13), 3, 2, 0)
                ix[u, 0:2 * n10:2] = 1
                ix[u, 0:2 * n10:4] = -1
            else:
                ix[u] = make_unit(T, sri, s, seed=u + 1)
            specs[u] = dict(s)
            g = gr[u]
            g["big_values"], g["count1"], g["count1table_select"] = s["bv"], s["c1"], s["c1sel"]
            g["table_select"] = s["ts"]
            g["region0_count"], g["region1_count"] = s["r0c"], s["r1c"]
            g["quantizer_step"] = (u * 5) % 40 - 20
            g["part2_3_length"] = unit_bits(T, sri, ix[u], s)
            g["xrmax"] = 1 if (u // 2) % 3 else 0
            assert g["part2_3_length"] <= 4095
            used += int(g["part2_3_length"])
        assert used <= cap, (rate, kbps, fi, used, cap)
    # band energies: equal in both granules of some channels (scfsi 1111 with both xrmax set), far apart in others
    en = np.zeros((total * 4, 22), dtype=np.int32)
    for c in range(total * 2):
        en[2 * c] = np.arange(22) * 3 - c
        en[2 * c + 1] = en[2 * c] + (0 if c % 2 else np.arange(22) % 4)
    scfsi = np.zeros((total, 2, 4), dtype=np.int32)
    for c in range(total * 2):
        d = np.abs(en[2 * c] - en[2 * c + 1])
        cond = 2 + int(gr[2 * c]["xrmax"] != 0) + int(gr[2 * c + 1]["xrmax"] != 0) + int(d[21] < 10) + int(d[:21].sum() < 100)
        for b, (lo, hi) in enumerate(((0, 6), (6, 11), (11, 16), (16, 21))):
            scfsi[c // 2, c % 2, b] = int(cond == 6 and d[lo:hi].sum() < 10)
    pad = pad_all[:total].astype(np.int32)
    off = np.concatenate([[0], np.cumsum(slots + pad)]).astype(np.uint32)
    return {"rate": rate, "kbps": kbps, "sri": sri, "slots": slots, "first": first, "n": n, "ix": ix, "gr": gr, "en": en, "scfsi": scfsi,
            "pad": pad, "off": off, "specs": specs}


def check_coverage(T, calls):
    """every case of the list is in the generated arrays"""
    have = set()
    for c in calls:
        sl = slice(c["first"] * 4, (c["first"] + c["n"]) * 4)
        pads = set(int(p) for p in c["pad"][c["first"]:c["first"] + c["n"]])
        if c["rate"] == 44100 and pads == {0, 1}:
            have.add("padded and unpadded")
        if c["slots"] == 1440:
            have.add("longest frame")
        for f in range(c["first"], c["first"] + c["n"]):
            p23 = [int(c["gr"][f * 4 + k]["part2_3_length"]) for k in range(4)]
            stuffing = frame_capacity(c["slots"], int(c["pad"][f])) - sum(p23)
            assert stuffing >= 0
            have.add("no stuffing" if stuffing == 0 else "stuffing fits unit 0" if p23[0] + stuffing < 4095 else "stuffing spills at 4095")
        for u in range(sl.start, sl.stop):
            g, ix = c["gr"][u], c["ix"][u].astype(int)
            bv, c1 = int(g["big_values"]), int(g["count1"])
            r1s, r2s = _region_starts(T, c["sri"], int(g["region0_count"]), int(g["region1_count"]))
            assert not ix[2 * bv + 4 * c1:].any() and bv + 2 * c1 <= 288
            if bv == 0 and c1 == 0 and not ix.any():
                have.add("all-zero unit")
            if bv == 0 and c1 > 0:
                have.add("big_values 0 with count1")
            if bv == 288:
                have.add("big_values 288")
            if c1 == 0 and bv:
                have.add("count1 0")
            if c1:
                have.add("count1 table %d" % int(g["count1table_select"]))
                if bv & 1:
                    have.add("odd big_values")
                if bv + 2 * c1 == 288:
                    have.add("count1 ends at pair 287")
                for q in range(c1):
                    p = bv + 2 * q
                    if p % 5 == 4 and ix[2 * p:2 * p + 2].any() and ix[2 * p + 2:2 * p + 4].any():
                        have.add("quadruple over two lanes")
            for name, start in (("region 1", r1s // 2), ("region 2", r2s // 2)):
                if 0 < start < bv:
                    have.add("bound inside a lane" if start % 5 else "bound on a lane boundary")
                if start >= bv and bv:
                    have.add("bound beyond big_values")
            if int(g["region0_count"]) == 0 and bv > 2:
                have.add("region0_count 0")
            if int(g["region0_count"]) + int(g["region1_count"]) == 13 and bv > r2s // 2:
                have.add("largest region counts")
            all_max = bv > 0
            for p in range(bv):
                book = int(g["table_select"][(2 * p >= r1s) + (2 * p >= r2s)])
                x, y = int(ix[2 * p]), int(ix[2 * p + 1])
                if book == 0:
                    all_max = False
                    if x or y:
                        have.add("table 0 over pairs with values")
                    continue
                have.add("family %s" % ("13" if book == 13 else "15" if book == 15 else "16-23" if book < 24 else "24-31"))
                have.add("x=%d" % x)
                have.add("y=%d" % y)
                if x and not y:
                    have.add("x=%d beside 0" % x)
                if y and not x:
                    have.add("y=%d beside 0" % y)
                if not (T["lin"][book] == 13 and abs(x) == MAXV and abs(y) == MAXV):
                    all_max = False
            if all_max:
                have.add("maximum in every pair")
    want = {"padded and unpadded", "longest frame", "no stuffing", "stuffing fits unit 0", "stuffing spills at 4095", "all-zero unit",
            "big_values 0 with count1", "big_values 288", "count1 0", "count1 table 0", "count1 table 1", "odd big_values",
            "count1 ends at pair 287", "quadruple over two lanes", "bound inside a lane", "bound on a lane boundary",
            "bound beyond big_values", "region0_count 0", "largest region counts", "table 0 over pairs with values",
            "family 13", "family 15", "family 16-23", "family 24-31", "maximum in every pair"}
    for v in PALETTE:
        want |= {"x=%d" % v, "y=%d" % v}
        if v:
            want |= {"x=%d beside 0" % v, "y=%d beside 0" % v}
    assert not (want - have), sorted(want - have)
    assert sorted(len(c["specs"]) // 4 - c["first"] - 1 for c in calls) == [2, 3, 3]


def expected_bytes(mlib, c):
    """the formatter's bytes of the call's frames"""
    mp3 = mlib.format_stream(c["rate"], c["kbps"], c["ix"].reshape(-1, 4, 576), c["gr"], c["scfsi"])
    lo, hi = int(c["off"][c["first"]]), int(c["off"][c["first"] + c["n"]])
    assert len(mp3) >= hi
    return mp3[lo:hi]


def build_all(mlib):
    T = _tables(mlib)
    calls = [build_call(mlib, T, rate, kbps, frames) for rate, kbps, frames in CALLS]
    check_coverage(T, calls)
    return T, calls


def test_pack_pairs_generator_cpu(mlib):
    """the generator covers its list and the formatter takes every unit: the frames come out at their sizes, with the sync word in front"""
    _, calls = build_all(mlib)
    for c in calls:
        exp = expected_bytes(mlib, c)
        assert len(exp) == int(c["off"][c["first"] + c["n"]] - c["off"][c["first"]])
        for f in range(c["first"], c["first"] + c["n"]):
            o = int(c["off"][f] - c["off"][c["first"]])
            assert exp[o] == 0xff and exp[o + 1] == 0xfb and (exp[o + 2] >> 1) & 1 == int(c["pad"][f])


@pytest.mark.gpu
def test_pack_pairs_device_matches_formatter(ctx, mlib):
    L = mlib.lib()
    _, calls = build_all(mlib)
    n_short = 0
    for c in calls:
        exp = expected_bytes(mlib, c)
        f0, n = c["first"], c["n"]
        ix, gr, en = c["ix"][f0 * 4:(f0 + n) * 4], c["gr"][f0 * 4:(f0 + n) * 4], c["en"][f0 * 4:(f0 + n) * 4]
        off = (c["off"][f0:f0 + n + 1] - c["off"][f0]).astype(np.uint32)
        pad = c["pad"][f0:f0 + n].astype(np.uint8)
        size = int(off[-1])
        d_ix, d_gr, d_en = ctx.to_device(np.ascontiguousarray(ix)), ctx.to_device(np.ascontiguousarray(gr)), ctx.to_device(np.ascontiguousarray(en))
        d_off, d_pad = ctx.to_device(off), ctx.to_device(pad)
        d_mp3, d_sc, d_st = ctx.alloc(size + 16), ctx.alloc(n * 8 * 4), ctx.alloc(4)
        held = [d_ix, d_gr, d_en, d_off, d_pad, d_mp3, d_sc, d_st]

        def run(d_units):
            ctx.upload(d_mp3, np.full(size + 16, 0xa5, dtype=np.uint8))
            mlib.check(L.mp3s_pack_frames_dev(ctx.handle, d_ix, d_units, d_en, n, c["rate"], c["kbps"], d_off, d_pad, d_mp3, d_sc, d_st))
            ctx.sync()
            return int(ctx.download(d_st, np.int32, (1,))[0]), ctx.download(d_mp3, np.uint8, (size + 16,)).tobytes()

        st, out = run(d_gr)
        assert st == 0
        assert out[size:] == b"\xa5" * 16, "bytes behind the last frame were written"
        bad = [i for i in range(size) if out[i] != exp[i]]
        assert not bad, (c["rate"], c["kbps"], "first differing byte", bad[0], "frame", int(np.searchsorted(off, bad[0], side="right")) - 1, len(bad))
        assert np.array_equal(ctx.download(d_sc, np.int32, (n, 2, 4)), c["scfsi"][f0:f0 + n])
        # a book the encoder never selects, over pairs: status 2; and the launch behind it is clean again, with the same bytes
        u_bad = next(u for u in range(n * 4) if gr[u]["big_values"] > 2 and gr[u]["table_select"][0] in (13, 15))
        g_bad = gr.copy()
        g_bad["table_select"][u_bad][0] = 5
        d_bad = ctx.to_device(g_bad)
        held.append(d_bad)
        assert run(d_bad)[0] == 2
        assert run(d_gr) == (0, out)
        # part2_3_length one bit too small (in a unit that is not the frame's first, which takes the stuffing): status bit 0
        u_short = next((u for u in range(n * 4) if u % 4 == 1 and gr[u]["part2_3_length"] > 0 and
                        frame_capacity(c["slots"], int(pad[u // 4])) - int(gr["part2_3_length"][u - 1:u + 3].sum()) + int(gr[u - 1]["part2_3_length"]) + 1 < 4095), None)
        if u_short is not None:                             # (a frame whose stuffing spills fills the short unit up again)
            g_short = gr.copy()
            g_short["part2_3_length"][u_short] -= 1
            d_short = ctx.to_device(g_short)
            held.append(d_short)
            assert run(d_short)[0] & 1
            assert run(d_gr) == (0, out)
            n_short += 1
        for q in held:
            ctx.free(q)
    assert n_short >= 2
