"""The device's chain re-runs, mp3s_chain_redo_dev (k_chain_sum / k_chain_apply, k_rate_redo, the check again: csrc/k_chain.hpp,
csrc/k_rate.hpp), pinned to the reference's serial order: given units the rate loop's own tests pin one by one (test_rate_units.py,
test_reference_rates.py), do the listing, the re-runs, the chain following and the second check leave the records the serial order leaves
-- and when the verdict says "final", is it?  The serial order is chain_model.serial_truth (the oracle hook, unit by unit); the check is
chain_model.walk.  The streams are built from spectra, aimed at the machinery's own edges: the list's capacity, the chain walk's limit,
a walk meeting another entry, the end of a stream inside a batch, a block that starts with a carry, a call without a message.

The case builders assert from the oracle alone that the cases are what they claim (test_conditions_hold_on_the_oracle, no device); the
device tests reuse the same cached cases.  Everything is bit-exact."""
import functools

import numpy as np
import pytest

import chain_model as cm
import test_rate_units as tru
from test_rate_units import ADDR, GI

KBPS = 128
REDO_CAP, REDO_CHAIN_MAX = 4096, 64            # csrc/k_rate.hpp
NO_CURSOR = cm.NO_CURSOR


# ------------------------------------------------------------------------------------------------------------------------ streams
@functools.lru_cache(maxsize=None)
def pools(orc, mlib, rate):
    """(loud, quiet, loud_reading) spectra int32 [n][576], qualified on zero state under every budget the frames of this rate have:
    loud: ends with big_values > 0, leaves non-zero addresses, and the search's first probe (step -60) has big values already, so
    that every later probe finds addresses of the unit's own: it never reads what it inherits and a walk ends in front of it;
    quiet: active, big_values == 0 at the final step and no probe in front set the addresses (they end as given: zero) -- it reads what
    it inherits and passes it on;
    loud_reading: ends like a loud one, but its first probe has no big values: that probe reads the inherited addresses, a walk that
    comes by runs it again and goes on behind it."""
    t = tru.tables(mlib)
    budgets = np.unique(tru.rate_frames(mlib, rate, KBPS, 256)["max_bits"])
    xs, _ = tru.mixed(t, 41, 1024, ("sparse", "ties", "escape_edges"))
    xq, _ = tru.mixed(t, 42, 2048, ("quiet",), steps=(-119, -119, -90, -60))
    loud, quiet = np.ones(len(xs), dtype=bool), np.abs(xq).max(1) > 0
    for mb in budgets:
        z, q = orc.rate_units_from(rate, int(mb), xs), orc.rate_units_from(rate, int(mb), xq)
        loud &= (z["rc"] == 0) & (z["gi"]["big_values"] > 0) & (z["gi"]["address1"] > 0)
        quiet &= (q["rc"] == 0) & (q["gi"]["big_values"] == 0) & (q["gi"]["address3"] == 0)
    bits, bv, _ = orc.probe_bits(rate, -60, xs)
    deaf, reading = loud & (bv > 0), loud & (bv == 0) & (bits >= 0) & (bits < 100000)
    assert deaf.sum() >= 128 and quiet.sum() >= 128 and reading.sum() >= 32, (int(deaf.sum()), int(quiet.sum()), int(reading.sum()))
    return xs[deaf], xq[quiet], xs[reading]


def spectra_of(pattern, pool, rng):
    """one frame per letter -- L: four loud units, Q: four quiet ones, M: four loud ones that read what they inherit, S: silence"""
    kinds = np.repeat(np.frombuffer(pattern.encode(), dtype=np.uint8), 4)
    xr = np.zeros((len(kinds), 576), dtype=np.int32)
    for letter, src in (("L", pool[0]), ("Q", pool[1]), ("M", pool[2])):
        m = kinds == ord(letter)
        xr[m] = src[rng.integers(0, len(src), int(m.sum()))]
    return xr


class Batch:
    """streams in one call: what the device is given, and (lazily, once) what the oracle says to it"""

    def __init__(self, orc, mlib, rate, seed, patterns, hide=None, spans=None, guess=None, chain_in=None):
        """patterns: one string per stream; hide: the batch's message array; spans[s] = (hide_base, hide_begin, hide_end) or None: the
        stream hides nothing; guess: "none" = MP3S_NO_CURSOR everywhere, "3u" = hide_begin + 3 * (unit in the stream); chain_in[s]"""
        self.orc, self.mlib, self.rate, self.patterns = orc, mlib, rate, patterns
        rng = np.random.default_rng(seed)
        pool = pools(orc, mlib, rate)
        self.xr = np.concatenate([spectra_of(p, pool, rng) for p in patterns])
        n = sum(len(p) for p in patterns)
        self.rf = mlib.rate_frames(rate, KBPS, 2, n)[0]
        self.segs = np.zeros(len(patterns), dtype=mlib.CHAIN_SEG_DTYPE)
        self.hide = None if hide is None else np.ascontiguousarray(hide, dtype=np.uint8)
        self.cursor = None if hide is None else np.full(n * 4, NO_CURSOR, dtype=np.int32)
        f0 = 0
        for s, p in enumerate(patterns):
            sp = (0, 0, 0) if spans is None or spans[s] is None else spans[s]
            self.segs[s] = (f0, len(p), sp[0], sp[1], sp[2], 0, np.zeros((4, 4)) if chain_in is None or chain_in[s] is None else chain_in[s])
            self.rf["stream"][f0:f0 + len(p)] = s
            self.rf["hide_end"][f0:f0 + len(p)] = sp[2]
            if guess == "3u" and sp[2] > sp[0]:
                self.cursor[f0 * 4:(f0 + len(p)) * 4] = sp[1] + 3 * np.arange(len(p) * 4)
            f0 += len(p)
        self.units = n * 4
        self.active = np.abs(self.xr).max(1) > 0
        self.counts = {}

    @functools.cached_property
    def truth(self):
        t = cm.serial_truth(self.orc, self.rate, self.rf, self.xr, self.segs, self.hide)
        assert (t["rc"] == 0).all(), "a quantizer step leaves the table in the serial order: another seed"
        return t

    @functools.cached_property
    def first(self):
        r = cm.first_pass(self.orc, self.rate, self.rf, self.xr, self.hide, self.cursor)
        assert (r["rc"] == 0).all(), "a quantizer step leaves the table in the first pass: another seed"
        return r

    @functools.cached_property
    def matters(self):
        """units whose TRUE result is not their first-pass result: each of them the check must list or a walk must reach"""
        return self.active & ~tru.same_result(self.truth, self.first)

    def with_spectra(self, xr):
        """the same batch on other spectra (its oracle results are its own)"""
        other = Batch.__new__(Batch)
        other.__dict__.update({k: v for k, v in self.__dict__.items() if k not in ("truth", "first", "matters")})
        other.xr, other.active = xr, np.abs(xr).max(1) > 0
        return other

    def hides(self, s):
        return int(self.segs["hide_end"][s]) > int(self.segs["hide_base"][s])

    def say(self, u):
        s = int(self.rf["stream"][u >> 2])
        f = (u >> 2) - int(self.segs["first_frame"][s])
        return "unit %d (stream %d frame %d '%s' chain %d)" % (u, s, f, self.patterns[s][f], u & 3)


def rows(r, n_rows):
    return "L" + ("Q" * r + "L") * n_rows


@functools.lru_cache(maxsize=None)
def case_a(orc, mlib, rate):
    """A: one stream, loud / quiet frames in turn, no message: every quiet unit inherits a loud unit's addresses, the loud unit behind
    it ends its walk"""
    b = Batch(orc, mlib, rate, 100 + rate, ["LQ" * 20])
    b.counts = {"units": b.units, "state_matters": int(b.matters.sum())}
    assert b.counts["state_matters"] >= 32, b.counts
    return b


# B, R = 200: a re-run and the re-runs it chains to share REDO_CHAIN_MAX steps, one per unit looked at and one per unit run again, so one
# call settles the first 33 quiet units of a row (k_rate.hpp: `steps`).  The row of 200 alone would keep the verdict where it is from call
# to call (one unit per chain until the row is through); the two rows of 40 behind it are settled by the second call, which is what
# lowers it.
# R = 2: half of the rows end on a loud frame that reads what it inherits -- the walk runs it again and meets the next row's first unit, an entry
ROWS = {1: rows(1, 8), 2: "L" + "QQM" * 4 + "QQL" * 4, 32: rows(32, 4), 200: "L" + "Q" * 200 + "L" + "Q" * 40 + "L" + "Q" * 40 + "L"}


@functools.lru_cache(maxsize=None)
def case_b(orc, mlib, r):
    """B: rows of quiet frames behind a loud one: the first check can fault only a row's first units, the rest is the walk's work"""
    b = Batch(orc, mlib, 44100, 200 + r, [ROWS[r]])
    pat = np.repeat(np.frombuffer(ROWS[r].encode(), dtype=np.uint8), 4)
    quiet = pat == ord("Q")
    head = quiet & (np.concatenate([[0] * 4, pat[:-4]]) != ord("Q"))
    b.counts = {"units": b.units, "quiet_units": int(quiet.sum()), "state_matters": int(b.matters.sum()),
                "row_heads": int(head.sum()), "row_heads_that_matter": int((head & b.matters).sum()),
                "matter_behind_a_head": int((b.matters & quiet & ~head).sum())}
    # every row's first units must be faults (or nothing starts), and for R > 1 most of the work must lie behind them
    assert b.counts["row_heads_that_matter"] == b.counts["row_heads"], b.counts
    assert r == 1 or b.counts["matter_behind_a_head"] >= (b.counts["quiet_units"] - b.counts["row_heads"]) // 2, b.counts
    return b


C_FRAMES = 2100


@functools.lru_cache(maxsize=None)
def case_c(orc, mlib):
    """C: case A made long: more faults than the list holds"""
    b = Batch(orc, mlib, 44100, 300, ["LQ" * (C_FRAMES // 2)])
    b.counts = {"units": b.units, "state_matters": int(b.matters.sum())}
    assert b.counts["state_matters"] >= REDO_CAP + 64, b.counts
    return b


D_LENGTHS = (3, 7, 40)


def listed_for_cursor(b, s):
    """what the first check makes of a hiding stream's first pass, from the oracle: the active units it lists for their cursor, and
    whether the TRUE table counts of those units are their first-pass counts (then the cursors it hands them are the true ones)"""
    u0, u1 = cm.stream_units(b.segs, s)
    adv = b.first["advance"][u0:u1].astype(np.int64)
    cur = int(b.segs["hide_begin"][s]) + np.concatenate([[0], np.cumsum(adv)[:-1]])
    end = int(b.segs["hide_end"][s])
    listed = b.active[u0:u1] & (b.cursor[u0:u1] != cur) & (np.minimum(b.cursor[u0:u1], cur) < end)
    return u0 + np.nonzero(listed)[0], bool((b.truth["advance"][u0:u1][listed] == adv[listed]).all())


@functools.lru_cache(maxsize=None)
def case_d(orc, mlib):
    """D: loud frames, a message of 3, 7 and 40 bits, the first pass with MP3S_NO_CURSOR everywhere: the first units are listed for their
    cursor.  -> ({length: batch}, the lengths whose listed units take as many tables with the message as without)"""
    for seed in range(400, 432):
        msg = np.random.default_rng(seed).integers(0, 2, max(D_LENGTHS)).astype(np.uint8)
        out, exact = {}, []
        for n in D_LENGTHS:
            b = Batch(orc, mlib, 44100, seed, ["L" * 60], hide=msg[:n], spans=[(0, 0, n)], guess="none")
            listed, same = listed_for_cursor(b, 0)
            b.counts = {"seed": seed, "message_bits": n, "listed_for_cursor": len(listed), "table_counts_as_in_the_first_pass": same,
                        "state_matters": int(b.matters.sum())}
            assert len(listed) >= (n + 2) // 3, b.counts
            out[n] = b
            if same:
                exact.append(n)
        if exact:
            return out, tuple(exact)
    raise AssertionError("no seed gives a length whose listed units keep their table counts")


@functools.lru_cache(maxsize=None)
def case_d_silence(orc, mlib):
    """D, second sub-case: cursors guessed as 3 * u, a silence in the middle of a 300-bit message: behind it every guess is wrong, run
    after run of consecutive units of every chain is a list entry, each entry's walk runs into the next entry"""
    msg = np.random.default_rng(450).integers(0, 2, 300).astype(np.uint8)
    b = Batch(orc, mlib, 44100, 450, ["L" * 8 + "S" * 12 + "L" * 20 + "Q" * 4 + "L" * 76], hide=msg, spans=[(0, 0, 300)], guess="3u")
    listed, _ = listed_for_cursor(b, 0)
    per_chain = [int(((listed & 3) == k).sum()) for k in range(4)]
    b.counts = {"units": b.units, "listed_for_cursor": len(listed), "per_chain": per_chain, "state_matters": int(b.matters.sum())}
    assert min(per_chain) >= 16, b.counts
    return b


@functools.lru_cache(maxsize=None)
def case_e(orc, mlib):
    """E: three streams in one call: A's (it ends on a quiet frame: its last walks end with the stream, not with the batch); a short one
    that starts with quiet frames on a carry (chain_in: addresses a chain can hold, as test_rate_units.donor_state takes them); a hiding
    one with its own hide_base"""
    loud = pools(orc, mlib, 44100)[0]
    z = orc.rate_units_from(44100, int(tru.rate_frames(mlib, 44100, KBPS, 8)["max_bits"][0]), loud[:4])
    carry = np.array([[z["gi"][f][k] for f in ADDR] + [-40 - k] for k in range(4)], dtype=np.int32)
    assert (carry[:, :3] > 0).all()
    base = 11
    for seed in range(500, 532):
        rng = np.random.default_rng(seed)
        hide = rng.integers(0, 2, base + 7).astype(np.uint8)      # (the bytes in front of hide_base are another stream's)
        b = Batch(orc, mlib, 44100, seed, ["LQ" * 20, "QQQQLQQL", "L" * 30], hide=hide, spans=[None, None, (base, base, base + 7)],
                  guess="none", chain_in=[None, carry, None])
        listed, same = listed_for_cursor(b, 2)
        if not same:
            continue
        u0, u1 = cm.stream_units(b.segs, 1)
        b.counts = {"seed": seed, "units": b.units, "state_matters": int(b.matters.sum()), "listed_for_cursor": len(listed),
                    "matter_on_the_carry": int(b.matters[u0:u0 + 16].sum())}
        assert b.counts["state_matters"] >= 32 and b.counts["matter_on_the_carry"] >= 8 and len(listed) >= 3, b.counts
        return b
    raise AssertionError("no seed keeps the table counts of the hiding stream's listed units")


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_serial_truth_is_the_encoder(orc, mlib, golden_dir):
    """serial_truth on the encoder's own spectra: every GrInfo field (part2_3_length with the frame's stuffing), ix and the end cursor
    are orc.encode's, which the goldens pin -- for a stream with a message and one with silence inside"""
    for name, pcm, rate, kbps, hide in tru.chained_streams(golden_dir):
        o = orc.encode(pcm, rate, kbps, hide)
        assert o["rc"] == 0
        n = o["n_frames"]
        rf, pad = mlib.rate_frames(rate, kbps, 2, n)
        rf["hide_end"] = len(hide)
        segs = np.zeros(1, dtype=mlib.CHAIN_SEG_DTYPE)
        segs["n_frames"], segs["hide_end"] = n, len(hide)
        xr = np.ascontiguousarray(o["mdct_freq"].reshape(n * 4, 576))            # [f][ch][gr]: the unit order
        t = cm.serial_truth(orc, rate, rf, xr, segs, hide)
        assert (t["rc"] == 0).all()
        whole = int((2 * 576 / rate) * (1000 * kbps / 8))
        active = np.abs(xr).max(1) > 0
        assert np.array_equal(t["ix"][active], np.abs(o["ix"].reshape(n * 4, 576))[active]), name
        gi = t["gi"].reshape(n, 2, 2).transpose(0, 2, 1).copy()                  # [f][gr][ch] as the encoder's frames keep them
        for f in range(n):
            gi["part2_3_length"][f] = tru.resv_frame_end(gi["part2_3_length"][f], int((8 * (whole + int(pad[f])) - 8 * 36) / 2))
        for k in orc.GRINFO_DTYPE.names:
            assert np.array_equal(gi[k], o["frames"]["gi"][k]), (name, k)
        assert np.array_equal(t["cursor"][4::4], o["frames"]["hide_off"][:-1]), name
        assert t["end_cursor"] == [o["hide_offset"]], name
        inherits = int((active & t["state"][:, :3].any(1)).sum())
        print("serial_truth", name, "frames", n, "end cursor", t["end_cursor"][0], "active units that inherit addresses", inherits)


def test_walk_of_the_truth_finds_nothing(orc, mlib):
    """walk() and serial_truth() agree where they overlap: records written from the TRUE results, given what they were given, have no
    fault for the walk, and its cursors, chains and ends are the truth's -- so a verdict of the walk means what the tests take it for"""
    b = case_e(orc, mlib)
    t = b.truth
    rec = np.zeros(b.units, dtype=mlib.GR_OUT_DTYPE)
    for a, f in GI:
        rec[a] = t["gi"][f]
    rec["address"] = np.stack([t["gi"][f] for f in ADDR], axis=1)
    rec["n_tables"], rec["reserved0"] = t["advance"], cm.pack3(t["state"])
    rec["flags"] = np.where(b.active, cm.RF_ACTIVE | cm.RF_USED_ADDR_IN, 0)      # (as if every unit had read what it was given)
    for s, w in enumerate(cm.walk(rec, b.rf, b.segs, np.minimum(t["cursor"], NO_CURSOR))):
        u0, u1 = w["first"], w["stop"]
        assert len(w["faulted"]) == 0 and w["end_cursor"] == t["end_cursor"][s] and np.array_equal(w["end_chain"], t["end_chain"][s])
        assert np.array_equal(w["cursor"], t["cursor"][u0:u1]) and np.array_equal(w["chain"], t["state"][u0:u1])
        assert np.array_equal(w["records"], rec[u0:u1])
    # ... and the first pass's records do have faults: at least one per run of units whose state matters
    rec["reserved0"] = 0
    for a, f in GI:
        rec[a] = b.first["gi"][f]
    rec["address"] = np.stack([b.first["gi"][f] for f in ADDR], axis=1)
    rec["n_tables"] = b.first["advance"]
    assert sum(len(w["faulted"]) for w in cm.walk(rec, b.rf, b.segs, b.cursor)) >= 16


def test_conditions_hold_on_the_oracle(orc, mlib):
    """what makes the device tests below mean something, from the oracle's results alone (the builders assert; the counts are printed).
    MP3S_RF_USED_ADDR_IN exists only on the device; it must be set on every unit whose state matters (test_inherited_addresses pins
    that), so "state_matters" is a lower bound on what the check lists and the walks reach."""
    d, exact = case_d(orc, mlib)
    assert exact, "no message length whose listed units keep their table counts"
    cases = {"A": {r: case_a(orc, mlib, r).counts for r in (44100, 48000)}, "B": {r: case_b(orc, mlib, r).counts for r in ROWS},
             "C": case_c(orc, mlib).counts, "D": {n: d[n].counts for n in D_LENGTHS}, "D exact lengths": exact,
             "D silence": case_d_silence(orc, mlib).counts, "E": case_e(orc, mlib).counts}
    print("chain-redo conditions", cases)                           # (pytest -s shows them)


# ------------------------------------------------------------------------------------------------------------------------ device
class Snapshot:
    def __init__(self, gr, ix, en, cursor, verdict=None, seg_out=None):
        self.gr, self.ix, self.en, self.cursor, self.verdict, self.seg_out = gr, ix, en, cursor, verdict, seg_out


class Dev:
    """the device buffers of a batch: first_pass() = mp3s_rate_loop_dev without d_state_in on the batch's cursor guesses, redo() =
    mp3s_chain_redo_dev on what is there; both bring everything down"""

    def __init__(self, ctx, mlib, b, xr=None):
        self.ctx, self.mlib, self.b, self.L = ctx, mlib, b, mlib.lib()
        u = b.units
        self.sizes = {"ix": u * 576 * 2, "out": u * 72, "en": u * 88, "ix2": u * 576 * 2, "out2": u * 72, "en2": u * 88, "ver": 16,
                      "so": len(b.segs) * 80, "state": u * 16, "cur2": u * 4}
        self.d = {k: ctx.alloc(v) for k, v in self.sizes.items()}
        self.d.update(mdct=ctx.to_device(b.xr if xr is None else xr), rf=ctx.to_device(b.rf), segs=ctx.to_device(b.segs),
                      hide=None if b.hide is None else ctx.to_device(b.hide), cur=None if b.hide is None else ctx.to_device(b.cursor))
        self.n_hide = 0 if b.hide is None else len(b.hide)

    def close(self):
        for p in self.d.values():
            if p is not None:
                self.ctx.free(p)

    def set_spectra(self, xr):
        self.ctx.upload(self.d["mdct"], np.ascontiguousarray(xr))

    def down(self, verdict=False, which=("out", "ix", "en")):
        c, d, u = self.ctx, self.d, self.b.units
        return Snapshot(c.download(d[which[0]], self.mlib.GR_OUT_DTYPE, (u,)), c.download(d[which[1]], np.int16, (u, 576)),
                        c.download(d[which[2]], np.int32, (u, 22)), None if d["cur"] is None else c.download(d["cur"], np.int32, (u,)),
                        c.download(d["ver"], np.int32, (2,)) if verdict else None,
                        c.download(d["so"], self.mlib.CHAIN_SEG_OUT_DTYPE, (len(self.b.segs),)) if verdict else None)

    def first_pass(self):
        d = self.d
        if d["cur"] is not None:
            self.ctx.upload(d["cur"], self.b.cursor)
        self.mlib.check(self.L.mp3s_rate_loop_dev(self.ctx.handle, d["mdct"], d["rf"], len(self.b.rf), d["hide"], self.n_hide, d["cur"], None,
                                                  None, 0, d["ix"], d["out"], d["en"]))
        self.ctx.sync()
        return self.down()

    def redo(self):
        d = self.d
        self.mlib.check(self.L.mp3s_chain_redo_dev(self.ctx.handle, d["mdct"], d["rf"], len(self.b.rf), d["hide"], self.n_hide, d["cur"],
                                                   d["segs"], len(self.b.segs), d["ix"], d["out"], d["en"], d["ver"], d["so"]))
        self.ctx.sync()
        return self.down(verdict=True)

    def rerun_on(self, state, cursor):
        """one mp3s_rate_loop_dev launch over all units on the given d_state_in / d_cursor_in, into buffers of its own"""
        d = self.d
        self.ctx.upload(d["state"], np.ascontiguousarray(state, dtype=np.int32))
        if cursor is not None:
            self.ctx.upload(d["cur2"], np.ascontiguousarray(cursor, dtype=np.int32))
        self.mlib.check(self.L.mp3s_rate_loop_dev(self.ctx.handle, d["mdct"], d["rf"], len(self.b.rf), d["hide"], self.n_hide,
                                                  None if cursor is None else d["cur2"], d["state"], None, 0, d["ix2"], d["out2"], d["en2"]))
        self.ctx.sync()
        return self.down(which=("out2", "ix2", "en2"))


def first_bad(b, bad, what, got=None, want=None):
    u = int(np.nonzero(bad)[0][0])
    more = "" if got is None else ": device %s expected %s" % (np.asarray(got)[u].tolist(), np.asarray(want)[u].tolist())
    return "%s: %d units, first %s%s" % (what, int(np.asarray(bad).sum()), b.say(u), more)


def against_oracle(b, xr, snap, want, what, cursors_too):
    """records and ix of a snapshot against oracle results `want` (rate_units_from's or serial_truth's), in the fields of
    test_rate_units.GI and ADDR, n_tables, |ix| and the signs of ix against the spectrum"""
    ok, active = want["rc"] == 0, np.abs(xr).max(1) > 0
    ix = snap.ix.astype(np.int32)

    def same(name, a, c, where):
        bad = where & ~(np.asarray(a) == np.asarray(c)).reshape(len(xr), -1).all(1)
        assert not bad.any(), first_bad(b, bad, "%s: %s" % (what, name), a, c)
    everyone = np.ones(len(xr), dtype=bool)
    same("MP3S_RF_STEP_RANGE against rc", (snap.gr["flags"] & cm.RF_STEP_RANGE) != 0, ~ok, everyone)
    same("MP3S_RF_ACTIVE", (snap.gr["flags"] & cm.RF_ACTIVE) != 0, active, everyone)
    for a, f in GI:
        same(a, snap.gr[a], want["gi"][f], ok)
    for k, f in enumerate(ADDR):
        same(f, snap.gr["address"][:, k], want["gi"][f], ok)
    same("n_tables", snap.gr["n_tables"], want["advance"], ok)
    same("abs(ix)", np.abs(ix), want["ix"], ok & active)
    same("ix of a silent unit", ix, np.zeros_like(ix), ~active)
    same("signs of ix", (ix == 0) | ((ix < 0) == (xr < 0)), np.ones(ix.shape, dtype=bool), ok)
    if cursors_too:                          # the units that hide: the live part of a hiding stream
        end = np.repeat(b.rf["hide_end"], 4).astype(np.int64)
        hiding = np.repeat(np.array([b.hides(s) for s in b.rf["stream"]]), 4)
        live = hiding & active & (np.minimum(want["cursor"], snap.cursor) < end)
        same("cursor", snap.cursor, want["cursor"], live)


def reachable(b, before, faulted):
    """the active units a call may write: the faulted ones and what a walk from one of them can reach -- the units behind it on its
    chain, in its stream, up to the first active unit that did not read what it inherited (the walk of k_rate.hpp ends in front of it).
    Silent units are the check's to write and are judged through walk()."""
    may = np.zeros(b.units, dtype=bool)
    flags = before.gr["flags"]
    for s in range(len(b.segs)):
        u0, u1 = cm.stream_units(b.segs, s)
        for k in range(4):
            on = False
            for u in range(u0 + k, u1, 4):
                if faulted[u]:
                    on = True
                elif flags[u] & cm.RF_ACTIVE:
                    on = on and bool(flags[u] & cm.RF_USED_ADDR_IN)
                may[u] = on and bool(flags[u] & cm.RF_ACTIVE)
    return may


def faults_of(b, snap):
    w = cm.walk(snap.gr, b.rf, b.segs, snap.cursor)
    f = np.zeros(b.units, dtype=bool)
    for x in w:
        f[x["faulted"]] = True
    return w, f


def check_call(dev, b, xr, before, after, label):
    """Invariants 1, 3 and 4 of a call of mp3s_chain_redo_dev, `before` and `after` being the buffers around it.  -> figures.
    The band energies have one comparator only: a mp3s_rate_loop_dev launch over all units, handed as d_state_in / d_cursor_in the inputs
    the final records name; that launch is pinned to the reference elsewhere (test_rate_units.py compare(): "en against calc_scfsi")."""
    mlib = dev.mlib
    # 4. no internal mark leaves the call
    bad = (after.gr["flags"] & cm.RF_LISTED) != 0
    assert not bad.any(), first_bad(b, bad, label + ": MP3S_RF_LISTED in a record the caller reads")
    bad = (after.gr["flags"] & ~cm.RF_ALL) != 0
    assert not bad.any(), first_bad(b, bad, label + ": a flag bit outside MP3S_RF_*")
    # 1. the verdict is the walk's
    w, faulted_after = faults_of(b, after)
    assert int(after.verdict[0]) == int(faulted_after.sum()), "%s: verdict %s, the walk of the final records faults %d units" % (
        label, after.verdict.tolist(), int(faulted_after.sum()))
    assert int(after.verdict[1]) == int(any(x["step_range"] for x in w)), (label, after.verdict.tolist())
    silent_ok = np.concatenate([x["records"] for x in w]) == after.gr
    assert silent_ok.all(), first_bad(b, ~silent_ok, label + ": a silent unit does not carry what it inherits")
    for s, x in enumerate(w):
        so = after.seg_out[s]
        assert int(so["cursor"]) == x["end_cursor"] and np.array_equal(so["chain"], x["end_chain"]) and \
            bool(so["carry_used"]) == x["carry_used"], "%s: seg_out of stream %d: %s, the walk: %s" % (
                label, s, so.tolist(), (x["end_cursor"], x["end_chain"].tolist(), x["carry_used"]))
    # 3. no torn record: every unit is the oracle's answer to the inputs its record names
    active = (after.gr["flags"] & cm.RF_ACTIVE) != 0
    state = np.concatenate([cm.unpack3(after.gr["reserved0"]), np.zeros((b.units, 1), dtype=np.int32)], axis=1)
    state[~active, :3], state[~active, 3] = after.gr["address"][~active], after.gr["quantizer_step"][~active]
    frame = np.arange(b.units) // 4
    named = b.orc.rate_units_from(b.rate, b.rf["max_bits"][frame], xr, state, b.hide, after.cursor, b.rf["hide_end"][frame])
    against_oracle(b, xr, after, named, label + ": record against the oracle on the inputs it names", False)
    again = dev.rerun_on(state, after.cursor)
    bad = ~(again.en == after.en).all(1)
    assert not bad.any(), first_bad(b, bad, label + ": band energies against a launch on the inputs the records name", again.en, after.en)
    bad = active & ((again.gr != after.gr) | ~(again.ix == after.ix).all(1))
    assert not bad.any(), first_bad(b, bad, label + ": record or ix against a launch on the inputs the records name")
    # ... and what the call had no reason to touch is as it was
    _, faulted_before = faults_of(b, before)
    may = reachable(b, before, faulted_before)
    still = active & ~may
    bad = still & ((after.gr != before.gr) | ~(after.ix == before.ix).all(1) | ~(after.en == before.en).all(1))
    assert not bad.any(), first_bad(b, bad, label + ": written although neither faulted nor within reach of a walk")
    if after.cursor is not None:
        bad = ~faulted_before & (after.cursor != before.cursor)
        assert not bad.any(), first_bad(b, bad, label + ": cursor of a unit the check did not list", after.cursor, before.cursor)
    reached = active & ~faulted_before & (after.gr != before.gr)
    fig = {"faulted_before": int(faulted_before.sum()), "listed": min(int(faulted_before.sum()), REDO_CAP),
           "verdict": after.verdict.tolist(), "reached_by_a_walk": int(reached.sum())}
    print("chain redo", label, fig)
    return fig


def check_final(b, xr, after, truth, label):
    """Invariant 2: a verdict of [0, 0] means the serial order's records, cursors and ends"""
    assert after.verdict.tolist() == [0, 0], (label, after.verdict.tolist())
    against_oracle(b, xr, after, truth, label + ": final against the serial order", after.cursor is not None)
    for s in range(len(b.segs)):
        so = after.seg_out[s]
        assert int(so["cursor"]) == truth["end_cursor"][s], (label, s, int(so["cursor"]), truth["end_cursor"][s])
        assert np.array_equal(so["chain"], truth["end_chain"][s]), (label, s, so["chain"].tolist(), truth["end_chain"][s].tolist())


def run_calls(ctx, mlib, b, label, calls=1, must_be_final=True):
    """first pass, then `calls` calls of mp3s_chain_redo_dev, the invariants after each; "verdict 0 => TRUE" always, and the verdict
    required to be 0 after the last call if must_be_final.  -> the figures of each call"""
    dev = Dev(ctx, mlib, b)
    try:
        before, figs = dev.first_pass(), []
        for i in range(calls):
            after = dev.redo()
            figs.append(check_call(dev, b, b.xr, before, after, "%s call %d" % (label, i + 1)))
            before = after
        if must_be_final or after.verdict.tolist() == [0, 0]:
            check_final(b, b.xr, after, b.truth, label)
        return figs
    finally:
        dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rate", (44100, 48000))
def test_independent_faults_without_a_message(ctx, mlib, orc, rate):
    """A: n_hide == 0, d_cursor NULL.  Every quiet unit is a fault of its own; one call, verdict [0, 0], the serial order's records"""
    b = case_a(orc, mlib, rate)
    fig = run_calls(ctx, mlib, b, "A %d" % rate)[0]
    assert fig["faulted_before"] >= b.counts["state_matters"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("r", (1, 2, 32))
def test_rows_of_inheriting_units(ctx, mlib, orc, r):
    """B, rows no longer than a walk reaches: only a row's first units are listed, the walks do the rest; one call, verdict 0, TRUE"""
    b = case_b(orc, mlib, r)
    fig = run_calls(ctx, mlib, b, "B R=%d" % r)[0]
    assert fig["faulted_before"] >= b.counts["row_heads"]
    assert fig["faulted_before"] + fig["reached_by_a_walk"] >= b.counts["state_matters"]


@pytest.mark.gpu
def test_a_row_longer_than_a_walk(ctx, mlib, orc):
    """B, R = 200 (and two rows of 40 behind it): a walk ends after REDO_CHAIN_MAX steps, so the verdict after one call is > 0 -- and it
    is the walk's count of the records that came down (check_call); a second call on the same buffers goes on from there (k_chain_apply
    reads what every re-run recorded as given) and lowers it; calls until it is 0 end in the serial order's records."""
    b = case_b(orc, mlib, 200)
    dev = Dev(ctx, mlib, b)
    try:
        before, verdicts = dev.first_pass(), []
        for i in range(8):              # 200 quiet units of a chain, 33 per call
            after = dev.redo()
            check_call(dev, b, b.xr, before, after, "B R=200 call %d" % (i + 1))
            verdicts.append(int(after.verdict[0]))
            before = after
            if verdicts[-1] == 0:
                break
        print("chain redo B R=200 verdicts", verdicts)
        assert verdicts[0] > 0 and verdicts[1] < verdicts[0], verdicts
        assert verdicts[-1] == 0 and all(a >= c for a, c in zip(verdicts, verdicts[1:])), verdicts
        check_final(b, b.xr, after, b.truth, "B R=200")
    finally:
        dev.close()


def thin_out(b, dev, want_faults):
    """case C's stream with the spectra of surplus faulted units zeroed until the first check faults exactly `want_faults`: chosen on
    the first pass's own records (a silent unit passes its chain on: the unit behind it must not be one that reads it), confirmed by a
    first pass on the result.  -> (xr, the first pass's snapshot)"""
    first = dev.first_pass()
    _, faulted = faults_of(b, first)
    flags = first.gr["flags"]
    behind = np.concatenate([flags[4:], np.zeros(4, dtype=flags.dtype)])
    quiet = (np.arange(b.units) // 4) % 2 == 1                      # (the stream is "LQLQ ...")
    safe = faulted & quiet & ((behind & cm.RF_USED_ADDR_IN) == 0)
    surplus = int(faulted.sum()) - want_faults
    assert 0 <= surplus <= int(safe.sum()), (int(faulted.sum()), int(safe.sum()), want_faults)
    xr = b.xr.copy()
    # (taken evenly over the stream, so that what is left still spreads over all of it)
    pick = np.nonzero(safe)[0][np.linspace(0, int(safe.sum()) - 1, surplus).round().astype(np.int64)] if surplus else np.zeros(0, dtype=np.int64)
    assert len(set(pick.tolist())) == surplus
    xr[pick] = 0
    dev.set_spectra(xr)
    first = dev.first_pass()
    _, faulted = faults_of(b, first)
    assert int(faulted.sum()) == want_faults, "the first check would fault %d units, %d were aimed at" % (int(faulted.sum()), want_faults)
    return xr, first


@pytest.mark.gpu
@pytest.mark.parametrize("over", (-1, 0, 1, 40))
def test_list_capacity(ctx, mlib, orc, over):
    """C: exactly REDO_CAP + over faults.  Up to the capacity: one call, verdict 0, TRUE.  Above it the entries beyond the capacity are
    counted, not kept: the verdict after one call is exactly their number (which units they are is the order of an atomic), a second
    call gives 0 and the serial order's records."""
    b = case_c(orc, mlib)
    dev = Dev(ctx, mlib, b)
    try:
        xr, before = thin_out(b, dev, REDO_CAP + over)
        thin = b.with_spectra(xr)
        truth = thin.truth
        after = dev.redo()
        fig = check_call(dev, thin, xr, before, after, "C K=CAP%+d call 1" % over)
        assert fig["faulted_before"] == REDO_CAP + over
        assert after.verdict.tolist() == [max(over, 0), 0], after.verdict.tolist()
        if over > 0:
            before, after = after, dev.redo()
            check_call(dev, thin, xr, before, after, "C K=CAP%+d call 2" % over)
        check_final(thin, xr, after, truth, "C K=CAP%+d" % over)
    finally:
        dev.close()


@pytest.mark.gpu
def test_message_cursors(ctx, mlib, orc):
    """D: the first pass ran with MP3S_NO_CURSOR everywhere, the stream's first units are listed for their cursor.  Where the listed units
    take as many tables with the message as without (chosen on the oracle), the cursors the check hands out are the true ones: one call,
    verdict 0, TRUE.  For the other lengths: the invariants, and verdict 0 => TRUE."""
    cases, exact = case_d(orc, mlib)
    for n in D_LENGTHS:
        fig = run_calls(ctx, mlib, cases[n], "D %d bits" % n, must_be_final=n in exact)[0]
        assert fig["faulted_before"] >= cases[n].counts["listed_for_cursor"]


@pytest.mark.gpu
def test_entries_in_a_row(ctx, mlib, orc):
    """D, second sub-case: behind a silence inside a 300-bit message every guessed cursor (3 * u) is wrong: consecutive units of every
    chain are list entries, each entry's walk meets the next entry at once and must leave it to its own wave (MP3S_RF_LISTED: one
    writer per unit) -- a second writer shows as a record that is not the oracle's answer to the inputs it names"""
    b = case_d_silence(orc, mlib)
    fig = run_calls(ctx, mlib, b, "D silence", must_be_final=False)[0]
    assert fig["faulted_before"] >= b.counts["listed_for_cursor"]


@pytest.mark.gpu
def test_a_batch_of_three_streams(ctx, mlib, orc):
    """E: A's stream (its last walk ends with the stream, the next stream's units are not its chain), a block that starts with quiet
    frames on a carry (listed against chain_in), a hiding stream with its own hide_base: one call, verdict 0, TRUE and seg_out per
    stream"""
    b = case_e(orc, mlib)
    fig = run_calls(ctx, mlib, b, "E")[0]
    assert fig["faulted_before"] >= b.counts["matter_on_the_carry"] + b.counts["listed_for_cursor"]
