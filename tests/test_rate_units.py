"""The rate loop unit by unit, as units in the MIDDLE of a stream see it: inherited address1/2/3 and quantizerStepSize, the message cursor
inside, at and behind the end of a message, the variant entries of the selection, budgets set by hand, unit lists -- csrc/k_rate.hpp through
mp3s_rate_loop_dev / mp3s_rate_variants_dev against the reference's own loop (iterate_unit of oracle/orc_encoder.c: MP3_Encoder.py:766-813)
on a GrInfo preset with the same state (oracle_lib.rate_units_from).  On top: the CPU tests that tie that hook to the encoder the goldens pin.

The conditions that keep the data honest (enough units whose result really depends on the state, on the message's end, on a tie ...) are
computed from the oracle's results alone, in the case builders below; test_conditions_hold_on_the_oracle runs them without a device, the device
tests reuse the same (cached) cases."""
import functools
import os

import numpy as np
import pytest

import spectra

RATES = (44100, 48000, 32000)
FRAMES, UNITS = 256, 1024                     # one launch
NO_CURSOR = 0x3fffffff                        # MP3S_NO_CURSOR
BUDGETS = (1, 2, 9, 37, 300, 764, 2000, 4095)  # 764: 44.1 kHz / 128 kbit/s, the benchmark's stream
GI = (("quantizer_step", "quantizerStepSize"), ("big_values", "big_values"), ("count1", "count1"), ("part2_3_length", "part2_3_length"),
      ("region0_count", "region0_count"), ("region1_count", "region1_count"), ("count1table_select", "count1table_select"),
      ("table_select", "table_select"))
ADDR = ("address1", "address2", "address3")


def bits_of(s):
    return np.frombuffer("".join(format(b, "08b") for b in s.encode()).encode(), dtype=np.uint8) - ord("0")


# ------------------------------------------------------------------------------------------------------------------------ data
def base_at(t, step):
    """|xr| that quantises to 1 at `step`: the device's own threshold rl_t1 (tests/test_tables.py pins it against the quantiser), as the
    rate loop's other tests aim.  It is 2 ** (30 + step / 4) but for the rounding of the quantiser's integer scale, and it is a whole number:
    at the lowest steps (1.19 at -119, where the scale is exact) the power itself is returned, the rounded one being up to 70 % off."""
    exact, t1 = 2.0 ** (30 + step / 4.0), float(t["rl_t1"][step + 127])
    assert abs(t1 - exact) <= exact * 2e-3 + 1, step
    return t1 if t1 >= 4096 else exact


def mixed(t, seed, n, families, steps=(-60, -30, -90, -119)):
    """n spectra: the families in equal parts, each aimed at `steps` in turn, shuffled.  -> (xr int32 [n][576], labels [n] "family@step")"""
    rng = np.random.default_rng(seed)
    xs, labels = [], []
    per = -(-n // (len(families) * len(steps)))
    for fi, fam in enumerate(families):
        for si, st in enumerate(steps):
            s = seed * 131 + fi * 17 + si
            b = base_at(t, st)
            xs.append(spectra.sparse_spectra(s, per, base=max(int(np.ceil(b)), 1)) if fam == "sparse" else getattr(spectra, fam)(s, per, base=b))
            labels += ["%s@%d" % (fam, st)] * per
    order = rng.permutation(len(labels))[:n]
    return np.ascontiguousarray(np.concatenate(xs)[order]), np.array(labels)[order]


def pack_state(state):
    return state[:, 0] | (state[:, 1] << 10) | (state[:, 2] << 20)


def donor_state(rng, gi0, rc0, zero_share=0.25):
    """[n][4]: address1..3 = the final triple the oracle leaves for ANOTHER spectrum of the launch (so only triples a chain can hold), zeros
    for `zero_share` of the units; the inherited step random in -120..0 (an active unit overwrites it, a silent one passes it on)"""
    n = len(gi0)
    ok = np.nonzero(rc0 == 0)[0]
    donor = ok[rng.integers(0, len(ok), n)]
    st = np.zeros((n, 4), dtype=np.int32)
    for k, f in enumerate(ADDR):
        st[:, k] = gi0[f][donor]
    st[rng.random(n) < zero_share, :3] = 0
    st[:, 3] = rng.integers(-120, 1, n)
    return st


def same_result(a, b):
    """per unit: two oracle results agree in everything the device reports"""
    eq = (a["ix"] == b["ix"]).all(1) & (a["advance"] == b["advance"]) & (a["rc"] == b["rc"])
    for _, f in GI:
        eq &= (a["gi"][f] == b["gi"][f]).reshape(len(eq), -1).all(1)
    for f in ADDR:
        eq &= a["gi"][f] == b["gi"][f]
    return eq


class Case:
    """the inputs of one launch and what the oracle says to them"""

    def __init__(self, orc, rate, rf, xr, labels, state=None, hide=None, cursor=None, units=None):
        self.rate, self.rf, self.xr, self.labels, self.state, self.hide, self.cursor = rate, rf, xr, labels, state, hide, cursor
        frame = (np.arange(len(xr)) if units is None else units) // 4     # `units`: row i is a run of unit units[i] (variant entries)
        self.max_bits, self.hide_end = rf["max_bits"][frame], rf["hide_end"][frame]
        self.want = orc.rate_units_from(rate, self.max_bits, xr, state, hide, cursor, self.hide_end)
        self.ok = self.want["rc"] == 0

    def say(self, u):
        return "unit %d (%s) max_bits %d state %s cursor %s hide_end %d" % (
            u, self.labels[u], self.max_bits[u], None if self.state is None else self.state[u].tolist(),
            None if self.cursor is None or self.hide is None else int(self.cursor[u]), self.hide_end[u])


def tables(mlib):
    return mlib.debug_tables()


@functools.lru_cache(maxsize=None)
def rate_frames(mlib, rate, kbps=128, n=FRAMES):
    return mlib.rate_frames(rate, kbps, 2, n)[0]


@functools.lru_cache(maxsize=None)
def inherited_cases(orc, mlib, rate):
    """test_inherited_addresses: quiet spectra mixed with sparse_spectra, donor state; without and with a 3-bit message at cursor 0"""
    rng = np.random.default_rng(rate + 1)
    xr, labels = mixed(tables(mlib), rate + 1, UNITS, ("quiet", "quiet", "sparse"))
    rf = rate_frames(mlib, rate).copy()
    zero = Case(orc, rate, rf, xr, labels)
    state = donor_state(rng, zero.want["gi"], zero.want["rc"])
    plain = Case(orc, rate, rf, xr, labels, state)
    hide = np.array([1, 0, 1], dtype=np.uint8)
    rfh = rf.copy()
    rfh["hide_end"] = len(hide)
    cur = np.zeros(UNITS, dtype=np.int32)
    zero_h = Case(orc, rate, rfh, xr, labels, None, hide, cur)
    hidden = Case(orc, rate, rfh, xr, labels, state, hide, cur)
    out = []
    for c, z in ((plain, zero), (hidden, zero_h)):
        assert (~c.ok).sum() <= UNITS // 10, (~c.ok).sum()
        act = (np.abs(xr).max(1) > 0) & c.ok & z.ok
        c.depends = act & ~same_result(c.want, z.want)                      # units whose result changes with the state they are given
        deep = c.depends & ((c.want["gi"]["quantizerStepSize"] != z.want["gi"]["quantizerStepSize"]) |
                            (c.want["gi"]["part2_3_length"] != z.want["gi"]["part2_3_length"]))
        c.counts = {"step_range": int((~c.ok).sum()), "state_matters": int(c.depends.sum()), "step_or_bits_change": int(deep.sum())}
        assert c.counts["state_matters"] >= 64 and c.counts["step_or_bits_change"] >= 32, c.counts
        out.append(c)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cursor_cases(orc, mlib, rate):
    """test_cursor_positions: one 40-bit message; cursors inside it, at its last bits, at and behind its end; zero and donor state mixed.
    The second launch ends the message of half the frames early through hide_end."""
    rng = np.random.default_rng(rate + 2)
    xr, labels = mixed(tables(mlib), rate + 2, UNITS, ("sparse", "quiet", "ties", "escape_edges"))
    rf = rate_frames(mlib, rate).copy()
    hide = rng.integers(0, 2, 40).astype(np.uint8)
    zero = Case(orc, rate, rf, xr, labels)
    state = donor_state(rng, zero.want["gi"], zero.want["rc"], zero_share=0.5)
    state[rng.random(UNITS) < 0.5] = 0
    cur = rng.choice(np.array(list(range(38)) + [38] * 12 + [39] * 12 + [40] * 6 + [41] * 6 + [NO_CURSOR] * 6), UNITS).astype(np.int32)
    first = Case(orc, rate, rf, xr, labels, state, hide, cur)
    rf2 = rf.copy()
    ends = np.array([1, 2, 3, 20])[np.arange(FRAMES // 2) % 4]
    rf2["hide_end"][1::2] = ends
    cur2 = cur.copy()
    cut_units = (np.arange(UNITS) // 4) % 2 == 1
    cur2[cut_units] = np.maximum(np.repeat(rf2["hide_end"], 4)[cut_units] - rng.integers(0, 4, int(cut_units.sum())), 0)
    second = Case(orc, rate, rf2, xr, labels, state, hide, cur2)
    nomsg = Case(orc, rate, rf, xr, labels, state)
    counts = {}
    for name, c in (("first", first), ("second", second)):
        assert (~c.ok).sum() <= UNITS // 10, (~c.ok).sum()
        adv, left = c.want["advance"], np.minimum(c.hide_end, len(hide)).astype(np.int64) - c.cursor
        took = c.ok & (adv > 0)
        by_end = c.hide_end < len(hide)
        counts[name] = {"step_range": int((~c.ok).sum()), "two_left": int((took & ~by_end & (left == 2)).sum()),
                        "one_left": int((took & ~by_end & (left == 1)).sum()), "none_left": int((took & ~by_end & (left <= 0)).sum()),
                        "cut_by_hide_end": int((took & by_end & (left > 0) & (left < adv)).sum()),
                        "swap_changes_a_table": int((c.ok & nomsg.ok & (c.want["gi"]["table_select"] != nomsg.want["gi"]["table_select"]).any(1)).sum())}
    for k in ("two_left", "one_left", "none_left", "swap_changes_a_table"):
        assert counts["first"][k] >= 32, counts
    assert counts["second"]["cut_by_hide_end"] >= 32 and counts["second"]["swap_changes_a_table"] >= 32, counts
    first.counts, second.counts = counts["first"], counts["second"]
    return first, second


def region_sums(t, ix, gi):
    """bits of books 13 and 15 for the three regions of quantised spectra whose values stay below 15: int [n][3][2]"""
    h13, h15 = np.array(t["hlen13"], dtype=np.int64), np.array(t["hlen15"], dtype=np.int64)
    x, y = ix[:, 0::2].astype(np.int64), ix[:, 1::2].astype(np.int64)
    idx = np.minimum(x, 15) * 16 + np.minimum(y, 15)
    nz = (x != 0).astype(np.int64) + (y != 0)
    pair = np.arange(288)[None, :] * 2
    bounds = [np.zeros(len(ix), dtype=np.int64), gi["address1"], gi["address2"], gi["big_values"] * 2]
    sums = np.zeros((len(ix), 3, 2), dtype=np.int64)
    for r in range(3):
        m = (pair >= bounds[r][:, None]) & (pair < bounds[r + 1][:, None])
        sums[:, r, 0] = ((h13[idx] + nz) * m).sum(1)
        sums[:, r, 1] = ((h15[idx] + nz) * m).sum(1)
    return sums


@functools.lru_cache(maxsize=None)
def budget_case(orc, mlib, rate):
    """test_budgets: every family, max_bits written into the frames by hand; a step that leaves the table is the subject here"""
    t = tables(mlib)
    xr, labels = mixed(t, rate + 3, UNITS, ("sparse", "quiet", "escape_edges", "ties"))
    rf = rate_frames(mlib, rate).copy()
    rf["max_bits"] = np.array(BUDGETS)[np.arange(FRAMES) % len(BUDGETS)]
    c = Case(orc, rate, rf, xr, labels)
    c.counts = {"step_range": int((~c.ok).sum()), "step_range_by_budget": {b: int((~c.ok & (c.max_bits == b)).sum()) for b in BUDGETS}}
    assert 0 < c.counts["step_range"] < UNITS // 2, c.counts       # both outcomes are there
    return c


@functools.lru_cache(maxsize=None)
def edge_case(orc, mlib, rate):
    """escape_edges and ties under a budget that lets every unit end where it was aimed: the lowest step of the search, -119"""
    t = tables(mlib)
    xr, labels = mixed(t, rate + 4, UNITS, ("escape_edges", "ties"), steps=(-119, -119, -119, -100))
    rf = rate_frames(mlib, rate, 320).copy()
    c = Case(orc, rate, rf, xr, labels)
    assert (~c.ok).sum() <= UNITS // 10, (~c.ok).sum()
    gi, ix = c.want["gi"], c.want["ix"]
    edge = np.char.startswith(c.labels, "escape_edges") & c.ok
    top = ix.max(1)
    c.counts = {"step_range": int((~c.ok).sum()), "final_maximum": {v: int((edge & (top == v)).sum()) for v in spectra.EDGE_VALUES}}
    # quantize refuses above 8192 (:392), so 8193, 15 + 8191 and 15 + 8192 cannot be anybody's final maximum: units aimed there end further up
    for v in spectra.EDGE_VALUES:
        assert (c.counts["final_maximum"][v] >= 1) == (v <= 8192), c.counts
    assert top[c.ok].max() == 8192
    tie = np.char.startswith(c.labels, "ties") & c.ok
    ts = gi["table_select"]
    c.counts["books"] = {b: int((tie[:, None] & (ts == b)).any(1).sum()) for b in (3, 6, 8, 9, 11, 12, 13, 15)}
    small = c.ok & (top < 15)
    sums = region_sums(t, ix, gi)
    exact = small[:, None] & (ts == 15) & (sums[:, :, 0] == sums[:, :, 1])
    c.counts["regions_where_13_and_15_tie"] = int(exact.sum())
    # below 15 the reference's scan for x_len > ix_max starts at book 13, whose x_len is 16, and ends there (:1190-1193): books 3, 6, 8, 9,
    # 11 and 12 are never candidates, and the swap leads from 13 / 15 to each other only -- the one `<=` that decides is 13 against 15
    assert all(c.counts["books"][b] == 0 for b in (3, 6, 8, 9, 11, 12)), c.counts
    assert c.counts["books"][15] >= 32 and c.counts["books"][13] >= 32 and c.counts["regions_where_13_and_15_tie"] >= 32, c.counts
    return c


@functools.lru_cache(maxsize=None)
def variant_case(orc, mlib):
    """test_variant_entries: one stream of 64 frames, mixed families, a message of 200 bits behind the 32 pattern bytes"""
    rate, n = 44100, 64
    rng = np.random.default_rng(5)
    xr, labels = mixed(tables(mlib), 5, n * 4, ("sparse", "quiet", "escape_edges", "ties"))
    msg = rng.integers(0, 2, 200).astype(np.uint8)
    hide = np.concatenate([mlib.select_patterns(), msg])
    rf = rate_frames(mlib, rate, 128, n).copy()
    rf["hide_end"] = len(hide)
    segs = np.zeros(1, dtype=mlib.CHAIN_SEG_DTYPE)
    segs["n_frames"], segs["hide_base"], segs["hide_begin"], segs["hide_end"] = n, 32, 32, len(hide)
    spans, eu, ec = mlib.select_plan(segs, 1 << 16)
    reach = int(spans["reach"][0])
    tail = (200 - 2) // 3
    assert 0 < tail < reach < n * 4 and len(eu) == 8 * reach + 2 * (reach - tail)
    assert sorted(set(ec.tolist())) == [0, 4, 8, 12, 16, 20, 24, 28, len(hide) - 2, len(hide) - 1]
    own = Case(orc, rate, rf, xr, labels, None, hide, np.full(n * 4, NO_CURSOR, dtype=np.int32))
    ent = Case(orc, rate, rf, xr[eu], labels[eu], None, hide, ec.astype(np.int32), units=eu)
    for c in (own, ent):
        assert (~c.ok).sum() <= len(c.ok) // 10
    swapped = (ent.want["gi"]["table_select"] != own.want["gi"]["table_select"][eu]).any(1)
    ent.counts = {"entries": len(eu), "reach": reach, "entries_whose_tables_differ_from_the_units_own": int((ent.ok & swapped).sum())}
    assert ent.counts["entries_whose_tables_differ_from_the_units_own"] >= 32, ent.counts
    return own, ent, hide, eu, ec


# ------------------------------------------------------------------------------------------------------------------------ CPU: the hook
def test_hook_equals_rate_units_on_fresh_state(orc):
    """zero state, cursor 0, the whole message: rate_units_from is rate_units"""
    xr = spectra.sparse_spectra(11, 512)
    mb = np.array([130, 225, 764, 2000], dtype=np.int32)[np.arange(512) % 4]
    for hide in (None, np.array([1, 0, 1], dtype=np.uint8)):
        a, b = orc.rate_units(44100, mb, xr, hide), orc.rate_units_from(44100, mb, xr, None, hide)
        assert (a["rc"] == 0).sum() > 460
        for k in ("ix", "gi", "rc"):
            assert np.array_equal(a[k], b[k]), (k, hide)
        tabs = (b["gi"]["table_select"] > 0).sum(1)
        assert np.array_equal(b["advance"][b["rc"] == 0], tabs[b["rc"] == 0])


def resv_frame_end(p23, mean_bits):
    """MP3_Encoder.py:1097-1145 for resv_max == 0, two channels: what the frame's budget leaves goes into part2_3_length as stuffing bits.
    p23: [gr][ch] before, returns after."""
    p23 = p23.copy()
    stuffing = sum(mean_bits / 2 - int(v) for v in p23.reshape(-1)) + (mean_bits & 1)
    assert stuffing >= 0 and stuffing == int(stuffing)
    stuffing = int(stuffing)
    if stuffing:
        if p23[0][0] + stuffing < 4095:
            p23[0][0] += stuffing
        else:
            for gr in range(2):
                for ch in range(2):
                    this = min(4095 - p23[gr][ch], stuffing)
                    p23[gr][ch] += this
                    stuffing -= this
    return p23


def chained_streams(golden_dir):
    g = np.load(os.path.join(golden_dir, "g6_synth128.npz"))
    yield "g6_synth128", g["pcm"], 44100, 128, g["hide_bits"]
    n, rate, freq, amp = 48, 44100, 19000, 5           # tests/test_gpu_parity.py test_pilot_tone_in_digital_silence_at_low_bit_rates
    sig = np.rint(amp * np.sin(2 * np.pi * freq * np.arange(n * 1152) / rate)).astype(np.int16)
    pcm = np.ascontiguousarray(np.stack([sig, np.roll(sig, 7)], axis=1))
    pcm[20 * 1152:24 * 1152] = 0
    yield "pilot_tone", pcm, rate, 48, bits_of("12#pilot tones..")


def test_hook_chained_is_the_encoder(orc, mlib, golden_dir):
    """The encoder's own spectra fed to the hook unit by unit in the reference's order (ch outer, gr inner), the state taken from the same
    (gr, ch) of the frame before, the cursor carried: every GrInfo field, ix and the final cursor are orc.encode's -- which the goldens pin."""
    for name, pcm, rate, kbps, hide in chained_streams(golden_dir):
        o = orc.encode(pcm, rate, kbps, hide)
        assert o["rc"] == 0
        n = o["n_frames"]
        rf, pad = mlib.rate_frames(rate, kbps, 2, n)
        whole = int((2 * 576 / rate) * (1000 * kbps / 8))
        state = np.zeros((2, 2, 4), dtype=np.int32)    # [ch][gr]
        cursor, inherited_nonzero = 0, 0
        for f in range(n):
            got = np.zeros((2, 2), dtype=orc.GRINFO_DTYPE)   # [gr][ch]
            for ch in range(2):
                for gr in range(2):
                    r = orc.rate_units_from(rate, rf["max_bits"][f], o["mdct_freq"][f, ch, gr], state[ch, gr], hide, cursor)
                    assert r["rc"][0] == 0, (name, f, ch, gr)
                    gi = r["gi"][0]
                    inherited_nonzero += int(state[ch, gr, :3].any() and np.abs(o["mdct_freq"][f, ch, gr]).max() > 0)
                    state[ch, gr] = [gi["address1"], gi["address2"], gi["address3"], gi["quantizerStepSize"]]
                    cursor += int(r["advance"][0])
                    got[gr, ch] = gi
                    if np.abs(o["mdct_freq"][f, ch, gr]).max() > 0:          # (a silent unit leaves l3_enc as the frame before filled it)
                        assert np.array_equal(r["ix"][0], np.abs(o["ix"][f, ch, gr])), (name, f, ch, gr)
            mean_bits = int((8 * (whole + int(pad[f])) - 8 * 36) / 2)
            assert min(mean_bits // 2, 4095) == rf["max_bits"][f]
            got["part2_3_length"] = resv_frame_end(got["part2_3_length"], mean_bits)
            want = o["frames"]["gi"][f]
            for k in orc.GRINFO_DTYPE.names:
                assert np.array_equal(got[k], want[k]), (name, f, k, got[k].tolist(), want[k].tolist())
            assert cursor == o["frames"]["hide_off"][f]
        assert cursor == o["hide_offset"], name
        print("chained", name, "frames", n, "cursor", cursor, "active units that inherit addresses", inherited_nonzero)


@pytest.mark.parametrize("rate", RATES)
def test_conditions_hold_on_the_oracle(orc, mlib, rate):
    """what makes the device tests below mean something, from the oracle's results alone (the builders assert; the counts are printed)"""
    cases = {"inherited": [c.counts for c in inherited_cases(orc, mlib, rate)], "cursor": [c.counts for c in cursor_cases(orc, mlib, rate)],
             "budgets": budget_case(orc, mlib, rate).counts, "edges": edge_case(orc, mlib, rate).counts}
    if rate == 44100:
        cases["variants"] = variant_case(orc, mlib)[1].counts
    print("rate-unit conditions", rate, cases)                      # (pytest -s shows them)


# ------------------------------------------------------------------------------------------------------------------------ device
class Launch:
    """device buffers of one case; run() launches mp3s_rate_loop_dev (optionally on a unit list) and brings everything down"""

    def __init__(self, ctx, mlib, case):
        self.ctx, self.mlib, self.case, self.n = ctx, mlib, case, len(case.xr)
        self.frames = len(case.rf)
        self.bufs = {"mdct": ctx.to_device(case.xr), "rf": ctx.to_device(case.rf),
                     "ix": ctx.alloc(self.n * 576 * 2), "out": ctx.alloc(self.n * 72), "en": ctx.alloc(self.n * 22 * 4)}
        for k in ("hide", "cursor", "state"):
            v = getattr(case, k)
            self.bufs[k] = None if v is None or (k == "cursor" and case.hide is None) else ctx.to_device(np.ascontiguousarray(v))

    def clear(self):
        for k, size in (("ix", self.n * 576 * 2), ("out", self.n * 72), ("en", self.n * 22 * 4)):
            self.mlib.check(self.mlib.lib().mp3s_dev_memset(self.ctx.handle, self.bufs[k], 0, size))

    def run(self, unit_list=None):
        b, L = self.bufs, self.mlib.lib()
        d_list = None if unit_list is None else self.ctx.to_device(np.ascontiguousarray(unit_list, dtype=np.int32))
        try:
            self.mlib.check(L.mp3s_rate_loop_dev(self.ctx.handle, b["mdct"], b["rf"], self.frames, b["hide"],
                                                 0 if self.case.hide is None else len(self.case.hide), b["cursor"], b["state"], d_list,
                                                 0 if unit_list is None else len(unit_list), b["ix"], b["out"], b["en"]))
            self.ctx.sync()
        finally:
            if d_list is not None:
                self.ctx.free(d_list)
        return self.down()

    def down(self):
        return (self.ctx.download(self.bufs["out"], self.mlib.GR_OUT_DTYPE, (self.n,)),
                self.ctx.download(self.bufs["ix"], np.int16, (self.n, 576)).astype(np.int32),
                self.ctx.download(self.bufs["en"], np.int32, (self.n, 22)))

    def close(self):
        for p in self.bufs.values():
            if p is not None:
                self.ctx.free(p)


def launch(ctx, mlib, case):
    run = Launch(ctx, mlib, case)
    try:
        return run.run()
    finally:
        run.close()


def compare(mlib, case, got, given_state=True, units=None):
    """every record of a launch against the oracle's; `units`: only these (positions in the case)"""
    out, ix, en = got
    want, xr = case.want, case.xr
    gi, ok = want["gi"], case.ok
    pick = np.ones(len(xr), dtype=bool) if units is None else units

    def fail_at(bad, what, a, b):
        u = int(np.nonzero(bad)[0][0])
        return "%s: %d units, first %s: device %s oracle %s" % (what, int(bad.sum()), case.say(u), np.asarray(a)[u].tolist(), np.asarray(b)[u].tolist())

    def same(what, a, b, where):
        bad = pick & where & ~(np.asarray(a) == np.asarray(b)).reshape(len(xr), -1).all(1)
        assert not bad.any(), fail_at(bad, what, a, b)
    everyone = np.ones(len(xr), dtype=bool)
    nonzero = np.abs(xr).max(1) > 0
    same("MP3S_RF_STEP_RANGE against rc", (out["flags"] & mlib.RF_STEP_RANGE) != 0, ~ok, everyone)
    same("MP3S_RF_ACTIVE", (out["flags"] & mlib.RF_ACTIVE) != 0, nonzero, everyone)
    same("xrmax", out["xrmax"], np.abs(xr.astype(np.int64)).max(1), everyone)
    given = pack_state(case.state) if (case.state is not None and given_state) else np.zeros(len(xr), dtype=np.int32)
    same("reserved0 against the state given", out["reserved0"], given, everyone)
    for a, b in GI:                                     # (a silent unit: zeros, and the step it inherited)
        same(a, out[a], gi[b], ok)
    for k, f in enumerate(ADDR):
        same(f, out["address"][:, k], gi[f], ok)
    same("n_tables against the cursor's advance", out["n_tables"], want["advance"], ok)
    same("abs(ix)", np.abs(ix), want["ix"], ok & nonzero)
    same("ix of a silent unit", ix, np.zeros_like(ix), ~nonzero)
    same("signs of ix", (ix == 0) | ((ix < 0) == (xr < 0)), np.ones(ix.shape, dtype=bool), ok)
    same("en against calc_scfsi", en, want["en"], nonzero)


@pytest.mark.gpu
@pytest.mark.parametrize("rate", RATES)
def test_inherited_addresses(ctx, mlib, orc, rate):
    """state_in[u][0..2]: a probe (or the final step) without big values keeps the addresses the unit inherited, and the tables and bits of
    that probe are taken over THEM (MP3_Encoder.py:1004-1006, 1147-1168, 294-318) -- the search, the final step and the tables follow"""
    for case in inherited_cases(orc, mlib, rate):
        got = launch(ctx, mlib, case)
        print("test_inherited_addresses", rate, case.counts)
        compare(mlib, case, got)
        used = (got[0]["flags"] & mlib.RF_USED_ADDR_IN) != 0
        bad = case.depends & ~used
        assert not bad.any(), "no MP3S_RF_USED_ADDR_IN although the state changes the result: %d units, first %s" % (
            int(bad.sum()), case.say(int(np.nonzero(bad)[0][0])))


@pytest.mark.gpu
@pytest.mark.parametrize("rate", RATES)
def test_cursor_positions(ctx, mlib, orc, rate):
    """the cursor inside a message, two / one / no bits in front of its end -- the end being n_hide in the first launch, the frame's
    hide_end in the second (MP3_Encoder.py:1257-1263: only while idx < len(hide_str))"""
    for case in cursor_cases(orc, mlib, rate):
        got = launch(ctx, mlib, case)
        print("test_cursor_positions", rate, case.counts)
        compare(mlib, case, got)


@pytest.mark.gpu
@pytest.mark.parametrize("rate", RATES)
def test_budgets(ctx, mlib, orc, rate):
    """max_bits from 1 to 4095 on every family; the units whose step leaves the table (IndexError in the reference) are the oracle's"""
    case = budget_case(orc, mlib, rate)
    print("test_budgets", rate, case.counts)
    compare(mlib, case, launch(ctx, mlib, case))


@pytest.mark.gpu
@pytest.mark.parametrize("rate", RATES)
def test_table_choice_boundaries(ctx, mlib, orc, rate):
    """escape_edges and ties where they were aimed: every boundary of the table choice as a unit's final maximum, regions whose books 13 and
    15 cost exactly the same (the reference's `<=` takes 15)"""
    case = edge_case(orc, mlib, rate)
    print("test_table_choice_boundaries", rate, case.counts)
    compare(mlib, case, launch(ctx, mlib, case))


@pytest.mark.gpu
@pytest.mark.parametrize("rate", RATES)
def test_unit_lists_with_message_and_state(ctx, mlib, orc, rate):
    """lists that do not fill a workgroup's four units, with a message, cursors and state: the listed units as in the full launch, record
    for record, nothing else written"""
    case = cursor_cases(orc, mlib, rate)[1]
    run = Launch(ctx, mlib, case)
    try:
        full = run.run()
        compare(mlib, case, full)
        rng = np.random.default_rng(rate)
        for k in (1, 3, 5, 257):
            lst = rng.choice(UNITS, k, replace=False).astype(np.int32)
            listed = np.zeros(UNITS, dtype=bool)
            listed[lst] = True
            run.clear()
            part = run.run(lst)
            for name, a, b in zip(("out", "ix", "en"), part, full):
                bad = listed & ~(a == b).reshape(UNITS, -1).all(1) if name != "out" else listed & (a != b)
                assert not bad.any(), "list of %d, %s differs from the full launch: %s" % (k, name, case.say(int(np.nonzero(bad)[0][0])))
                spill = ~listed & (a.view(np.uint8).reshape(UNITS, -1) != 0).any(1)
                assert not spill.any(), "list of %d, %s written for a unit not listed: %s" % (k, name, case.say(int(np.nonzero(spill)[0][0])))
    finally:
        run.close()


@pytest.mark.gpu
def test_variant_entries(ctx, mlib, orc):
    """mp3s_rate_variants_dev: the entries behind the launch's own units -- a unit at the cursor of each of the eight 3-bit patterns and at
    "two bits left" / "one bit left" of its stream's message -- and the units' own runs behind every message"""
    own, ent, hide, eu, ec = variant_case(orc, mlib)
    n, ne, L = len(own.xr), len(eu), mlib.lib()
    print("test_variant_entries", ent.counts)
    dev = [ctx.to_device(a) for a in (own.xr, own.rf, hide, own.cursor, eu, ec)]
    outs = [ctx.alloc(n * 1152), ctx.alloc(n * 72), ctx.alloc(n * 88), ctx.alloc(ne * 1152), ctx.alloc(ne * 72 + ((ne + 15) & ~15)), ctx.alloc(ne * 88)]
    try:
        d_mdct, d_rf, d_hide, d_cur, d_eu, d_ec = dev
        d_ix, d_out, d_en, d_ixv, d_outv, d_env = outs
        mlib.check(L.mp3s_rate_variants_dev(ctx.handle, d_mdct, d_rf, len(own.rf), d_hide, len(hide), d_cur, d_eu, d_ec, ne, d_ix, d_out, d_en,
                                            d_ixv, d_outv, d_env))
        ctx.sync()
        got_own = (ctx.download(d_out, mlib.GR_OUT_DTYPE, (n,)), ctx.download(d_ix, np.int16, (n, 576)).astype(np.int32),
                   ctx.download(d_en, np.int32, (n, 22)))
        raw = ctx.download(d_outv, np.uint8, (ne * 72 + ((ne + 15) & ~15),))
        got_ent = (raw[:ne * 72].view(mlib.GR_OUT_DTYPE), ctx.download(d_ixv, np.int16, (ne, 576)).astype(np.int32),
                   ctx.download(d_env, np.int32, (ne, 22)))
        counts = raw[ne * 72:ne * 72 + ne]
    finally:
        for p in dev + outs:
            ctx.free(p)
    compare(mlib, own, got_own)
    compare(mlib, ent, got_ent)
    bad = ent.ok & (counts != ent.want["advance"])
    assert not bad.any(), "table count byte of an entry: %s" % ent.say(int(np.nonzero(bad)[0][0]))
