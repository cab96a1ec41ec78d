"""The rate loop and the encoder at 32 / 44.1 / 48 kHz against what the upstream reference ITSELF answered, not against our restatement of it.

tests/golden/g12_rate_units.npz: the reference's __iteration_loop on units of the case builders of tests/test_rate_units.py (inherited
addresses and step, cursors around the message's end, budgets from 1 bit, the boundaries of the table choice, the variant entries), chosen
and recorded by tests/golden/gen_rate_units_golden.py.  tests/golden/g13_encode_rates.npz: whole encodes and their decodes by the
reference at 48 and 32 kHz (32 / 128 / 320 kbit/s), at 44.1 kHz with 32 and 64 kbit/s, and one long stream whose message of more than 1024
bits ends inside it (tests/golden/gen_encode_rates_golden.py).

CPU: the oracle equals both fixtures in everything recorded, and the conditions that make the fixtures worth having (enough units of every
kind, every reachable final maximum, exact 13/15 ties, refusals) hold on the REFERENCE's records.  GPU: k_rate.hpp through mp3s_rate_loop_dev
/ mp3s_rate_variants_dev and the whole encoder / decoder against the fixtures."""
import hashlib
import importlib.util
import os

import numpy as np
import pytest

import spectra
import test_rate_units as RU


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _generator(golden_dir, name):
    """the generator's module: the case list, the kinds and the digests are its own (it imports the reference only when it runs)"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(golden_dir, name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def gen12(golden_dir):
    return _generator(golden_dir, "gen_rate_units_golden")


@pytest.fixture(scope="module")
def gen13(golden_dir):
    return _generator(golden_dir, "gen_encode_rates_golden")


@pytest.fixture(scope="module")
def g12(golden_dir):
    g = np.load(os.path.join(golden_dir, "g12_rate_units.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def g13(golden_dir):
    g = np.load(os.path.join(golden_dir, "g13_encode_rates.npz"))
    return {k: g[k] for k in g.files}


# ------------------------------------------------------------------------------------------------------------------------ g12: records
def records(g12, name, twin):
    """rows of the fixture for case `name` and twin code `twin`"""
    ci = list(g12["case_names"]).index(name)
    return np.nonzero((g12["case"] == ci) & (g12["twin"] == twin))[0]


def raised(g12, rows):
    return g12["error_names"][g12["error"][rows]] != ""


def reference_results(g12, name, twin, n):
    """the reference's records of a case in the shape gen_rate_units_golden.kinds reads: [n] arrays, `have` where a unit is pinned"""
    rows = records(g12, name, twin)
    u = g12["unit"][rows]
    R = {"have": np.zeros(n, dtype=bool), "ok": np.zeros(n, dtype=bool), "gi": np.zeros((n, g12["gi"].shape[1]), dtype=np.int64),
         "ts": np.zeros((n, 3), dtype=np.int64), "advance": np.zeros(n, dtype=np.int64), "top": np.zeros(n, dtype=np.int64),
         "ixd": np.zeros(n, dtype=np.uint64), "tie_regions": np.zeros(n, dtype=np.int64)}
    R["have"][u], R["ok"][u] = True, ~raised(g12, rows)
    R["gi"][u], R["ts"][u], R["advance"][u] = g12["gi"][rows], g12["table_select"][rows], g12["advance"][rows]
    R["top"][u], R["ixd"][u] = g12["ix_max"][rows], g12["ix_digest"][rows]
    s13, s15 = g12["sum13"][rows], g12["sum15"][rows]                # -1 where the generator did not count (not an edge case, or a value >= 15)
    R["tie_regions"][u] = ((s13 >= 0) & (s13 == s15) & (g12["table_select"][rows] == 15)).sum(1)
    return R


def rate_cases(gen12, orc, mlib, rate):
    return {k: c for k, c in gen12.cases(orc, mlib).items() if k.startswith("%d/" % rate)}


# ------------------------------------------------------------------------------------------------------------------------ CPU: oracle == g12
@pytest.mark.parametrize("rate", RU.RATES)
def test_oracle_rate_units_equal_the_reference(orc, mlib, gen12, g12, rate):
    """orc.rate_units_from on every pinned unit and twin: rc != 0 exactly where the reference raised (IndexError: the step left steptab),
    elsewhere every GrInfo field, the tables, the addresses, the cursor's advance and the quantised lines are the reference's"""
    fields = list(g12["gi_fields"])
    assert fields == gen12.GI_FIELDS == orc.GI_FIELDS
    total = 0
    for name, case in rate_cases(gen12, orc, mlib, rate).items():
        for twin in (gen12.OWN, gen12.ZERO_STATE, gen12.NO_MESSAGE):
            rows = records(g12, name, twin)
            if not len(rows):
                continue
            c = gen12.twin_inputs(case, twin) if twin else case
            u = g12["unit"][rows]
            drift = [int(v) for v, d in zip(u, g12["in_digest"][rows]) if gen12.input_digest(c, int(v)) != d]
            assert not drift, "%s twin %d: the builders' inputs are no longer the fixture's (run gen_rate_units_golden.py): units %s" % (name, twin, drift[:8])
            r = orc.rate_units_from(c.rate, c.max_bits[u], c.xr[u], None if c.state is None else c.state[u], c.hide,
                                    None if c.cursor is None else c.cursor[u], c.hide_end[u])
            bad = raised(g12, rows)
            assert set(g12["error_names"][g12["error"][rows]][bad]) <= {"IndexError"}, name
            assert np.array_equal(r["rc"] != 0, bad), "%s twin %d: oracle rc %s where the reference %s" % (
                name, twin, r["rc"][(r["rc"] != 0) != bad][:8].tolist(), "raised" if bad[(r["rc"] != 0) != bad][0] else "did not raise")
            assert (r["rc"][bad] == -3).all()
            ok = ~bad

            def same(what, a, b):
                miss = ok & ~(np.asarray(a) == np.asarray(b)).reshape(len(rows), -1).all(1)
                assert not miss.any(), "%s twin %d, %s: %d units, first %s: oracle %s reference %s" % (
                    name, twin, what, int(miss.sum()), c.say(int(u[miss][0])), np.asarray(a)[miss][0].tolist(), np.asarray(b)[miss][0].tolist())
            for k, f in enumerate(fields):
                same(f, r["gi"][f], g12["gi"][rows, k])
            same("table_select", r["gi"]["table_select"], g12["table_select"][rows])
            same("advance", r["advance"], g12["advance"][rows])
            same("max ix", r["ix"].max(1), g12["ix_max"][rows])
            same("sum ix", r["ix"].astype(np.int64).sum(1), g12["ix_sum"][rows])
            same("digest of ix", np.array([gen12.ix_digest(x) for x in r["ix"]], dtype=np.uint64), g12["ix_digest"][rows])
            counted = ok & (g12["sum13"][rows, 0] >= 0)
            if counted.any():                                       # books 13 and 15 over the regions: the reference's count_bit against our tables
                sums = RU.region_sums(mlib.debug_tables(), r["ix"], r["gi"])
                assert np.array_equal(sums[counted, :, 0], g12["sum13"][rows][counted]) and np.array_equal(sums[counted, :, 1], g12["sum15"][rows][counted])
            total += len(rows)
    print("pinned units and twins at", rate, ":", total)


@pytest.mark.parametrize("rate", RU.RATES)
def test_conditions_hold_on_the_reference(orc, mlib, gen12, g12, rate):
    """what the fixture is for, counted from the reference's own records (the builders' inputs, not the oracle's results): at least 32 units
    of every kind a builder promises, every fourth unit, a refusal among the budgets, every boundary of the table choice up to 8192 as a
    final maximum, regions whose books 13 and 15 tie exactly and went to 15"""
    cases = rate_cases(gen12, orc, mlib, rate)
    counts = {}
    for name, c in cases.items():
        n, what = len(c.xr), name.split("/")[1]
        R = reference_results(g12, name, gen12.OWN, n)
        u = np.arange(n)
        assert R["have"][(u + u // 4) % gen12.STRIDE == 0].all(), name
        zero = reference_results(g12, name, gen12.ZERO_STATE, n)
        nomsg = reference_results(g12, name, gen12.NO_MESSAGE, n)
        own = reference_results(g12, "44100/variant_own", gen12.OWN, len(cases["44100/variant_own"].xr)) if what == "variant_entries" else None
        k = {kind: int(m.sum()) for kind, m in gen12.kinds(name, c, R, zero, nomsg, own).items()}
        counts[name] = {kind: v for kind, v in k.items() if v}
        for kind in gen12.PROMISED[what]:
            assert k[kind] >= gen12.PER_KIND, (name, kind, k[kind])
        if what == "budgets":
            assert k["refused"] >= 1, name
        if what == "edges":
            for v in spectra.EDGE_VALUES:                            # quantize refuses above 8192 (MP3_Encoder.py:394): nobody ends there
                assert (k["final_maximum_%d" % v] >= 1) == (v <= 8192), (name, v)
            assert R["top"][R["have"] & R["ok"]].max() == 8192
            assert all(k["book_%d" % b] == 0 for b in (3, 6, 8, 9, 11, 12)), (name, k)
            assert int(R["tie_regions"].sum()) >= gen12.PER_KIND, name
            counts[name]["regions_where_13_and_15_tie"] = int(R["tie_regions"].sum())
    print("reference conditions", rate, counts)


# ------------------------------------------------------------------------------------------------------------------------ CPU: oracle == g13
def g13_case(g13, gen13, name):
    """-> (rate, kbps, pcm, message bits or None, {key: array}) with the PCM made again and checked against the fixture's hash"""
    g = {k[len(name) + 2:]: v for k, v in g13.items() if k.startswith(name + "__")}
    rate, kbps, text = int(g["rate"]), int(g["kbps"]), str(g["text"])
    pcm = gen13.long_pcm(int(g["n_frames"])) if name == "long" else gen13.case_pcm(rate, kbps)
    assert int(g["seed"]) == gen13.case_seed(rate, kbps)
    assert sha(np.ascontiguousarray(pcm, dtype="<i2").tobytes()) == bytes(g["pcm_sha256"]).decode(), "synth_pcm no longer makes the fixture's samples"
    return rate, kbps, pcm, (gen13.framed(text) if text else None), g


def g13_names(g13):
    return [str(n) for n in g13["names"]]


def test_g13_cases_are_the_generators(gen13, g13):
    assert g13_names(g13) == [gen13.case_name(r, k) for r, k in gen13.CASES]
    texts = [str(g13[n + "__text"]) for n in g13_names(g13)]
    assert texts == [gen13.case_text(i) or "" for i in range(len(texts))] and sum(1 for t in texts if t) == len(texts) // 2
    assert str(g13["long__text"]) == gen13.LONG_TEXT and len(gen13.framed(gen13.LONG_TEXT)) > 1024


def test_oracle_encodes_and_decodes_equal_the_reference(orc, gen13, g13):
    """orc.encode on every case: bytes, every GrInfo field, tables, scfsi, frame sizes, cursors, padding, too_long, the first frames' mdct_freq
    and ix; orc.decode of the reference's MP3: bits and both PCM hashes"""
    for name in g13_names(g13):
        rate, kbps, pcm, hide, g = g13_case(g13, gen13, name)
        r = orc.encode(pcm, rate, kbps, hide)
        assert r["rc"] == 0 and r["mp3"] == g["mp3"].tobytes(), name
        for i, k in enumerate(bytes(g["gi_fields"]).decode().split(",")):
            assert np.array_equal(r["frames"]["gi"][k], g["gi"][..., i]), (name, k)
        assert np.array_equal(r["frames"]["gi"]["table_select"], g["table_select"]), name
        for k in ("scfsi", "written", "hide_off", "padding"):
            assert np.array_equal(r["frames"][k], g[k]), (name, k)
        assert bool(r["too_long"]) == bool(int(g["too_long"])) and r["hide_offset"] == int(g["hide_off"][-1]), name
        head = len(g["mdct_freq"])
        assert np.array_equal(r["mdct_freq"][:head], g["mdct_freq"]) and np.array_equal(r["ix"][:head], g["ix"]), name
        d = orc.decode(g["mp3"].tobytes())
        assert d["rc"] == 0 and d["sampling_rate"] == rate and d["bit_rate"] == kbps * 1000, name
        assert np.array_equal(d["bits"], g["dec_bits"]), name
        assert sha(np.ascontiguousarray(d["pcm"]).tobytes()) == bytes(g["dec_pcm_sha256"]).decode(), name
        assert sha(orc.pcm_to_i16(d["pcm"]).tobytes()) == bytes(g["dec_pcm_i16_sha256"]).decode(), name


def test_oracle_long_message_equals_the_reference(orc, gen13, g13):
    rate, kbps, pcm, hide, g = g13_case(g13, gen13, "long")
    r = orc.encode(pcm, rate, kbps, hide)
    assert r["rc"] == 0 and r["mp3"] == g["mp3"].tobytes()
    assert np.array_equal(r["frames"]["hide_off"], g["hide_off"]) and bool(r["too_long"]) == bool(int(g["too_long"]))


def test_g13_conditions_hold_on_the_reference(gen13, g13):
    """from the reference's records alone: both paddings at 44.1 kHz, a granule without big values between active ones, messages that
    were placed, and the long message ending inside its stream"""
    pads_44 = set()
    for name in g13_names(g13):
        pad, bv = g13[name + "__padding"], g13[name + "__gi"][..., 1]                     # [f][gr][ch]
        assert bytes(g13[name + "__gi_fields"]).decode().split(",")[1] == "big_values"
        if int(g13[name + "__rate"]) == 44100:                       # (64 kbit/s: 208.98 slots a frame, padded but once in 49 frames)
            pads_44 |= set(pad.tolist())
        active = (bv > 0).any((1, 2))
        inside = [f for f in range(1, len(bv) - 1) if (bv[f] == 0).any() and active[:f].any() and active[f + 1:].any()]
        assert inside, name
        if str(g13[name + "__text"]):
            assert int(g13[name + "__hide_off"][-1]) > 0, name
    assert pads_44 == {0, 1}
    off, n_bits = g13["long__hide_off"], len(gen13.framed(gen13.LONG_TEXT))
    assert not int(g13["long__too_long"]) and len(off) == int(g13["long_frames"]) == int(g13["long__n_frames"])
    assert off[-1 - gen13.LONG_SPARE] >= n_bits > off[-2 - gen13.LONG_SPARE]


# ------------------------------------------------------------------------------------------------------------------------ GPU: rate loop
def compare_with_reference(mlib, gen12, g12, name, case, got):
    """the device's records of the pinned units of a case against the reference's"""
    out, ix, _ = got
    rows = records(g12, name, gen12.OWN)
    u = g12["unit"][rows]
    fields = list(g12["gi_fields"])
    bad = raised(g12, rows)
    ok = ~bad

    def same(what, a, b, where):
        miss = where & ~(np.asarray(a) == np.asarray(b)).reshape(len(rows), -1).all(1)
        assert not miss.any(), "%s, %s: %d units, first %s: device %s reference %s" % (
            name, what, int(miss.sum()), case.say(int(u[miss][0])), np.asarray(a)[miss][0].tolist(), np.asarray(b)[miss][0].tolist())
    everyone = np.ones(len(rows), dtype=bool)
    same("MP3S_RF_STEP_RANGE against the reference's IndexError", (out["flags"][u] & mlib.RF_STEP_RANGE) != 0, bad, everyone)
    for a, b in RU.GI:
        same(a, out[a][u], g12["table_select"][rows] if b == "table_select" else g12["gi"][rows, fields.index(b)], ok)
    for k, f in enumerate(RU.ADDR):
        same(f, out["address"][u, k], g12["gi"][rows, fields.index(f)], ok)
    same("n_tables against the cursor's advance", out["n_tables"][u], g12["advance"][rows], ok)
    same("max |ix|", np.abs(ix[u]).max(1), g12["ix_max"][rows], ok)
    same("digest of |ix|", np.array([gen12.ix_digest(x) for x in ix[u]], dtype=np.uint64), g12["ix_digest"][rows], ok)
    xr = case.xr[u]
    same("signs of ix", (ix[u] == 0) | ((ix[u] < 0) == (xr < 0)), np.ones(xr.shape, dtype=bool), ok)
    return len(rows), int(bad.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("rate", RU.RATES)
def test_rate_loop_equals_the_reference(ctx, mlib, orc, gen12, g12, rate):
    """mp3s_rate_loop_dev on the builders' launches (1024 units each); on the pinned units every GrInfo field, the tables, the addresses,
    the advance, the quantised lines (digest and signs) and the refusals are the reference's"""
    for name, case in rate_cases(gen12, orc, mlib, rate).items():
        if name.split("/")[1].startswith("variant"):
            continue
        n, refused = compare_with_reference(mlib, gen12, g12, name, case, RU.launch(ctx, mlib, case))
        print("test_rate_loop_equals_the_reference", name, "pinned", n, "refused", refused)


@pytest.mark.gpu
def test_variant_entries_equal_the_reference(ctx, mlib, orc, gen12, g12):
    """mp3s_rate_variants_dev (the launch of tests/test_rate_units.py test_variant_entries): the units' own runs and the entries at the
    cursors of the eight patterns and of the message's last bits, against the reference's records of both"""
    own, ent, hide, eu, ec = RU.variant_case(orc, mlib)
    n, ne, L = len(own.xr), len(eu), mlib.lib()
    dev = [ctx.to_device(a) for a in (own.xr, own.rf, hide, own.cursor, eu, ec)]
    outs = [ctx.alloc(n * 1152), ctx.alloc(n * 72), ctx.alloc(n * 88), ctx.alloc(ne * 1152), ctx.alloc(ne * 72 + ((ne + 15) & ~15)), ctx.alloc(ne * 88)]
    try:
        d_mdct, d_rf, d_hide, d_cur, d_eu, d_ec = dev
        d_ix, d_out, d_en, d_ixv, d_outv, d_env = outs
        mlib.check(L.mp3s_rate_variants_dev(ctx.handle, d_mdct, d_rf, len(own.rf), d_hide, len(hide), d_cur, d_eu, d_ec, ne, d_ix, d_out, d_en,
                                            d_ixv, d_outv, d_env))
        ctx.sync()
        got_own = (ctx.download(d_out, mlib.GR_OUT_DTYPE, (n,)), ctx.download(d_ix, np.int16, (n, 576)).astype(np.int32), None)
        raw = ctx.download(d_outv, np.uint8, (ne * 72 + ((ne + 15) & ~15),))
        got_ent = (raw[:ne * 72].view(mlib.GR_OUT_DTYPE), ctx.download(d_ixv, np.int16, (ne, 576)).astype(np.int32), None)
    finally:
        for p in dev + outs:
            ctx.free(p)
    cases = gen12.cases(orc, mlib)
    for name, got in (("44100/variant_own", got_own), ("44100/variant_entries", got_ent)):
        print("test_variant_entries_equal_the_reference", name, compare_with_reference(mlib, gen12, g12, name, cases[name], got))
    rows = records(g12, "44100/variant_entries", gen12.OWN)
    ok = ~raised(g12, rows)
    assert np.array_equal(raw[ne * 72:ne * 72 + ne][g12["unit"][rows]][ok], g12["advance"][rows][ok]), "table count byte of an entry"


# ------------------------------------------------------------------------------------------------------------------------ GPU: whole encoder
@pytest.mark.gpu
@pytest.mark.parametrize("index", range(8))
def test_encoder_equals_the_reference(ctx, mlib, orc, gen13, g13, index):
    """one case of g13 through encode_pcm (bytes, cursor, too_long, every granule, scfsi), encode_transform in both forms (the first frames'
    mdct_freq) and decode_stream of the reference's MP3 (bits, both PCM hashes).  A case with a message also goes through hide_messages on
    the reference's MP3 of the same PCM without a message; that leg compares with orc.encode of the decoded PCM, so it rests on
    test_oracle_encodes_and_decodes_equal_the_reference above."""
    from test_gpu_parity import _check_gr
    name = g13_names(g13)[index]
    rate, kbps, pcm, hide, g = g13_case(g13, gen13, name)
    r = ctx.encode_pcm(pcm, rate, kbps, hide)
    assert r["mp3"] == g["mp3"].tobytes(), name
    assert r["hide_offset"] == int(g["hide_off"][-1]) and r["too_long"] == bool(int(g["too_long"])), name
    _check_gr(r, g)                                                   # (part2_3_length: the bytes; the fixture's holds the frame's stuffing bits)
    head = len(g["mdct_freq"])
    for fused in (0, 1):
        old = ctx.set_option("fused_encode", fused)
        try:
            assert np.array_equal(ctx.encode_transform(pcm)[:head], g["mdct_freq"]), (name, fused)
        finally:
            ctx.set_option("fused_encode", old)
    d = ctx.decode_stream(g["mp3"].tobytes(), mlib.MP3S_PCM_F64)
    assert d["sampling_rate"] == rate and d["bit_rate"] == kbps * 1000 and np.array_equal(d["bits"], g["dec_bits"]), name
    assert sha(np.ascontiguousarray(d["pcm"]).tobytes()) == bytes(g["dec_pcm_sha256"]).decode(), name
    d16 = ctx.decode_stream(g["mp3"].tobytes(), mlib.MP3S_PCM_I16)
    assert sha(np.ascontiguousarray(d16["pcm"]).tobytes()) == bytes(g["dec_pcm_i16_sha256"]).decode(), name
    if hide is not None:
        plain = g["plain_mp3"].tobytes()
        got = ctx.hide_messages([plain], [str(g["text"])])[0]
        assert not isinstance(got, Exception), got
        o = orc.decode(plain)
        want = orc.encode(orc.pcm_to_i16(o["pcm"]), rate, kbps, hide)
        assert want["rc"] == 0 and got["data"] == want["mp3"], name
        assert got["hide_offset"] == want["hide_offset"] and got["too_long"] == bool(want["too_long"]), name


@pytest.mark.gpu
def test_long_message_equals_the_reference(ctx, gen13, g13):
    """a message of more than 1024 bits that ends inside the stream: bytes and cursor of encode_pcm"""
    rate, kbps, pcm, hide, g = g13_case(g13, gen13, "long")
    r = ctx.encode_pcm(pcm, rate, kbps, hide)
    assert r["mp3"] == g["mp3"].tobytes()
    assert r["hide_offset"] == int(g["hide_off"][-1]) and r["too_long"] == bool(int(g["too_long"]))
