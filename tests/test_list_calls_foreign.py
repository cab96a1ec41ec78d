"""The list-of-files calls -- reveal_messages, capacities, pcm_distortions / hide_distortions, pcm_alignments / stego_distortions and
table_audits -- on streams the library's own encoder never writes: per-frame VBR, rate switches inside one reservoir, reserved rate
bits, a last frame of its own, CRC on some frames, main_data_begin 511, short / start / stop / mixed blocks, inherited scalefactors
(gpu_ok == 0), mono, a late channel change (tests/vbr_streams.py, tests/frame_synth.py), mixed in one list with tests/golden/test.mp3
and a CBR file of the library's own.

No expectation comes from a call under test or from its kernels: the oracle's decode and re-encode (tests/oracle_lib.py, pinned to
the reference on such streams by tests/test_vbr_golden.py), numpy in int64 on the oracle's int16, and tests/table_audit_model.py.
What the inputs are worth (which stream reaches which clause) is asserted on the oracle's and the model's side, without a device."""
import functools
import os

import numpy as np
import pytest

import frame_synth as F
import table_audit_model as M
import vbr_streams as V
from test_capacity import hide_messages_list, oracle_clear_capacity
from test_pcm_alignment import check_alignment, expect_alignment
from test_pcm_distortion import check_pair, expect_pairs
from test_reveal_batch import last_definer
from test_table_audit import same as same_audit
from test_vbr_streams import FAMILIES, expect_hide, options, oracle_i16, ref, single_error, streams

gpu = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G7 = ["books_4_14_id3", "joint_ms_blocks_48", "long_reservoir_44", "mixed_blocks_44", "mono_crc_32", "no_reservoir_32k_lowrate"]
INHERIT = {"inherit_0": 0, "inherit_3": 3}                         # test_inherited_scalefactors_far_back_and_in_a_batch's streams 0 and 3 (stereo)
TOO_LONG = hide_messages_list()[3]                                   # 1 800 characters: fits into none of the streams
SHORT_MESSAGE = "list"
KDECODE_CHUNK = 16384                                                # kDecodeChunk of mp3s_decode_pipeline.cpp
OPTIONS = [dict(device_parse=0), dict(fast_imdct=0), dict(fused_decode=0)]


# ------------------------------------------------------------------------------------------------ the inputs
@functools.lru_cache(maxsize=None)
def stream_bytes(name):
    """one input by name; a family is synthesised when its first stream is asked for, so that no single test pays for all of them"""
    if name[:2] in ("a_", "c_", "d_", "e_"):
        return FAMILIES[name[0]]()[name]
    if name[:2] in ("g_", "f_"):
        return (V.family_g() if name[0] == "g" else V.family_f())[name]
    if name in INHERIT:
        i = INHERIT[name]
        return F.make_stream(20 + i, 90 + 17 * i, block_types=(0, 1, 2, 3), allow_mixed=True)
    if name == "mono_other_seed":
        return F.make_stream(1203, 36, bitrate_idx=V._vbr(36), mode=3, block_types=V.BLOCKS, allow_mixed=True)
    if name == "cbr":
        return open(os.path.join(GOLDEN, "test.mp3"), "rb").read()
    if name == "own_cbr":                                            # (test_own_cbr_is_the_librarys_output: the same bytes)
        from synth_pcm import synth_pcm
        import oracle_lib
        return oracle_lib.encode(synth_pcm(20, seed=6100), 44100, 128)["mp3"]
    assert name in G7, name
    return np.load(os.path.join(GOLDEN, "g7_decode_corpus.npz"))[name + "__mp3"].tobytes()


@functools.lru_cache(maxsize=None)
def inputs():
    """name -> bytes in the order of the batch: the short families a, c, d, e (c_offsets: 1 089 frames), family g, the g7 corpus, two
    inherited-scalefactor streams and a second mono stream; test.mp3 ("cbr"), the library's own CBR output and the two refused
    streams of family f stand between them"""
    foreign = list(streams("a", "c", "d", "e", long=False)) + list(V.G_SR_IDX) + G7 + list(INHERIT) + ["mono_other_seed"]
    between = {2: "cbr", 7: "f_to_mono_late", 12: "own_cbr", 19: "f_to_stereo_late"}
    names = []
    for k, name in enumerate(foreign):
        names += [between[k], name] if k in between else [name]
    assert len(names) == len(set(names)) == len(foreign) + 4
    return {name: stream_bytes(name) for name in names}


_known = {}                                                          # bytes -> the oracle's decode of them


def oracle(orc, name):
    """the oracle's decode of an input (shared with tests/test_vbr_streams.py through its cache), or None for a stream it refuses"""
    if name.startswith("f_"):
        return None
    data = stream_bytes(name)
    _known[data] = ref(orc, name, data)
    return _known[data]


class OracleDecodes:
    """stands where expect_pairs / expect_alignment take a context: decode_streams answers with the oracle's decode of the bytes"""

    def __init__(self, orc):
        self.orc, self.known = orc, _known

    def decode_streams(self, files, per_file=True):
        out = []
        for f in files:
            f = bytes(f)
            if f not in self.known:
                self.known[f] = self.orc.decode(f)
                assert self.known[f]["rc"] == 0
            o = self.known[f]
            out.append({"pcm": oracle_i16(o), "channels": o["channels"], "sampling_rate": o["sampling_rate"], "n_frames": o["n_frames"]})
        return out


def oracle_decodes(orc):
    return OracleDecodes(orc)


def g_rates(name):
    """each frame's effective rate index of a family g stream, from the list the stream was built with: reserved bits keep the rate"""
    out, eff = [], None
    for s in V.G_SR_IDX[name]:
        eff = s if s != 3 else eff
        out.append(eff)
    return out


@functools.lru_cache(maxsize=None)
def audit_model(name):
    from mp3stego import _lib
    return M.audit_file(_lib, stream_bytes(name), g_rates(name) if name in V.G_SR_IDX else None)


def capacity_clear(orc, mlib, name):
    """oracle_clear_capacity of an input, computed once"""
    o = oracle(orc, name)
    if "cap" not in o:
        o["cap"] = oracle_clear_capacity(orc, mlib, o)
    return o["cap"]


SHORT_PAIRS = [("a_48_stereo", "a_48_joint"),                        # stereo against joint, device-parsed.  Both decode far outside [-1, 1]: the wrapped int16 differ by more than 60 000 and a frame's err2 passes 2^32
               ("a_44_joint", "a_44_stereo"),                        # ... and host-repaired (mixed blocks: gpu_ok == 0)
               ("e_reserved_48", "a_48_stereo"),                     # reserved rate bits against VBR, 40 frames against 36
               ("c_per_frame", "g_reserved_44_long"),                # a rate switch per frame (the last frame is 44.1 kHz) against 44.1 kHz, 96 against 40
               ("inherit_0", "inherit_3"),                           # gpu_ok == 0 on both sides, 90 against 141
               ("mono_other_seed", "a_44_mono"),
               ("d_last_rate", "a_32_stereo"),                       # 39 frames at 48 kHz and a last one at 32: a 32 kHz stream to the pair calls
               ("a_48_joint", "clear:a_48_joint")]                   # a foreign stream against the library's re-encode of it
ALIGN_PAIRS = [SHORT_PAIRS[0], SHORT_PAIRS[4], SHORT_PAIRS[5]]
HIDE_NAMES = ["a_44_joint", "a_48_stereo", "d_last_bitrate", "e_reserved_48"]   # d_last_bitrate: 39 frames at 224 kbit/s, the last at 80; none at 32 kHz
HIDE_MESSAGES = ["list a_44_joint", TOO_LONG, "list d_last_bitrate", "list e_reserved_48"]


def pair_bytes(orc, mlib, name):
    if name.startswith("clear:"):
        return expect_hide(orc, mlib, oracle(orc, name[6:]), None)["mp3"]
    oracle(orc, name)                                                # (its decode is known to oracle_decodes from here on)
    return stream_bytes(name)


def pair_lists(orc, mlib, pairs):
    return [pair_bytes(orc, mlib, a) for a, _ in pairs], [pair_bytes(orc, mlib, b) for _, b in pairs]


_pair_wants = {}


def short_pair_wants(orc, mlib):
    if "short" not in _pair_wants:
        a, b = pair_lists(orc, mlib, SHORT_PAIRS)
        _pair_wants["short"] = (a, b, expect_pairs(oracle_decodes(orc), a, b))
    return _pair_wants["short"]


# ------------------------------------------------------------------------------------------------ no device: what the inputs are worth
def test_inputs_reach_the_clauses(mlib, orc):
    names = list(inputs())
    assert names.index("a_44_stereo") < names.index("cbr") < names.index("own_cbr") < names.index("mono_other_seed")
    o = {n: oracle(orc, n) for n in names}
    for n in V.family_f():
        assert o[n] is None and orc.decode(inputs()[n])["rc"] != 0
    good = [n for n in names if o[n] is not None]
    # CRC on some frames only; mono; several (rate, bit rate) groups and both channel counts in one list
    some_crc = [n for n in good if 0 < ((o[n]["frames"]["hdr"][:, 1] & 1) == 0).sum() < o[n]["n_frames"]]
    assert "a_44_crc_some" in some_crc
    assert sum(o[n]["channels"] == 1 for n in good) >= 5
    assert len({(o[n]["sampling_rate"], o[n]["bit_rate"]) for n in good}) >= 10
    # more than one mode and more than one rate inside a stream
    assert len(set(o["c_per_frame"]["frames"]["sr_idx"])) == 3 and len(set(o["c_offsets"]["frames"]["sr_idx"])) == 3
    assert len(set(o["a_44_joint"]["frames"]["hdr"][:, 3] >> 4)) == 4            # joint stereo with every mode extension
    # a window-switching granule in the first frame of a 256-frame tile inherits a non-zero third index from the tile before
    carries = 0
    for n in good:
        u = o[n]["frames"]
        for f in range(mlib.REVEAL_TILE, o[n]["n_frames"], mlib.REVEAL_TILE):
            for gr in range(2):
                for ch in range(o[n]["channels"]):
                    if u[f]["window_switching"][gr][ch] and u[f]["table_select"][gr][ch][2]:
                        d = last_definer(u, f, gr, ch)
                        assert 0 <= d < f and u[d]["table_select"][gr][ch][2] == u[f]["table_select"][gr][ch][2]
                        carries += 1
    assert carries >= 2, carries
    # host-repaired and device-parsed streams side by side
    ok = {n: mlib.scan_stream(inputs()[n])["gpu_ok"] for n in good}
    assert not ok["inherit_0"] and not ok["inherit_3"] and not ok["a_44_stereo"] and ok["a_48_stereo"] and ok["cbr"] and ok["own_cbr"]
    assert sum(not v for v in ok.values()) >= 5 and sum(ok.values()) >= 15
    # decoded far outside [-1, 1]: the int16 wrap
    assert sum(np.abs(o[n]["pcm"]).max() > 20 for n in good) >= 10
    assert all(oracle_i16(o[n]).shape == (o[n]["n_frames"] * 1152, o[n]["channels"]) for n in good)


def test_family_g_rates_come_from_the_frame_before(mlib, orc):
    for name, data in V.family_g().items():
        bits, eff = V.G_SR_IDX[name], g_rates(name)
        assert sum(b == 3 for b in bits) >= 5 and bits[-1] == 3 and bits[0] != 3 and len(bits) == 40
        s = mlib.scan_stream(data)
        assert s["n_frames"] == 40 and [(int(h[2]) >> 2) & 3 for h in oracle(orc, name)["frames"]["hdr"]] == bits
        assert [int(x) for x in s["side"]["sr_idx"]] == eff, name
        assert [int(x) for x in oracle(orc, name)["frames"]["sr_idx"]] == eff, name
        assert not s["side"]["unit"]["window_switching"].any() and set(eff) == {bits[0]} and bits[0] in (0, 1)
        assert (s["sampling_rate"], oracle(orc, name)["sampling_rate"]) == ((44100, 48000)[bits[0]],) * 2


def test_audit_model_depends_on_the_rate(mlib):
    """on the model's side: a rate-switching stream has long-block units in frames of several rates, and in family g a unit of a
    reserved frame classifies differently under the 32 kHz bounds (the header's two bits, clamped) and under the 44.1 kHz bounds (a
    rate index of 0) than under its own"""
    for name in ("c_offsets", "c_per_frame"):
        s = mlib.scan_stream(stream_bytes(name))
        plain = (s["side"]["unit"]["window_switching"] == 0).reshape(s["n_frames"], -1).any(axis=1)
        assert len(set(int(r) for r in s["side"]["sr_idx"][plain])) == 3, name
    for name, data in V.family_g().items():
        p, s = mlib.parse_stream(data), mlib.scan_stream(data)
        eff = g_rates(name)
        reserved = np.array([b == 3 for b in V.G_SR_IDX[name]])
        true = M.audit_units(p["is"], s["side"], 2, eff)
        as_32k = M.audit_units(p["is"], s["side"], 2, [2 if r else e for r, e in zip(reserved, eff)])
        assert (true[reserved] != as_32k[reserved]).any() and (true[~reserved] == as_32k[~reserved]).all(), name
        assert M.audit_stream(true)[0] != M.audit_stream(as_32k)[0], name
    p, s = mlib.parse_stream(V.family_g()["g_reserved_48_long"]), mlib.scan_stream(V.family_g()["g_reserved_48_long"])
    assert M.audit_stream(M.audit_units(p["is"], s["side"], 2, [0] * 40))[0] != M.audit_stream(M.audit_units(p["is"], s["side"], 2, g_rates("g_reserved_48_long")))[0]
    assert audit_model("g_reserved_48_long")["regions"] > 300 and audit_model("c_offsets")["window_units"] > 0


def test_oracle_expectations_without_a_device(mlib, orc):
    """the capacity of the oracle's clear re-encode is the bit count its own decoder reads back; the short pairs hold what they are
    listed for"""
    for name in inputs():
        o = oracle(orc, name)
        if o is None or o["channels"] != 2:
            continue
        w = capacity_clear(orc, mlib, name)
        assert len(w["profile"]) == o["n_frames"] and int(w["profile"][-1]) == w["bits"] and 0 < w["active_units"] <= 4 * o["n_frames"], name
        back = orc.decode(w["mp3"])
        if back["n_frames"] == o["n_frames"]:                        # (at 32 kHz and some bit rates the reference's decoder loses sync on the reference's output)
            assert len(back["bits"]) == w["bits"], name
        else:
            assert o["sampling_rate"] == 32000, name
    a, b, want = short_pair_wants(orc, mlib)
    assert all(w is not None for w in want)
    assert [w["channels"] for w in want] == [2, 2, 2, 2, 2, 1, 2, 2] and [w["sampling_rate"] for w in want] == [48000, 44100, 48000, 44100, 44100, 44100, 32000, 48000]
    assert [(w["rows_a"] // 1152, w["rows_b"] // 1152) for w in want] == [(36, 36), (36, 36), (40, 36), (96, 40), (90, 141), (36, 36), (40, 36), (36, 36)]
    w = want[0]                                                      # a_48_stereo against a_48_joint
    assert (w["profile"]["err2"] > 1 << 32).any() and w["max_abs"] > 60000 and w["profile"]["max_abs"].max() > 60000
    assert all(w["err2"] > 0 for w in want)


# ------------------------------------------------------------------------------------------------ GPU
@gpu
def test_own_cbr_is_the_librarys_output(ctx, mlib):
    from synth_pcm import synth_pcm
    assert bytes(ctx.encode_pcm(synth_pcm(20, seed=6100), 44100, 128, None)["mp3"]) == stream_bytes("own_cbr")


@gpu
def test_a_pair_batch_past_one_decode_chunk(ctx, mlib, orc):
    """three pairs of 3 001 frames a side: A and B of each pair lie side by side in one batch of 18 006 frames, so the decode chunk
    ends, and its halo frame and the copy into the kept PCM fall, inside the fourth of the six streams"""
    fb = V.family_b()
    x, y = fb["b_32_then_320"], fb["b_320_then_32"]
    ox, oy = ref(orc, "b_32_then_320", x), ref(orc, "b_320_then_32", y)
    assert ox["n_frames"] == oy["n_frames"] == 3001 and ox["channels"] == oy["channels"] == 2 and ox["sampling_rate"] == oy["sampling_rate"] == 44100
    firsts = np.cumsum([0] + [3001] * 6)
    inside = [k for k in range(6) if firsts[k] < KDECODE_CHUNK < firsts[k + 1]]
    assert inside == [5] and firsts[6] == 18006                      # strictly inside the last stream
    dec = oracle_decodes(orc)
    dec.known[x], dec.known[y] = ox, oy
    a, b = [x, y, x], [y, x, y]
    want = expect_pairs(dec, a, b)
    assert want[0]["err2"] > 0 and want[0]["n_frames"] == 3001
    out = ctx.pcm_distortions(a, b, profile=True)
    for i, (r, w) in enumerate(zip(out, want)):
        check_pair(i, r, w)
    out = ctx.pcm_alignments(a, b, lags=[0, 0, 0], profile=True)
    for i, r in enumerate(out):
        check_alignment(i, r, align_want(orc, a[i], b[i], 64, 1152, lag=0))
        check_pair(i, r, want[i])
    out = ctx.pcm_alignments(a, b, max_lag=64, search_rows=1152, profile=True)
    for i, r in enumerate(out):
        w = align_want(orc, a[i], b[i], 64, 1152)
        assert w["scores"] is not None and len(w["scores"]) == 129
        check_alignment(i, r, w)


def align_want(orc, a, b, max_lag, search_rows, lag=None):
    key = ("align", a, b, max_lag, search_rows, lag)
    if key not in _pair_wants:
        _pair_wants[key] = expect_alignment(oracle_decodes(orc), a, b, max_lag, search_rows, lag)
    return _pair_wants[key]


@gpu
def test_pcm_alignments_of_foreign_pairs_match_the_numpy_loop(ctx, mlib, orc):
    a, b = pair_lists(orc, mlib, ALIGN_PAIRS)
    out = ctx.pcm_alignments(a, b, profile=True)                     # max_lag 2304, search_rows 4608: every stream has the rows
    for i, r in enumerate(out):
        w = align_want(orc, a[i], b[i], 2304, 4608)
        assert w["scores"] is not None and w["search_rows"] == 4608
        check_alignment(ALIGN_PAIRS[i], r, w)


def check_short_pairs(ctx, mlib, orc):
    a, b, want = short_pair_wants(orc, mlib)
    out = ctx.pcm_distortions(a, b, profile=True)
    assert len(out) == len(want)
    for i, (r, w) in enumerate(zip(out, want)):
        check_pair(SHORT_PAIRS[i], r, w)


@gpu
def test_pcm_distortions_of_foreign_pairs_match_numpy(ctx, mlib, orc):
    check_short_pairs(ctx, mlib, orc)
    assert bytes(ctx.clear_file(stream_bytes("a_48_joint"))["data"]) == pair_bytes(orc, mlib, "clear:a_48_joint")


def check_reveal(ctx, mlib, orc, max_streams=None):
    names, files = list(inputs()), list(inputs().values())
    out = ctx.reveal_messages(files, _max_streams=max_streams)
    assert len(out) == len(files)
    for n, f, r in zip(names, files, out):
        o = oracle(orc, n)
        if o is None:
            code = single_error(ctx, lambda: mlib.reveal_message(f))
            assert code in (mlib.E_MALFORMED, mlib.E_UNSUPPORTED) and code == single_error(ctx, lambda: ctx.decode_stream(f)), (n, code)
            assert isinstance(r, mlib.Mp3sError) and r.code == code, (n, r, code)
            continue
        assert not isinstance(r, Exception), (n, r)
        assert len(r["bits"]) == len(o["bits"]) and np.array_equal(r["bits"], o["bits"]), n
        assert r["data"] == mlib.message_reveal(o["bits"]), n
        assert (r["n_frames"], r["channels"], r["sampling_rate"], r["kbps"]) == (o["n_frames"], o["channels"], o["sampling_rate"], o["bit_rate"] // 1000), n


@gpu
@pytest.mark.parametrize("max_streams", [None, 1])
def test_reveal_messages_reads_the_oracles_bits(ctx, mlib, orc, max_streams):
    check_reveal(ctx, mlib, orc, max_streams)


def check_capacity(ctx, mlib, orc, message=None):
    names, files = list(inputs()), list(inputs().values())
    out = ctx.capacities(files, None if message is None else [message] * len(files), profile=True)
    assert len(out) == len(files)
    fits = 0
    for n, f, r in zip(names, files, out):
        o = oracle(orc, n)
        if o is None or o["channels"] != 2:                          # mono and the late channel change: what clear_file says
            code = single_error(ctx, lambda: ctx.clear_file(f))
            assert code != 0 and isinstance(r, mlib.Mp3sError) and r.code == code, (n, r, code)
            continue
        assert not isinstance(r, Exception), (n, r)
        assert (r["n_frames"], r["kbps"], r["sampling_rate"], r["channels"]) == (o["n_frames"], o["bit_rate"] // 1000, o["sampling_rate"], 2), n
        assert r["fallback"] in (0, 1), n
        if message is None:
            w = capacity_clear(orc, mlib, n)
            assert (r["bits"], r["active_units"]) == (w["bits"], w["active_units"]), (n, r["bits"], w["bits"], r["active_units"], w["active_units"])
            assert np.array_equal(r["profile"], w["profile"]), (n, np.nonzero(r["profile"] != w["profile"])[0][:4])
            assert r["text_bytes"] == mlib.capacity_text_bytes(w["bits"]) and not r["too_long"], n
        else:
            e = expect_hide(orc, mlib, o, message)
            assert (r["hide_offset"], r["too_long"]) == (e["hide_offset"], e["too_long"]), (n, r["hide_offset"], r["too_long"], e["hide_offset"], e["too_long"])
            if e["too_long"]:
                assert r["bits"] == e["hide_offset"], (n, r["bits"], e["hide_offset"])
            fits += not e["too_long"]
    return fits


@gpu
def test_clear_capacities_are_the_oracles_re_encode(ctx, mlib, orc):
    check_capacity(ctx, mlib, orc)


@gpu
def test_capacities_with_a_message_that_does_not_fit(ctx, mlib, orc):
    fits = check_capacity(ctx, mlib, orc, TOO_LONG)
    assert fits == 0                                                 # (not even into the 1 089 frames of c_offsets)


@gpu
def test_capacities_with_a_short_message(ctx, mlib, orc):
    fits = check_capacity(ctx, mlib, orc, SHORT_MESSAGE)
    assert fits >= 20


@gpu
def test_refused_pairs_get_their_code_and_their_neighbours_their_answer(ctx, mlib, orc):
    pairs = [SHORT_PAIRS[0], ("a_44_mono", "a_44_stereo"), ("d_last_rate", "a_48_stereo"), SHORT_PAIRS[3], ("f_to_mono_late", "a_44_stereo"),
             ("a_44_stereo", "f_to_stereo_late"), SHORT_PAIRS[4], ("a_32_stereo", "a_44_stereo")]
    a, b = pair_lists(orc, mlib, pairs)
    late = [single_error(ctx, lambda: ctx.decode_stream(V.family_f()[n])) for n in ("f_to_mono_late", "f_to_stereo_late")]
    assert all(c in (mlib.E_MALFORMED, mlib.E_UNSUPPORTED) for c in late)
    codes = {1: mlib.E_UNSUPPORTED, 2: mlib.E_UNSUPPORTED, 4: late[0], 5: late[1], 7: mlib.E_UNSUPPORTED}
    _, _, want = short_pair_wants(orc, mlib)
    out = ctx.pcm_distortions(a, b, profile=True)
    for i, r in enumerate(out):
        if i in codes:
            assert isinstance(r, mlib.Mp3sError) and r.code == codes[i], (pairs[i], r, codes[i])
        else:
            check_pair(pairs[i], r, want[SHORT_PAIRS.index(pairs[i])])
    lagged = ctx.pcm_alignments(a, b, lags=[0] * len(a), profile=True)
    for i, r in enumerate(lagged):
        if i in codes:
            assert isinstance(r, mlib.Mp3sError) and r.code == codes[i], (pairs[i], r, codes[i])
        else:
            check_pair(pairs[i], r, want[SHORT_PAIRS.index(pairs[i])])


@gpu
def test_hide_distortions_is_numpy_on_the_oracles_re_encodes(ctx, mlib, orc):
    files = [stream_bytes(n) for n in HIDE_NAMES]
    clear = [expect_hide(orc, mlib, oracle(orc, n), None) for n in HIDE_NAMES]
    hidden = [expect_hide(orc, mlib, oracle(orc, n), m) for n, m in zip(HIDE_NAMES, HIDE_MESSAGES)]
    want = expect_pairs(oracle_decodes(orc), [c["mp3"] for c in clear], [h["mp3"] for h in hidden])
    assert [h["too_long"] for h in hidden] == [False, True, False, False] and all(w["err2"] > 0 for w in want)
    assert all(oracle(orc, n)["sampling_rate"] != 32000 and w["n_frames"] == oracle(orc, n)["n_frames"] for n, w in zip(HIDE_NAMES, want))
    out = ctx.hide_distortions(files, HIDE_MESSAGES, profile=True)
    for n, r, w, h in zip(HIDE_NAMES, out, want, hidden):
        check_pair(n, r, w)
        assert (r["hide_offset"], r["too_long"]) == (h["hide_offset"], h["too_long"]), (n, r["hide_offset"], r["too_long"], h["hide_offset"], h["too_long"])


@gpu
def test_stego_distortions_is_the_numpy_loop_on_the_oracles_re_encode(ctx, mlib, orc):
    files = [stream_bytes(n) for n in HIDE_NAMES]
    hidden = [expect_hide(orc, mlib, oracle(orc, n), m) for n, m in zip(HIDE_NAMES, HIDE_MESSAGES)]
    out = ctx.stego_distortions(files, HIDE_MESSAGES, profile=True)
    for n, f, r, h in zip(HIDE_NAMES, files, out, hidden):
        oracle(orc, n)
        w = align_want(orc, h["mp3"], f, 2304, 4608)
        assert w["scores"] is not None
        check_alignment(n, r, w)
        assert (r["hide_offset"], r["too_long"]) == (h["hide_offset"], h["too_long"]), n


def clear_re_encodes(orc, mlib):
    """name -> the oracle's clear re-encode of every stereo input (what clear_file writes)"""
    return {n: capacity_clear(orc, mlib, n)["mp3"] for n in inputs() if oracle(orc, n) is not None and oracle(orc, n)["channels"] == 2}


def test_model_finds_nothing_forced_where_nothing_was_hidden(mlib, orc):
    """files of this encoder at low bit rates have units with fewer big values than their first bands have lines: the encoder chose the
    books of those regions from lines behind the big values, which the audit does not judge"""
    behind = 0
    for n, mp3 in clear_re_encodes(orc, mlib).items():
        r = M.audit_file(mlib, mp3)
        assert (r["forced"], r["foreign"], r["window_units"], r["verdict"]) == (0, 0, 0, "clean"), (n, r)
        assert r["natural"] + r["empty"] == r["regions"] == len(mlib.scan_stream(mp3)["bits"]), n
        behind += r["empty"]
    assert behind > 200


def check_audits(ctx, mlib, orc):
    names, files = list(inputs()), list(inputs().values())
    out = ctx.table_audits(files, profile=True)
    assert len(out) == len(files)
    for n, f, r in zip(names, files, out):
        if n in V.family_f():
            code = single_error(ctx, lambda: mlib.scan_stream(f))
            assert code in (mlib.E_MALFORMED, mlib.E_UNSUPPORTED) and isinstance(r, mlib.Mp3sError) and r.code == code, (n, r, code)
            continue
        same_audit(r, audit_model(n), n)
        o = oracle(orc, n)
        assert (r["n_frames"], r["channels"], r["sampling_rate"], r["kbps"]) == (o["n_frames"], o["channels"], o["sampling_rate"], o["bit_rate"] // 1000), n


@gpu
def test_table_audits_match_the_model(ctx, mlib, orc):
    check_audits(ctx, mlib, orc)


@gpu
def test_clear_re_encodes_audit_as_clean(ctx, mlib, orc):
    clear = clear_re_encodes(orc, mlib)
    out = ctx.table_audits(list(clear.values()), profile=True)
    for (n, mp3), r in zip(clear.items(), out):
        same_audit(r, M.audit_file(mlib, mp3), n)
        assert (r["forced"], r["foreign"], r["verdict"]) == (0, 0, "clean"), (n, r)


@gpu
def test_table_audit_of_the_hide_re_encode_of_vbr_streams(ctx, mlib, orc):
    names = ["c_per_frame", "d_last_bitrate"]
    files = [stream_bytes(n) for n in names]
    hidden = ctx.hide_messages(files + files, ["audit " + TOO_LONG[:300], "fits: " + TOO_LONG[:20], None, None])
    assert not any(isinstance(h, Exception) for h in hidden)
    out = ctx.table_audits([h["data"] for h in hidden], profile=True)
    for i, (h, r) in enumerate(zip(hidden, out)):
        same_audit(r, M.audit_file(mlib, h["data"]), i)
        assert r["foreign"] == 0 and r["window_units"] == 0, i
        if i < 2:
            assert r["forced"] > 0 and r["verdict"] == "carries", (i, r)
            if not h["too_long"]:
                assert r["last_forced"] + 1 <= h["hide_offset"], (i, r["last_forced"], h["hide_offset"])
        else:
            assert r["forced"] == 0 and r["verdict"] == "clean", (i, r)
    assert not hidden[1]["too_long"]
    for n, h in zip(names, hidden[:2]):                              # (the re-encode is the oracle's, at the last frame's rate and bit rate)
        o = oracle(orc, n)
        assert (h["kbps"], h["sampling_rate"]) == (o["bit_rate"] // 1000, o["sampling_rate"])


@gpu
@pytest.mark.parametrize("opts", OPTIONS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_the_same_answers_under_options(ctx, mlib, orc, opts):
    with options(ctx, **opts):
        check_reveal(ctx, mlib, orc)
        check_capacity(ctx, mlib, orc)
        check_audits(ctx, mlib, orc)
        check_short_pairs(ctx, mlib, orc)
