"""How much fits: the message capacity of lists of MP3 and WAV files (include/mp3s.h section vi-b) -- mp3s_capacity_files,
mp3s_capacity_wavs, k_capacity alone (mp3s_capacity_dev) and the host's mp3s_capacity_text_bytes.

The expected counts run no code of the capacity calls: decode_stream -> int16 -> encode_pcm(...)["gr"], and the sum of n_tables over
the records with MP3S_RF_ACTIVE (flags & 1), per stream; hide_offset / too_long are those of hide_messages / encode_files."""
import ctypes as C
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ no device
def test_capacity_symbols_and_layout(mlib):
    L = mlib.lib()
    for s in ("mp3s_capacity_dev", "mp3s_capacity_files", "mp3s_capacity_wavs", "mp3s_capacity_text_bytes"):
        assert hasattr(L, s) and s in mlib.SYMBOLS, s
    assert mlib.CAPACITY_SEG_DTYPE.itemsize == 16                   # sizeof(mp3s_capacity_seg)
    assert [(n, mlib.CAPACITY_SEG_DTYPE.fields[n][1]) for n in mlib.CAPACITY_SEG_DTYPE.names] == [("bits", 0), ("active_units", 8), ("reserved", 12)]
    # mp3s_capacity as include/mp3s.h declares it: three int64, eight int32, a pointer
    want = [("bits", 0, 8), ("hide_offset", 8, 8), ("text_bytes", 16, 8), ("too_long", 24, 4), ("n_frames", 28, 4), ("kbps", 32, 4),
            ("sampling_rate", 36, 4), ("channels", 40, 4), ("active_units", 44, 4), ("fallback", 48, 4), ("reserved", 52, 4),
            ("profile", 56, C.sizeof(C.c_void_p))]
    got = [(n, getattr(mlib.Capacity, n).offset, getattr(mlib.Capacity, n).size) for n, _ in mlib.Capacity._fields_]
    assert got == want and C.sizeof(mlib.Capacity) == 56 + C.sizeof(C.c_void_p)
    # the header says the same
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "mp3s.h")).read()
    assert "} mp3s_capacity_seg; /* 16 bytes */" in txt
    for decl in ("int64_t bits, hide_offset, text_bytes;", "int32_t too_long, n_frames, kbps, sampling_rate, channels, active_units;",
                 "int32_t fallback;", "const uint32_t *profile;"):
        assert decl in txt, decl
    # argument checks need no device
    assert L.mp3s_capacity_files(None, None, None, 0, None, None, 0, None, None, None) == mlib.E_ARG
    assert L.mp3s_capacity_wavs(None, None, None, 0, None, None, None, 0, None, None, None) == mlib.E_ARG
    assert L.mp3s_capacity_dev(None, None, None, 0, None, None) == mlib.E_ARG


def test_capacity_text_bytes_against_brute_force(mlib):
    """the largest n with len(message_frame("a" * n)) - 1 <= bits, 0 below the size of "0#" -- for bits 0 .. 20000 in steps of 7 and
    around every value where the digit count of n changes"""
    frame = [len(mlib.message_frame("a" * n)) for n in range(0, 20000 // 8 + 8)]      # bits of "<n>#" + n bytes; rises with n
    assert frame[0] == 16 and frame[9] == 88 and frame[10] == 104 and all(a < b for a, b in zip(frame, frame[1:]))
    values = set(range(0, 20001, 7))
    for n in (9, 10, 99, 100, 999, 1000):                            # where n gains a digit: every bit count around the frames of n - 1, n, n + 1
        for m in (n - 1, n, n + 1):
            values.update(range(frame[m] - 4, frame[m] + 3))
    for bits in sorted(values):
        fits = [n for n in range(len(frame)) if frame[n] - 1 <= bits] if bits < 200 else None
        if fits is None:                                             # (the same brute force, from the top: the first n whose frame fits)
            n = min(len(frame) - 1, bits // 8)
            while frame[n] - 1 > bits:
                n -= 1
            want = n
        else:
            want = max(fits) if fits else 0
        assert want < len(frame) - 1
        assert mlib.capacity_text_bytes(bits) == want, (bits, want)
    assert mlib.capacity_text_bytes(14) == 0 and mlib.capacity_text_bytes(15) == 0 and mlib.capacity_text_bytes(22) == 0
    assert mlib.capacity_text_bytes(23) == 1 and mlib.capacity_text_bytes(-5) == 0
    assert mlib.capacity_text_bytes(frame[10] - 2) == 9 and mlib.capacity_text_bytes(frame[10] - 1) == 10


# ------------------------------------------------------------------------------------------------ GPU
def per_frame_bits(gr):
    """records of a stream -> (bits per frame, active units)"""
    act = (gr["flags"] & 1) != 0
    return (gr["n_tables"] * act).reshape(-1, 4).sum(axis=1).astype(np.int64), int(act.sum())


def expect_of(ctx, mp3, hide_bits=None):
    d = ctx.decode_stream(mp3)
    assert d["pcm"].dtype == np.int16
    e = ctx.encode_pcm(d["pcm"], int(d["sampling_rate"]), int(d["bit_rate"]) // 1000, hide_bits)
    per, act = per_frame_bits(e["gr"])
    return {"bits": int(per.sum()), "active_units": act, "profile": np.cumsum(per), "hide_offset": e["hide_offset"], "too_long": e["too_long"]}


def oracle_clear_capacity(orc, mlib, o):
    """o: the oracle's decode of a stereo file -> bits, active_units and the per-frame running sum of the oracle's clear re-encode at the
    last frame's rate and bit rate (what clear_file writes): the non-zero table indices of the units whose 576 lines of mdct_freq are not
    all zero.  The indices are read back from the oracle's MP3 bytes by the host parser; where that parser loses sync behind the first frame
    (at 32 kHz and some bit rates the reference's encoder sets the padding bit without writing the byte, see expect_hide) they are the oracle
    encoder's own records, which the bytes are shown to repeat wherever they can be read.  No code of the capacity calls or of the device runs."""
    from test_vbr_streams import oracle_i16
    e = orc.encode(oracle_i16(o), int(o["sampling_rate"]), int(o["bit_rate"]) // 1000, None)
    assert e["rc"] == 0 and e["n_frames"] == o["n_frames"]
    ts = e["frames"]["gi"]["table_select"]                             # [n][gr][ch][3]
    back = mlib.parse_stream(e["mp3"])
    if back["n_frames"] == e["n_frames"]:
        assert np.array_equal(back["table_select"], ts)
    else:
        assert o["sampling_rate"] == 32000 and np.array_equal(back["table_select"], ts[:back["n_frames"]])
    active = e["mdct_freq"].any(axis=3).transpose(0, 2, 1)               # mdct_freq is [n][ch][gr][576] -> [n][gr][ch]
    per = ((ts != 0).sum(axis=3) * active).reshape(len(ts), -1).sum(axis=1).astype(np.int64)
    return {"bits": int(per.sum()), "active_units": int(active.sum()), "profile": np.cumsum(per), "mp3": e["mp3"]}


@pytest.fixture(scope="module")
def corpus(ctx, golden_dir):
    """the file list of test_hide_messages_batch_matches_oracle_and_single_calls (three (rate, bitrate) groups, 1 .. 260 frames, silence
    over frames 50 .. 70 of the long one), a stream of 257 and one of 513 frames (one frame past a tile of k_capacity, and past two),
    and a file of digital silence; with the clear re-encode's records of each"""
    from synth_pcm import synth_pcm
    files = []
    for i, (rate, kbps, n) in enumerate([(44100, 128, 60), (48000, 192, 35), (44100, 128, 1), (32000, 64, 90),
                                         (44100, 128, 260), (48000, 192, 2), (44100, 128, 17), (32000, 64, 5)]):
        pcm = synth_pcm(n, rate=rate, seed=1000 + i)
        if n > 100:
            pcm[50 * 1152:70 * 1152] = 0
        files.append(bytes(ctx.encode_pcm(pcm, rate, kbps, None)["mp3"]))
    files.append(np.load(os.path.join(golden_dir, "g6_synth128.npz"))["mp3"].tobytes())
    files.append(bytes(ctx.encode_pcm(synth_pcm(257, seed=1100), 44100, 128, None)["mp3"]))
    files.append(bytes(ctx.encode_pcm(synth_pcm(513, rate=48000, seed=1101), 48000, 192, None)["mp3"]))
    files.append(bytes(ctx.encode_pcm(np.zeros((10 * 1152, 2), dtype=np.int16), 44100, 128, None)["mp3"]))
    return {"files": files, "clear": [expect_of(ctx, f) for f in files], "silent": len(files) - 1}


def hide_messages_list():
    rng = np.random.default_rng(11)
    return ["short", None, "x", "a message that does not fit into five frames " * 40, "", "ab", None, "héllo wörld ✓",
            "".join(chr(int(c)) for c in rng.integers(32, 127, size=400))]


@gpu
def test_clear_capacity_matches_the_records(ctx, mlib, corpus):
    files, want = corpus["files"], corpus["clear"]
    out = ctx.capacities(files, profile=True)
    assert len(out) == len(files)
    for i, (r, w) in enumerate(zip(out, want)):
        assert not isinstance(r, Exception), (i, r)
        print(i, r["n_frames"], "frames:", r["bits"], "bits,", r["active_units"], "active units, fallback", r["fallback"])
        assert r["bits"] == w["bits"] and r["active_units"] == w["active_units"], (i, r, w["bits"], w["active_units"])
        assert r["profile"].dtype == np.uint32 and r["n_frames"] == len(w["profile"])
        assert np.array_equal(r["profile"], w["profile"]), i
        assert int(r["profile"][-1]) == r["bits"], i
        assert r["fallback"] == 0 and not r["too_long"] and r["channels"] == 2, i
    assert [r["n_frames"] for r in out[:8]] == [60, 35, 1, 90, 260, 2, 17, 5] and out[9]["n_frames"] == 257 and out[10]["n_frames"] == 513
    assert (out[0]["kbps"], out[0]["sampling_rate"]) == (128, 44100) and (out[3]["kbps"], out[3]["sampling_rate"]) == (64, 32000)
    assert out[4]["active_units"] < 260 * 4                          # the silence of the long one: inactive units
    s = out[corpus["silent"]]
    assert s["bits"] == 0 and s["active_units"] == 0 and s["text_bytes"] == 0 and not s["profile"].any()
    # without the profile nothing else changes
    plain = ctx.capacities(files)
    assert all(p["profile"] is None for p in plain)
    assert [(p["bits"], p["active_units"], p["fallback"]) for p in plain] == [(r["bits"], r["active_units"], r["fallback"]) for r in out]
    del out
    assert int(plain[0]["bits"]) == want[0]["bits"]


@gpu
def test_capacity_with_messages_is_the_hide_call_without_its_file(ctx, mlib, corpus):
    files, msgs = corpus["files"][:9], hide_messages_list()
    hidden = ctx.hide_messages(files, msgs)
    out = ctx.capacities(files, msgs, profile=True)
    some_too_long = 0
    for i, (f, m, h, r) in enumerate(zip(files, msgs, hidden, out)):
        assert not isinstance(r, Exception) and not isinstance(h, Exception), (i, r, h)
        print(i, "message" if m is not None else "clear", "bits", r["bits"], "hide_offset", r["hide_offset"], "too_long", r["too_long"], "fallback", r["fallback"])
        assert r["hide_offset"] == h["hide_offset"] and r["too_long"] == h["too_long"], (i, r, h["hide_offset"], h["too_long"])
        assert (r["n_frames"], r["kbps"], r["sampling_rate"], r["channels"]) == (h["n_frames"], h["kbps"], h["sampling_rate"], h["channels"]), i
        assert r["fallback"] in (0, 1)
        if m is None:                                                # a clear entry inside a list with messages
            w = corpus["clear"][i]
        else:                                                        # the count of THAT encode
            w = expect_of(ctx, f, np.array(mlib.message_frame(m), dtype=np.uint8))
            assert (w["hide_offset"], w["too_long"]) == (h["hide_offset"], h["too_long"]), i
        assert r["bits"] == w["bits"] and r["active_units"] == w["active_units"] and np.array_equal(r["profile"], w["profile"]), i
        if r["too_long"]:
            some_too_long += 1
            assert r["bits"] == r["hide_offset"], i
    assert out[3]["too_long"] and not out[0]["too_long"] and some_too_long >= 1


@gpu
def test_text_bytes_is_the_clear_estimate_in_bytes(ctx, mlib, corpus):
    """on the clear estimate's own terms: the field is capacity_text_bytes of the bits (no claim that a message of that length fits
    once it is hidden)"""
    out = ctx.capacities([corpus["files"][i] for i in (0, 3, 5)])
    for r in out:
        assert r["text_bytes"] == mlib.capacity_text_bytes(r["bits"]) and r["text_bytes"] > 0


@gpu
def test_capacity_reports_each_file(ctx, mlib, orc, golden_dir):
    from synth_pcm import synth_pcm
    g = np.load(os.path.join(golden_dir, "g7_decode_corpus.npz"))
    names = sorted({k.split("__")[0] for k in g.files})
    good = bytes(ctx.encode_pcm(synth_pcm(12, seed=5), 44100, 128, None)["mp3"])
    files = [good, b"", b"not an mp3 file at all" * 10, good[:-1000], good] + [g[n + "__mp3"].tobytes() for n in names]
    out = ctx.capacities(files)
    refused = by_oracle = 0
    for i, (f, r) in enumerate(zip(files, out)):
        try:
            single = ctx.clear_file(f)
        except mlib.Mp3sError as e:
            assert isinstance(r, mlib.Mp3sError) and r.code == e.code, (i, r, e)
            refused += 1
            continue
        assert not isinstance(r, Exception), (i, r)
        assert (r["n_frames"], r["kbps"], r["sampling_rate"], r["channels"]) == (single["n_frames"], single["kbps"], single["sampling_rate"], single["channels"]), i
        assert r["fallback"] in (0, 1) and r["text_bytes"] == mlib.capacity_text_bytes(r["bits"]), i
        if i in (0, 4) or i >= 5:                                    # the whole files: the count of the oracle's clear re-encode of the oracle's decode
            o = orc.decode(f)
            assert o["rc"] == 0, i
            w = oracle_clear_capacity(orc, mlib, o)
            assert (r["bits"], r["active_units"]) == (w["bits"], w["active_units"]), (i, r["bits"], w["bits"], r["active_units"], w["active_units"])
            by_oracle += 1
        else:
            assert r["bits"] >= 0, i
    assert by_oracle == 2 + 5                                        # (the g7 corpus without its mono stream)
    assert isinstance(out[1], mlib.Mp3sError) and isinstance(out[2], mlib.Mp3sError) and refused >= 3
    assert not isinstance(out[0], Exception) and not isinstance(out[3], Exception) and out[0]["bits"] == out[4]["bits"] > 0
    # status == NULL in the C call: the first failing file fails the call, no owner
    L = mlib.lib()
    bufs = [np.frombuffer(f, dtype=np.uint8) for f in files[:3]]
    ptr = (C.c_void_p * 3)(*[b.ctypes.data if len(b) else C.addressof(mlib._EMPTY) for b in bufs])
    lens = (C.c_size_t * 3)(*[len(b) for b in bufs])
    res, owner = (mlib.Capacity * 3)(), C.c_void_p()
    assert L.mp3s_capacity_files(ctx.handle, ptr, lens, 3, None, None, 0, C.byref(owner), res, None) == out[1].code
    assert not owner.value


def wav_of(mlib, pcm, rate, nch=2):
    return mlib.wav_header(pcm.shape[0], nch, rate) + np.ascontiguousarray(pcm, dtype="<i2").tobytes()


@gpu
def test_wav_capacity_matches_the_records_and_encode_files(ctx, mlib):
    from synth_pcm import synth_pcm
    shapes = [(1, 44100, 128), (3, 48000, 192), (40, 44100, 128), (3, 44100, 192), (40, 48000, 128), (1, 48000, 192)]
    pcms = [synth_pcm(n, rate=rate, seed=2000 + i) for i, (n, rate, _) in enumerate(shapes)]
    wavs = [wav_of(mlib, p, rate) for p, (_, rate, _) in zip(pcms, shapes)]
    kbps = [k for _, _, k in shapes]
    out = ctx.wav_capacities(wavs, kbps, profile=True)
    for i, (r, p, (n, rate, k)) in enumerate(zip(out, pcms, shapes)):
        assert not isinstance(r, Exception), (i, r)
        per, act = per_frame_bits(ctx.encode_pcm(p, rate, k, None)["gr"])
        assert (r["bits"], r["active_units"]) == (int(per.sum()), act) and np.array_equal(r["profile"], np.cumsum(per)), i
        assert (r["n_frames"], r["kbps"], r["sampling_rate"], r["channels"], r["fallback"]) == (n, k, rate, 2, 0), i
        assert r["text_bytes"] == mlib.capacity_text_bytes(r["bits"])
    # with messages: hide_offset / too_long are encode_files'
    msgs = ["a", None, "fits into forty frames", "does not fit into three frames " * 20, "", "q" * 30]
    enc = ctx.encode_files(wavs, kbps, messages=msgs)
    got = ctx.wav_capacities(wavs, kbps, messages=msgs)
    for i, (e, r) in enumerate(zip(enc, got)):
        assert not isinstance(r, Exception) and not isinstance(e, Exception), (i, r, e)
        assert (r["hide_offset"], r["too_long"], r["n_frames"]) == (e["hide_offset"], e["too_long"], e["n_frames"]), (i, r)
        if r["too_long"]:
            assert r["bits"] == r["hide_offset"], i
    assert got[3]["too_long"] and not got[2]["too_long"] and got[1]["bits"] == out[1]["bits"]
    # a mono file gets the code encode_files gives it; the file beside it is served
    mono = wav_of(mlib, pcms[1][:, :1], 48000, nch=1)
    e = ctx.encode_files([mono, wavs[0]], [128, 128])
    r = ctx.wav_capacities([mono, wavs[0]], [128, 128])
    assert isinstance(e[0], mlib.Mp3sError) and isinstance(r[0], mlib.Mp3sError) and r[0].code == e[0].code
    assert not isinstance(r[1], Exception) and r[1]["bits"] == out[0]["bits"]


@gpu
@pytest.mark.parametrize("option", ["wav_import", "wav_resample"])
def test_wav_capacity_under_the_readers_options(mlib, option):
    """a mono 8-bit file under wav_import, a 22 050 Hz file under wav_resample = 1: the same reader as encode_files on the same context
    -- compared through the hide_offset of a message that is too long"""
    import wav_import_files as W
    from synth_pcm import synth_pcm
    pcm = synth_pcm(6, seed=3000)
    if option == "wav_import":
        wav = W.wav_file((pcm[:5000, 0].astype(np.int64) >> 8) + 128, W.U8, rate=44100)
    else:
        wav = W.wav_file(pcm[:5000].astype(np.int64), W.S16, rate=22050)
    msg = "z" * 400
    c = mlib.Context(0)
    try:
        c.set_option(option, 1)
        e = c.encode_files([wav], 128, messages=[msg])[0]
        r = c.wav_capacities([wav], 128, messages=[msg], profile=True)[0]
        clear = c.wav_capacities([wav], 128)[0]
    finally:
        c.close()
    assert not isinstance(e, Exception) and not isinstance(r, Exception) and not isinstance(clear, Exception), (e, r, clear)
    assert e["too_long"] and r["too_long"] and r["hide_offset"] == e["hide_offset"] == r["bits"] > 0
    assert (r["n_frames"], r["kbps"], r["sampling_rate"], r["channels"]) == (e["n_frames"], e["kbps"], e["sampling_rate"], e["channels"])
    assert int(r["profile"][-1]) == r["bits"] and clear["bits"] > 0 and clear["n_frames"] == e["n_frames"]


@gpu
def test_capacity_kernel_alone(ctx, mlib):
    """hand-made records: flags with and without bit 0 and other bits at random, n_tables 0 .. 3, every other field noise; segments of
    0, 1, 255, 256, 257 and 600 frames back to back"""
    rng = np.random.default_rng(2024)
    lengths = [0, 1, 255, 256, 257, 600]
    n = sum(lengths)
    gr = np.frombuffer(rng.integers(-2 ** 31, 2 ** 31, size=n * 4 * 18, dtype=np.int64).astype("<i4").tobytes(), dtype=mlib.GR_OUT_DTYPE).copy()
    gr["n_tables"] = rng.integers(0, 4, size=n * 4)
    gr["flags"] = (rng.integers(0, 16, size=n * 4) << 1) | rng.integers(0, 2, size=n * 4)
    segs = np.zeros(len(lengths), dtype=mlib.CHAIN_SEG_DTYPE)
    segs["n_frames"] = lengths
    segs["first_frame"] = np.cumsum([0] + lengths[:-1])
    segs["hide_base"] = rng.integers(0, 1000, size=len(lengths))    # (not read)
    out, prof = ctx.capacity_dev(gr, segs, profile=True)
    per, _ = per_frame_bits(gr)
    act = ((gr["flags"] & 1) != 0).reshape(-1, 4).sum(axis=1)
    assert (gr["flags"] & 1).min() == 0 and (gr["flags"] & 1).max() == 1 and (gr["flags"] >> 1).max() > 0
    for s, (first, cnt) in enumerate(zip(segs["first_frame"], lengths)):
        assert int(out["bits"][s]) == int(per[first:first + cnt].sum()), s
        assert int(out["active_units"][s]) == int(act[first:first + cnt].sum()) and int(out["reserved"][s]) == 0, s
        assert np.array_equal(prof[first:first + cnt], np.cumsum(per[first:first + cnt])), s
    assert int(out["bits"][0]) == 0 and int(out["bits"][5]) > 0
    # without a profile array the records are the same
    again, none = ctx.capacity_dev(gr, segs, profile=False)
    assert none is None and np.array_equal(again, out)
