"""Table audit: does an MP3 file carry a payload, and how much (include/mp3s.h section vi-e) -- mp3s_table_audit_files /
Context.table_audits and the two kernels alone (mp3s_table_audit_dev / Context.table_audit_dev).

The expected values come from tests/table_audit_model.py, the rule restated in numpy over the host-only parse_stream / scan_stream;
it runs no code of the feature.  Every GPU test compares every field, and the per-frame profile, with the model exactly."""
import ctypes as C
import os

import numpy as np
import pytest

import table_audit_model as M

gpu = pytest.mark.gpu

# the model on tests/golden/test.mp3 and on the streams of g7_decode_corpus.npz (run once on the CPU; test_model_literals repeats it):
# regions, natural, forced, forced_ones, foreign, empty, excess_bits, first_forced, last_forced, window_units, n_frames, channels, kbps
LITERALS = {
    "test.mp3": (419, 419, 0, 0, 0, 0, 0, -1, -1, 0, 36, 2, 320),
    "books_4_14_id3": (63, 12, 1, 1, 22, 28, 11, 47, 47, 0, 6, 2, 320),
    "joint_ms_blocks_48": (69, 1, 1, 0, 62, 5, 5, 40, 40, 22, 8, 2, 192),
    "long_reservoir_44": (90, 6, 5, 3, 50, 29, 72, 12, 56, 0, 8, 2, 128),
    "mixed_blocks_44": (48, 0, 0, 0, 44, 4, 0, -1, -1, 20, 6, 2, 224),
    "mono_crc_32": (39, 0, 0, 0, 31, 8, 0, -1, -1, 8, 8, 1, 64),
    "no_reservoir_32k_lowrate": (55, 0, 0, 0, 28, 27, 0, -1, -1, 13, 6, 2, 32),
}
LITERAL_KEYS = M.COUNTERS + ("n_frames", "channels", "kbps")
FIELDS = M.COUNTERS + ("n_frames", "channels", "sampling_rate", "kbps", "payload_bits", "verdict")


def other_encoders(golden_dir):
    g = np.load(os.path.join(golden_dir, "g7_decode_corpus.npz"))
    files = {"test.mp3": open(os.path.join(golden_dir, "test.mp3"), "rb").read()}
    for n in sorted({k.split("__")[0] for k in g.files}):
        files[n] = g[n + "__mp3"].tobytes()
    return files


def same(got, want, where):
    """every field and the profile of an answer of table_audits against the model's"""
    assert not isinstance(got, Exception), (where, got)
    for k in FIELDS:
        assert got[k] == want[k], (where, k, got[k], want[k])
    assert got["profile"].dtype == np.uint32 and np.array_equal(got["profile"], want["profile"]), where


# ------------------------------------------------------------------------------------------------ no device
def test_table_audit_symbols_and_layout(mlib):
    L = mlib.lib()
    for s in ("mp3s_table_audit_dev", "mp3s_table_audit_files"):
        assert hasattr(L, s) and s in mlib.SYMBOLS, s
    want, off = [], 0
    for n in ("regions", "natural", "forced", "forced_ones", "foreign", "empty", "excess_bits", "first_forced", "last_forced"):
        want.append((n, off, 8)); off += 8
    for n in ("n_frames", "channels", "sampling_rate", "kbps", "window_units", "reserved"):
        want.append((n, off, 4)); off += 4
    want.append(("profile", off, C.sizeof(C.c_void_p)))
    got = [(n, getattr(mlib.TableAudit, n).offset, getattr(mlib.TableAudit, n).size) for n, _ in mlib.TableAudit._fields_]
    assert got == want and C.sizeof(mlib.TableAudit) == 96 + C.sizeof(C.c_void_p) == mlib.TABLE_AUDIT_DTYPE.itemsize == 104
    assert [(n, mlib.TABLE_AUDIT_DTYPE.fields[n][1]) for n in mlib.TABLE_AUDIT_DTYPE.names] == [(n, o) for n, o, _ in want]
    assert mlib.TABLE_AUDIT_UNIT_DTYPE.itemsize == 16 and mlib.TABLE_AUDIT_SEG_DTYPE.itemsize == 8
    assert [(n, mlib.TABLE_AUDIT_UNIT_DTYPE.fields[n][1]) for n in mlib.TABLE_AUDIT_UNIT_DTYPE.names] == \
        [("cls", 0), ("forced_bits", 3), ("nat", 4), ("window", 7), ("excess", 8), ("reserved", 14)]
    assert mlib.TABLE_AUDIT_UNIT_DTYPE == M.UNIT_DTYPE
    assert (mlib.TA_NONE, mlib.TA_NATURAL, mlib.TA_FORCED, mlib.TA_FOREIGN, mlib.TA_EMPTY) == (M.NONE, M.NATURAL, M.FORCED, M.FOREIGN, M.EMPTY)
    # the header says the same
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "mp3s.h")).read()
    for decl in ("} mp3s_table_audit_unit; /* 16 bytes */", "} mp3s_table_audit; /* 9 * 8 + 6 * 4 + 8 = 104 bytes */",
                 "int64_t regions, natural, forced, forced_ones, foreign, empty, excess_bits;", "int64_t first_forced, last_forced;",
                 "int32_t n_frames, channels, sampling_rate, kbps, window_units, reserved;", "const uint32_t *profile;",
                 "typedef struct { int32_t first_frame, n_frames; } mp3s_table_audit_seg; /* 8 bytes",
                 "#define MP3S_TA_NATURAL 1", "#define MP3S_TA_FORCED 2", "#define MP3S_TA_FOREIGN 3", "#define MP3S_TA_EMPTY 4"):
        assert decl in txt, decl
    assert "#define MP3S_OPT_COUNT 22" in txt and "#define MP3S_N_KERNELS 9" in txt


def test_table_audit_bad_arguments(mlib):
    """argument checks need no device: a made-up context is never looked into"""
    L = mlib.lib()
    fake = C.c_void_p(64)
    p = C.c_void_p(4096)
    one, lens = (C.c_void_p * 1)(C.addressof(mlib._EMPTY)), (C.c_size_t * 1)(0)
    out, status, owner = (mlib.TableAudit * 1)(), (C.c_int32 * 1)(), C.c_void_p()
    F = L.mp3s_table_audit_files
    assert F(None, one, lens, 1, 0, C.byref(owner), out, status) == mlib.E_ARG
    assert F(fake, None, lens, 1, 0, C.byref(owner), out, status) == mlib.E_ARG
    assert F(fake, one, None, 1, 0, C.byref(owner), out, status) == mlib.E_ARG
    assert F(fake, one, lens, 1, 0, None, out, status) == mlib.E_ARG
    assert F(fake, one, lens, 1, 0, C.byref(owner), None, status) == mlib.E_ARG
    assert F(fake, one, lens, 0, 0, C.byref(owner), out, status) == mlib.E_ARG
    assert F(fake, one, lens, -1, 0, C.byref(owner), out, status) == mlib.E_ARG
    assert not owner.value
    D = L.mp3s_table_audit_dev
    assert D(None, p, p, 1, 2, p, 1, p, p, p) == mlib.E_ARG
    assert D(fake, None, p, 1, 2, p, 1, p, p, p) == mlib.E_ARG
    assert D(fake, p, None, 1, 2, p, 1, p, p, p) == mlib.E_ARG
    assert D(fake, p, p, 1, 2, None, 1, p, p, p) == mlib.E_ARG
    assert D(fake, p, p, 1, 2, p, 1, p, None, p) == mlib.E_ARG
    assert D(fake, p, p, 0, 2, p, 1, p, p, p) == mlib.E_ARG
    assert D(fake, p, p, 1, 2, p, 0, p, p, p) == mlib.E_ARG
    assert D(fake, p, p, 1, 0, p, 1, p, p, p) == mlib.E_ARG
    assert D(fake, p, p, 1, 3, p, 1, p, p, p) == mlib.E_ARG
    assert D(fake, C.c_void_p(4098), p, 1, 2, p, 1, p, p, p) == mlib.E_ARG      # d_is not dword-aligned
    assert D(fake, p, p, 1, 2, p, 1, C.c_void_p(4100), p, p) == mlib.E_ARG      # d_units not 16-byte aligned


def test_model_on_the_reference_made_golden(mlib, golden_dir):
    """g6_synth128.npz: written by the reference itself, 48 frames, 56 message bits"""
    g = np.load(os.path.join(golden_dir, "g6_synth128.npz"))
    r = M.audit_file(mlib, g["mp3"].tobytes())
    assert (r["regions"], r["natural"], r["forced"]) == (540, 514, 26) and r["regions"] == len(g["dec_bits"])
    assert (r["forced"] - r["forced_ones"], r["forced_ones"]) == (16, 10)
    assert (r["first_forced"], r["last_forced"], r["excess_bits"], r["foreign"], r["empty"], r["window_units"]) == (1, 53, 207, 0, 0, 0)
    assert r["payload_bits"] == 54 <= 56 and r["verdict"] == "carries"
    assert (r["n_frames"], r["channels"], r["sampling_rate"], r["kbps"]) == (48, 2, 44100, 128)
    prof = r["profile"].astype(np.int64)
    per = (prof & 15) + ((prof >> 4) & 15) + ((prof >> 8) & 15) + ((prof >> 12) & 15)
    assert int(per.sum()) == 540 and int(((prof >> 4) & 15).sum()) == 26
    start = np.cumsum(per) - per
    assert not ((prof >> 4) & 15)[start >= 56].any()                 # behind the message nothing is forced


def test_model_literals(mlib, golden_dir):
    """the literals the GPU test expects of other encoders' files are what the model gives"""
    files = other_encoders(golden_dir)
    assert sorted(files) == sorted(LITERALS)
    for name, data in files.items():
        r = M.audit_file(mlib, data)
        assert tuple(r[k] for k in LITERAL_KEYS) == LITERALS[name], (name, [r[k] for k in LITERAL_KEYS])
    assert M.audit_file(mlib, files["test.mp3"])["verdict"] == "clean"
    assert all(M.audit_file(mlib, files[n])["verdict"] == "foreign" for n in files if n != "test.mp3")


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def corpus(ctx, mlib, golden_dir):
    """the file list of tests/test_capacity.py's corpus: three (rate, bitrate) groups, 1 .. 260 frames with a silence inside the long one,
    the reference-made golden, 257 and 513 frames (a frame past one tile of k_table_audit_streams, and past two), ten frames of digital
    silence; with the model's answer for each"""
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
    return {"files": files, "model": [M.audit_file(mlib, f) for f in files], "silent": len(files) - 1, "golden": 8}


def hide_messages_list():
    rng = np.random.default_rng(11)
    return ["short", None, "x", "a message that does not fit into five frames " * 40, "", "ab", None, "héllo wörld ✓",
            "".join(chr(int(c)) for c in rng.integers(32, 127, size=400))]


def regions_per_frame(profile):
    p = profile.astype(np.int64)
    return (p & 15) + ((p >> 4) & 15) + ((p >> 8) & 15) + ((p >> 12) & 15)


@gpu
def test_clean_corpus(ctx, mlib, corpus):
    files, want = corpus["files"], corpus["model"]
    out = ctx.table_audits(files, profile=True)
    revealed = ctx.reveal_messages(files)
    assert len(out) == len(files)
    for i, (r, w, v) in enumerate(zip(out, want, revealed)):
        same(r, w, i)
        print(i, r["n_frames"], "frames:", {k: r[k] for k in M.COUNTERS}, r["verdict"])
        assert r["regions"] == len(v["bits"]), (i, r["regions"], len(v["bits"]))
        if i == corpus["golden"]:                                    # the reference-made file carries its 56 bits
            assert (r["regions"], r["natural"], r["forced"], r["forced_ones"], r["first_forced"], r["last_forced"], r["excess_bits"]) == \
                (540, 514, 26, 10, 1, 53, 207) and r["verdict"] == "carries" and r["payload_bits"] == 54
            continue
        assert r["forced"] == 0 and r["foreign"] == 0 and r["verdict"] == "clean" and r["payload_bits"] == 0, (i, r)
        assert r["first_forced"] == -1 and r["last_forced"] == -1 and r["window_units"] == 0 and r["channels"] == 2, i
    assert [r["n_frames"] for r in out[:8]] == [60, 35, 1, 90, 260, 2, 17, 5] and out[9]["n_frames"] == 257 and out[10]["n_frames"] == 513
    assert (out[0]["kbps"], out[0]["sampling_rate"]) == (128, 44100) and (out[3]["kbps"], out[3]["sampling_rate"]) == (64, 32000)
    s = out[corpus["silent"]]
    assert all(s[k] == 0 for k in M.COUNTERS if k not in ("first_forced", "last_forced")) and s["last_forced"] == -1 and not s["profile"].any()
    assert s["n_frames"] == 10
    # without the profile nothing else changes
    plain = ctx.table_audits(files)
    assert all(p["profile"] is None for p in plain)
    assert [[p[k] for k in FIELDS] for p in plain] == [[r[k] for k in FIELDS] for r in out]


@gpu
def test_hidden_messages_are_found(ctx, mlib, corpus):
    # test_capacity.py's message list on its files, and behind it three messages of 64 bits and more that fit: 60, 260 and 90 frames
    rng = np.random.default_rng(12)
    files = corpus["files"][:9] + [corpus["files"][0], corpus["files"][4], corpus["files"][3]]
    msgs = hide_messages_list() + ["a longer message that fits", "".join(chr(int(c)) for c in rng.integers(32, 127, size=200)), "sixty-four bits and a few more"]
    hidden = ctx.hide_messages(files, msgs)
    assert not any(isinstance(h, Exception) for h in hidden)
    stego = [h["data"] for h in hidden]
    out = ctx.table_audits(stego, profile=True)
    fit_long = 0
    for i, (m, h, r) in enumerate(zip(msgs, hidden, out)):
        same(r, M.audit_file(mlib, stego[i]), i)
        print(i, "clear" if m is None else f"{len(mlib.message_frame(m))} bits", "too_long", h["too_long"], {k: r[k] for k in M.COUNTERS}, r["verdict"])
        assert r["foreign"] == 0 and r["window_units"] == 0, i
        if m is None:
            assert r["forced"] == 0 and r["verdict"] == "clean", i
            continue
        n_hide = len(mlib.message_frame(m))
        if h["too_long"]:
            continue
        assert r["last_forced"] < n_hide and r["forced"] <= h["hide_offset"], (i, r["last_forced"], n_hide, r["forced"], h["hide_offset"])
        per = regions_per_frame(r["profile"])
        start = np.cumsum(per) - per                                 # the index of each frame's first region
        assert not ((r["profile"] >> 4) & 15)[start >= n_hide].any(), i
        if n_hide >= 64:
            fit_long += 1
            assert r["forced"] > 0 and r["verdict"] == "carries" and r["payload_bits"] == r["last_forced"] + 1 > 0, (i, r)
    assert fit_long == 3 and hidden[3]["too_long"] and not any(h["too_long"] for h in hidden[9:])


@gpu
def test_raw_bits_without_a_frame_are_found(ctx, mlib):
    from synth_pcm import synth_pcm
    pcm = synth_pcm(30, seed=4100)
    wav = mlib.wav_header(pcm.shape[0], 2, 44100) + np.ascontiguousarray(pcm, dtype="<i2").tobytes()
    raw = np.random.default_rng(4101).integers(0, 2, size=200).astype(np.uint8)
    enc = ctx.encode_files([wav, wav], 128, hide_bits=[raw, None])
    assert not any(isinstance(e, Exception) for e in enc) and not enc[0]["too_long"]
    out = ctx.table_audits([enc[0]["data"], enc[1]["data"]], profile=True)
    for i in (0, 1):
        same(out[i], M.audit_file(mlib, enc[i]["data"]), i)
    r = out[0]
    assert r["forced"] > 0 and r["verdict"] == "carries" and r["last_forced"] < 200 and r["forced"] <= enc[0]["hide_offset"], r
    assert out[1]["forced"] == 0 and out[1]["verdict"] == "clean"
    # what was forced reads back as the hidden bit: the unit records of the stego file
    p, s = mlib.parse_stream(enc[0]["data"]), mlib.scan_stream(enc[0]["data"])
    segs = np.array([(0, p["n_frames"])], dtype=mlib.TABLE_AUDIT_SEG_DTYPE)
    rec, units, _ = ctx.table_audit_dev(p["is"], s["side"], segs, 2)
    assert np.array_equal(units, M.audit_units(p["is"], s["side"], 2)) and int(rec["forced"][0]) == r["forced"]
    idx = 0
    for u in units.reshape(-1):
        for g in range(3):
            if u["cls"][g] == M.NONE:
                continue
            if u["cls"][g] == M.FORCED:
                assert (int(u["forced_bits"]) >> g) & 1 == int(raw[idx]), idx
            idx += 1


@gpu
def test_files_of_other_encoders_and_per_file_status(ctx, mlib, golden_dir, corpus):
    others = other_encoders(golden_dir)
    names = sorted(others)
    good = others["test.mp3"]
    files = [corpus["files"][0]] + [others[n] for n in names] + [b"\xff" * 2000, None, b"not an mp3 file at all" * 10, good[:-1000], corpus["files"][2]]
    out = ctx.table_audits(files, profile=True)
    assert len(out) == len(files)
    same(out[0], corpus["model"][0], "clean file in front")
    same(out[-1], corpus["model"][2], "clean file behind")
    for k, n in enumerate(names):
        r = out[1 + k]
        same(r, M.audit_file(mlib, others[n]), n)
        assert tuple(r[key] for key in LITERAL_KEYS) == LITERALS[n], (n, [r[key] for key in LITERAL_KEYS])
    assert out[1 + names.index("test.mp3")]["verdict"] == "clean" and out[1 + names.index("mono_crc_32")]["channels"] == 1
    assert out[1 + names.index("mixed_blocks_44")]["verdict"] == "foreign" and not mlib.scan_stream(others["mixed_blocks_44"])["gpu_ok"]
    base = 1 + len(names)
    assert isinstance(out[base], mlib.Mp3sError) and out[base].code == mlib.E_MALFORMED
    assert isinstance(out[base + 1], mlib.Mp3sError) and out[base + 1].code == mlib.E_ARG
    nothing = out[base + 2]                                          # no sync: a stream without a frame
    assert not isinstance(nothing, Exception) and nothing["n_frames"] == 0 and nothing["regions"] == 0 and nothing["last_forced"] == -1
    assert nothing["verdict"] == "clean" and nothing["profile"] is None
    same(out[base + 3], M.audit_file(mlib, good[:-1000]), "cut file")
    # status == NULL in the C call: the first failing file fails the call, no owner
    bufs = [np.frombuffer(f, dtype=np.uint8) for f in (files[0], files[base])]
    ptr = (C.c_void_p * 2)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * 2)(*[len(b) for b in bufs])
    res, owner = (mlib.TableAudit * 2)(), C.c_void_p()
    assert mlib.lib().mp3s_table_audit_files(ctx.handle, ptr, lens, 2, 0, C.byref(owner), res, None) == mlib.E_MALFORMED
    assert not owner.value


# ---- the kernels alone on hand-made arrays
# regions whose two candidate books cost the same: (13, 15) below 15 -- the choice is 15 --, (c0, c1) from 15 up -- the choice is c0
TIES = [(0, 1), (15, 0), (16, 0, 1, 12), (31, 3, 0, 0)]


def tie_books(values):
    m = max(values)
    return (13, 15) if m < 15 else (M.first_book(15, 23, m - 15), M.first_book(24, 31, m - 15))


def made_units(mlib, n_frames, nch, seed):
    """side records and samples that reach every branch of the rule; returns (is, side)"""
    T = M.tables()
    rng = np.random.default_rng(seed)
    side = np.zeros(n_frames, dtype=mlib.FRAME_SIDE_DTYPE)
    is_ = np.zeros((n_frames, 2, 2, 576), dtype=np.int16)
    side["nch"] = nch
    side["sr_idx"] = rng.integers(0, 3, size=n_frames)
    maxima = [0, 1, 14, 15, 16, 17, 20, 25, 30, 31, 50, 100, 200, 300, 600, 1039, 3000, 8206]
    for tie in TIES:
        v, (c0, c1) = np.array(tie, dtype=np.int64), tie_books(tie)
        assert M.count_bit(v, c0) == M.count_bit(v, c1), tie
    k = 0
    for f in range(n_frames):
        for ch in range(nch):
            for gr in range(2):
                u = side[f]["unit"][gr][ch]
                spec = is_[f, gr, ch]
                kind = k % 16
                k += 1
                u["big_values"] = [0, 1, 288, 2, 40][kind % 5] if kind < 10 else int(rng.integers(0, 289))
                u["region0_count"], u["region1_count"] = (15, 7) if kind == 3 else (int(rng.integers(0, 16)), int(rng.integers(0, 8)))
                if kind == 5:
                    u["big_values"], u["region0_count"] = 4, 6            # 2 bv below sfb[r0 + 1]: regions 0 and 1 reach behind the big values
                u["window_switching"] = 1 if kind == 7 else 0
                u["block_type"] = 2 if kind == 7 else 0
                bv2 = 2 * min(int(u["big_values"]), 288)
                # values: a spectrum of falling size, every region's maximum pinned to one of the interesting values
                mag = rng.integers(0, 4, size=576) * (rng.random(576) < 0.6)
                spec[:] = mag
                sfb = T["sfb_long"][int(side[f]["sr_idx"])]
                a1 = min(int(sfb[min(int(u["region0_count"]) + 1, 22)]), bv2)
                a2 = min(int(sfb[min(int(u["region0_count"]) + int(u["region1_count"]) + 2, 22)]), bv2)
                for r, (lo, hi) in enumerate([(0, a1), (a1, a2), (a2, bv2)]):
                    if hi <= lo:
                        continue
                    m = maxima[int(rng.integers(0, len(maxima)))]
                    style = int(rng.integers(0, 6))
                    if style == 0:                                   # only the last pair of the region is non-zero
                        spec[lo:hi] = 0
                        spec[hi - 2 + int(rng.integers(0, 2))] = max(m, 1)
                    elif style == 1:                                 # only the first
                        spec[lo:hi] = 0
                        spec[lo + int(rng.integers(0, 2))] = max(m, 1)
                    elif style == 2 and hi - lo >= 4:                # a tie of the two candidates
                        tie = TIES[int(rng.integers(0, len(TIES)))]
                        spec[lo:hi] = 0
                        spec[lo:lo + len(tie)] = tie
                    elif m == 0:
                        spec[lo:hi] = 0
                    else:
                        if m > 3:                                    # a body of mid-sized values under the maximum: books 24.. win there
                            body = rng.integers(0, min(m, 15) + 1, size=hi - lo)
                            spec[lo:hi] = np.where(rng.random(hi - lo) < 0.5, body, spec[lo:hi])
                        spec[lo:hi] = np.minimum(spec[lo:hi], m)
                        spec[lo + int(rng.integers(0, hi - lo))] = m
                spec[bv2:] = rng.integers(0, 2, size=576 - bv2)      # count1 lines: not the audit's business
                spec *= rng.choice(np.array([-1, 1], dtype=np.int16), size=576)
                # books: from the natural choice -- itself, either transform, or anything
                u["table_select"] = 13
                nat = M.audit_unit(spec, u, side[f]["sr_idx"])["nat"]
                for r in range(3):
                    how = int(rng.integers(0, 8))
                    if how <= 1 or not nat[r]:
                        u["table_select"][r] = [0, int(nat[r]) or 13, int(rng.integers(0, 32)), 4][int(rng.integers(0, 4))]
                    else:
                        u["table_select"][r] = int(T["transform"][int(nat[r])][how & 1])
    return is_, side


@gpu
def test_kernels_alone_region_by_region(ctx, mlib):
    lengths = [1, 255, 256, 257]
    n = sum(lengths)
    is_, side = made_units(mlib, n, 2, 77)
    segs = np.zeros(len(lengths), dtype=mlib.TABLE_AUDIT_SEG_DTYPE)
    segs["n_frames"] = lengths
    segs["first_frame"] = np.cumsum([0] + lengths[:-1])
    want_units = M.audit_units(is_, side, 2)
    # the made-up batch reaches what it is meant to reach (a property of the inputs, read off the model)
    T = M.tables()
    flat = want_units.reshape(-1)
    reached = set()
    for u in flat:
        for g in range(3):
            if u["cls"][g] in (M.NATURAL, M.FORCED):
                reached.add((int(u["nat"][g]), int(u["cls"][g]), (int(u["forced_bits"]) >> g) & 1))
    for nat in [13] + list(range(15, 32)):
        for b in (0, 1):
            t = int(T["transform"][nat][b])
            assert ((nat, M.NATURAL, 0) in reached) if t == nat else ((nat, M.FORCED, b) in reached), (nat, b)
    assert {M.NONE, M.NATURAL, M.FORCED, M.FOREIGN, M.EMPTY} <= set(int(c) for c in flat["cls"].reshape(-1)) and flat["window"].any()
    assert (flat["excess"] < 0).any() and (flat["excess"] > 0).any()
    big = np.abs(is_.astype(np.int64)).reshape(n, 4, 576)
    assert big.max() == 8206 and {0, 1, 288} <= set(int(b) for b in side["unit"]["big_values"].reshape(-1))
    out, units, prof = ctx.table_audit_dev(is_, side, segs, 2)
    bad = np.nonzero(units.reshape(-1) != flat)[0]
    assert len(bad) == 0, (len(bad), bad[:5], units.reshape(-1)[bad[:5]], flat[bad[:5]])
    for s, (first, cnt) in enumerate(zip(segs["first_frame"], lengths)):
        w, wp = M.audit_stream(want_units[first:first + cnt])
        for k in M.COUNTERS:
            assert int(out[k][s]) == w[k], (s, k, int(out[k][s]), w[k])
        assert (int(out["n_frames"][s]), int(out["channels"][s]), int(out["sampling_rate"][s]), int(out["kbps"][s]), int(out["reserved"][s]),
                int(out["profile"][s])) == (cnt, 2, 0, 0, 0, 0), s
        assert np.array_equal(prof[first:first + cnt], wp), s
    assert int(out["forced"][1]) > 0 and int(out["first_forced"][2]) >= 0
    # without the unit and profile arrays the stream records are the same
    again, no_units, no_prof = ctx.table_audit_dev(is_, side, segs, 2, units=False, profile=False)
    assert no_units is None and no_prof is None and np.array_equal(again, out)


@gpu
def test_kernels_alone_mono(ctx, mlib):
    """a mono batch: channel 1 of the arrays is noise and is not looked at"""
    n = 70
    is_, side = made_units(mlib, n, 1, 78)
    rng = np.random.default_rng(79)
    is_[:, :, 1, :] = rng.integers(-20, 20, size=(n, 2, 576))
    side["unit"]["table_select"][:, :, 1, :] = rng.integers(0, 32, size=(n, 2, 3))
    side["unit"]["big_values"][:, :, 1] = rng.integers(0, 289, size=(n, 2))
    segs = np.array([(0, 64), (64, 6)], dtype=mlib.TABLE_AUDIT_SEG_DTYPE)
    want_units = M.audit_units(is_, side, 1)
    out, units, prof = ctx.table_audit_dev(is_, side, segs, 1)
    assert np.array_equal(units, want_units) and not units[:, 2:]["cls"].any()
    for s, (first, cnt) in enumerate(segs):
        w, wp = M.audit_stream(want_units[first:first + cnt])
        assert all(int(out[k][s]) == w[k] for k in M.COUNTERS) and int(out["channels"][s]) == 1, s
        assert np.array_equal(prof[first:first + cnt], wp), s
