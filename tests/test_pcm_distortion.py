"""What hiding changed: the exact PCM difference of MP3 file pairs (include/mp3s.h section vi-c) -- mp3s_pcm_distortion_files, the two
kernels alone (mp3s_pcm_diff_dev) and the facade's hide_distortions.

The expected values run no code of the new calls: hand-made int16 arrays for the kernels, decode_streams of both lists for the files,
and numpy in int64 for the sums.  Every integer is compared exactly."""
import ctypes as C
import math
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu
NO_DIFF = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------ no device
def test_distortion_symbols_and_layout(mlib):
    L = mlib.lib()
    for s in ("mp3s_pcm_diff_dev", "mp3s_pcm_distortion_files"):
        assert hasattr(L, s) and s in mlib.SYMBOLS, s
    assert (mlib.PCM_PAIR_DTYPE.itemsize, mlib.PCM_FRAME_DIFF_DTYPE.itemsize, mlib.PCM_PAIR_DIFF_DTYPE.itemsize) == (16, 32, 40)
    assert (C.sizeof(mlib.PcmPair), C.sizeof(mlib.PcmFrameDiff), C.sizeof(mlib.PcmPairDiff)) == (16, 32, 40)
    want = {mlib.PCM_PAIR_DTYPE: [("a_first", 0), ("b_first", 4), ("n_frames", 8), ("out_first", 12)],
            mlib.PCM_FRAME_DIFF_DTYPE: [("err2", 0), ("sig2", 8), ("max_abs", 16), ("n_diff", 20), ("first_diff", 24), ("reserved", 28)],
            mlib.PCM_PAIR_DIFF_DTYPE: [("err2", 0), ("sig2", 8), ("n_diff", 16), ("first_diff", 24), ("max_abs", 32), ("reserved", 36)]}
    for dt, fields in want.items():
        assert [(n, dt.fields[n][1]) for n in dt.names] == fields
    for st, dt in ((mlib.PcmPair, mlib.PCM_PAIR_DTYPE), (mlib.PcmFrameDiff, mlib.PCM_FRAME_DIFF_DTYPE), (mlib.PcmPairDiff, mlib.PCM_PAIR_DIFF_DTYPE)):
        assert [(n, getattr(st, n).offset, getattr(st, n).size) for n, _ in st._fields_] == [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names]
    assert mlib.PCM_PAIR_DIFF_DTYPE.fields["first_diff"][0] == np.dtype("<i8") and mlib.PCM_FRAME_DIFF_DTYPE.fields["first_diff"][0] == np.dtype("<u4")
    # mp3s_pcm_distortion as include/mp3s.h declares it: two uint64, five int64, uint32 + three int32, two doubles, a pointer
    want = [("err2", 0, 8), ("sig2", 8, 8), ("n_samples", 16, 8), ("n_diff", 24, 8), ("first_diff", 32, 8), ("rows_a", 40, 8), ("rows_b", 48, 8),
            ("max_abs", 56, 4), ("channels", 60, 4), ("sampling_rate", 64, 4), ("n_frames", 68, 4), ("snr_db", 72, 8), ("psnr_db", 80, 8),
            ("profile", 88, C.sizeof(C.c_void_p))]
    got = [(n, getattr(mlib.PcmDistortion, n).offset, getattr(mlib.PcmDistortion, n).size) for n, _ in mlib.PcmDistortion._fields_]
    assert got == want and C.sizeof(mlib.PcmDistortion) == 88 + C.sizeof(C.c_void_p)
    # the header says the same
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "mp3s.h")).read()
    for decl in ("typedef struct { uint32_t a_first, b_first, n_frames, out_first; } mp3s_pcm_pair;",
                 "typedef struct { uint64_t err2, sig2; uint32_t max_abs, n_diff, first_diff, reserved; } mp3s_pcm_frame_diff;   /* 32 bytes */",
                 "typedef struct { uint64_t err2, sig2, n_diff; int64_t first_diff; uint32_t max_abs, reserved; } mp3s_pcm_pair_diff; /* 40 bytes */",
                 "uint64_t err2, sig2; int64_t n_samples, n_diff, first_diff, rows_a, rows_b;",
                 "uint32_t max_abs; int32_t channels, sampling_rate, n_frames;", "double snr_db, psnr_db;", "const mp3s_pcm_frame_diff *profile;",
                 "(vi-c) what hiding changed"):
        assert decl in txt, decl
    assert txt.index("(vi-b) how much fits") < txt.index("(vi-c) what hiding changed") < txt.index("(vii) asynchronous host-fed pipeline")


def test_distortion_argument_checks_need_no_device(mlib):
    L = mlib.lib()
    assert L.mp3s_pcm_diff_dev(None, None, 2, None, None, 1, None, None) == mlib.E_ARG
    assert L.mp3s_pcm_distortion_files(None, None, None, None, None, 0, 0, None, None, None) == mlib.E_ARG
    # the range checks come before anything is touched: stand-ins for the context and the arrays (never read)
    mem = C.create_string_buffer(4096)
    p = (C.addressof(mem) + 255) & ~255
    pair = np.zeros(1, dtype=mlib.PCM_PAIR_DTYPE)
    for k in range(8):                                               # every pointer in turn
        args = [p, p, 2, p, pair.ctypes.data, 1, p, p]
        if k in (2, 5):
            continue
        args[k] = None
        assert L.mp3s_pcm_diff_dev(*args) == mlib.E_ARG, k
    assert L.mp3s_pcm_diff_dev(p, p, 2, p, pair.ctypes.data, 0, p, p) == mlib.E_ARG
    assert L.mp3s_pcm_diff_dev(p, p, 2, p, pair.ctypes.data, -3, p, p) == mlib.E_ARG
    for nch in (0, 3, -1):
        assert L.mp3s_pcm_diff_dev(p, p, nch, p, pair.ctypes.data, 1, p, p) == mlib.E_ARG
        assert b"nch" in L.mp3s_last_error()
    assert L.mp3s_pcm_diff_dev(p, p + 8, 2, p, pair.ctypes.data, 1, p, p) == mlib.E_ARG      # a lane loads 16 aligned bytes
    for k in (0, 1, 2, 3, 4, 7, 8):
        args = [p, p, p, p, p, 1, 0, C.cast(p, C.POINTER(C.c_void_p)), p, None]
        args[k] = None
        assert L.mp3s_pcm_distortion_files(*args) == mlib.E_ARG, k
    assert L.mp3s_pcm_distortion_files(p, p, p, p, p, 0, 0, C.cast(p, C.POINTER(C.c_void_p)), p, None) == mlib.E_ARG
    assert L.mp3s_pcm_distortion_files(p, p, p, p, p, -1, 0, C.cast(p, C.POINTER(C.c_void_p)), p, None) == mlib.E_ARG


# ------------------------------------------------------------------------------------------------ numpy's side
def frame_records(a, b, per_frame):
    """int16 arrays of whole frames, flattened -> the records of their frames (PCM_FRAME_DIFF fields as int64 / uint64 columns)"""
    a = np.asarray(a).astype(np.int64).reshape(-1, per_frame)
    b = np.asarray(b).astype(np.int64).reshape(-1, per_frame)
    d = a - b
    ne = d != 0
    first = np.where(ne.any(axis=1), ne.argmax(axis=1), NO_DIFF)
    return {"err2": (d * d).sum(axis=1), "sig2": (a * a).sum(axis=1), "max_abs": np.abs(d).max(axis=1) if len(d) else np.zeros(0, np.int64),
            "n_diff": ne.sum(axis=1), "first_diff": first}


def pair_record(fr, per_frame):
    n = len(fr["err2"])
    hit = np.nonzero(fr["first_diff"] != NO_DIFF)[0]
    return {"err2": int(fr["err2"].sum()), "sig2": int(fr["sig2"].sum()), "n_diff": int(fr["n_diff"].sum()),
            "max_abs": int(fr["max_abs"].max()) if n else 0,
            "first_diff": int(hit[0]) * per_frame + int(fr["first_diff"][hit[0]]) if len(hit) else -1}


def ratios(err2, sig2, n_samples):
    if err2 == 0:
        return math.inf, math.inf
    return 10 * math.log10(sig2 / err2), 10 * math.log10(32767 * 32767 * n_samples / err2)


def same_ratio(got, want):
    return got == want if math.isinf(want) or math.isinf(got) else abs(got - want) <= 1e-12 * abs(want)


# ------------------------------------------------------------------------------------------------ GPU, the kernels alone
@gpu
@pytest.mark.parametrize("nch", [1, 2])
def test_pcm_diff_kernels_alone(ctx, mlib, nch):
    """one buffer, the runs of all pairs scrambled over it (A and B of a pair apart, out_first not monotone): identical frames, both
    extremes of d over a full frame, a single differing sample at the very first and at the very last index, random pairs of 1, 2, 5,
    257 and 513 frames (one frame past one and two tiles of pass 2), a pair of 0 frames"""
    rng = np.random.default_rng(77 + nch)
    per = 1152 * nch

    def noise(n):
        x = rng.integers(-32768, 32768, size=n * per, dtype=np.int64).astype(np.int16)
        if n:
            x[rng.integers(0, len(x), size=4)] = [-32768, 32767, -32768, 32767]
        return x
    cases = []                                                       # (name, A, B)
    same = noise(3)
    cases.append(("identical", same, same.copy()))
    cases.append(("lowest against highest", np.full(per, -32768, np.int16), np.full(per, 32767, np.int16)))
    cases.append(("highest against lowest", np.full(per, 32767, np.int16), np.full(per, -32768, np.int16)))
    x = noise(3)
    y = x.copy()
    y[0] = np.int16(-5) if x[0] >= 0 else np.int16(9)
    cases.append(("first sample", x, y))
    x = noise(3)
    y = x.copy()
    y[-1] = np.int16(-7) if x[-1] >= 0 else np.int16(11)
    cases.append(("last sample", x, y))
    for n in (1, 2, 5, 257, 513):
        cases.append((f"random {n}", noise(n), noise(n)))
    cases.append(("no frame", noise(0), noise(0)))
    n_pairs = len(cases)
    # the runs in the buffer: all A in a shuffled order, then all B in another; the frame records in a third
    order_a, order_out = rng.permutation(n_pairs), rng.permutation(n_pairs)
    order_b = np.roll(order_a, -3)                                   # (the last run of A and the first of B belong to different pairs)
    pairs = np.zeros(n_pairs, dtype=mlib.PCM_PAIR_DTYPE)
    chunks, at = [], 0
    for which, order in (("a_first", order_a), ("b_first", order_b)):
        for k in order:
            run = cases[k][1 if which == "a_first" else 2]
            pairs[which][k] = at
            chunks.append(run)
            at += len(run) // per
    pcm = np.concatenate(chunks)
    assert pcm.nbytes < 10_000_000 and at == len(pcm) // per
    out_at = 0
    for k in order_out:
        pairs["n_frames"][k] = len(cases[k][1]) // per
        pairs["out_first"][k] = out_at
        out_at += len(cases[k][1]) // per
    with_frames = pairs["n_frames"] > 0
    assert (np.diff(pairs["out_first"][with_frames].astype(np.int64)) < 0).any(), "out_first is monotone"
    assert (pairs["a_first"][with_frames] + pairs["n_frames"][with_frames] != pairs["b_first"][with_frames]).all(), "A and B of a pair are adjacent"
    frames, got = ctx.pcm_diff_dev(pcm, pairs, nch)
    assert len(frames) == out_at and len(got) == n_pairs
    for k, (name, a, b) in enumerate(cases):
        fr = frame_records(a, b, per)
        want = pair_record(fr, per)
        n, first = int(pairs["n_frames"][k]), int(pairs["out_first"][k])
        print(nch, name, want, {f: int(got[f][k]) for f in got.dtype.names})
        for f in ("err2", "sig2", "max_abs", "n_diff", "first_diff"):
            assert np.array_equal(frames[f][first:first + n].astype(np.int64), fr[f].astype(np.int64)), (name, f)
            assert int(got[f][k]) == want[f], (name, f, int(got[f][k]), want[f])
        assert not frames["reserved"][first:first + n].any() and int(got["reserved"][k]) == 0, name
    by = {name: k for k, (name, _, _) in enumerate(cases)}
    k = by["identical"]
    assert (int(got["err2"][k]), int(got["n_diff"][k]), int(got["max_abs"][k]), int(got["first_diff"][k])) == (0, 0, 0, -1) and int(got["sig2"][k]) > 0
    assert (frames["first_diff"][pairs["out_first"][k]:pairs["out_first"][k] + 3] == NO_DIFF).all()
    for name, s in (("lowest against highest", 32768), ("highest against lowest", 32767)):
        k = by[name]
        assert int(got["err2"][k]) == per * 65535 ** 2 and int(got["sig2"][k]) == per * s * s, name       # (2304 * 65535^2 for stereo: past 2^32 in a lane, past 2^31 in d^2)
        assert (int(got["max_abs"][k]), int(got["n_diff"][k]), int(got["first_diff"][k])) == (65535, per, 0), name
    assert int(got["first_diff"][by["first sample"]]) == 0 and int(got["n_diff"][by["first sample"]]) == 1
    assert int(got["first_diff"][by["last sample"]]) == 3 * per - 1 and int(got["n_diff"][by["last sample"]]) == 1
    assert int(frames["first_diff"][pairs["out_first"][by["last sample"]] + 2]) == per - 1
    k = by["no frame"]
    assert [int(got[f][k]) for f in got.dtype.names] == [0, 0, 0, -1, 0, 0]


# ------------------------------------------------------------------------------------------------ GPU, files
def expect_pairs(ctx, files_a, files_b):
    """per pair the fields of mp3s_pcm_distortion from decode_streams of both lists + numpy (None where a file does not decode)"""
    da, db = ctx.decode_streams(files_a, per_file=True), ctx.decode_streams(files_b, per_file=True)
    out = []
    for x, y in zip(da, db):
        if isinstance(x, Exception) or isinstance(y, Exception) or x["channels"] != y["channels"]:
            out.append(None)
            continue
        nch = x["channels"]
        per = 1152 * nch
        rows = min(len(x["pcm"]), len(y["pcm"]))
        assert rows % 1152 == 0
        fr = frame_records(x["pcm"][:rows].reshape(-1), y["pcm"][:rows].reshape(-1), per)
        w = pair_record(fr, per)
        w.update(profile=fr, n_frames=rows // 1152, n_samples=rows * nch, rows_a=len(x["pcm"]), rows_b=len(y["pcm"]), channels=nch,
                 sampling_rate=x["sampling_rate"])
        w["snr_db"], w["psnr_db"] = ratios(w["err2"], w["sig2"], w["n_samples"])
        out.append(w)
    return out


def check_pair(i, r, w, profile=True):
    assert not isinstance(r, Exception), (i, r)
    print(i, {k: v for k, v in r.items() if k != "profile"})
    for f in ("err2", "sig2", "n_diff", "first_diff", "max_abs", "n_frames", "n_samples", "rows_a", "rows_b", "channels", "sampling_rate"):
        assert int(r[f]) == int(w[f]), (i, f, r[f], w[f])
    assert same_ratio(r["snr_db"], w["snr_db"]) and same_ratio(r["psnr_db"], w["psnr_db"]), (i, r["snr_db"], w["snr_db"], r["psnr_db"], w["psnr_db"])
    if not profile:
        assert r["profile"] is None
        return
    from mp3stego import _lib                                        # (the module the mlib fixture hands out)
    assert r["profile"].dtype == _lib.PCM_FRAME_DIFF_DTYPE and len(r["profile"]) == w["n_frames"], i
    for f in ("err2", "sig2", "max_abs", "n_diff", "first_diff"):
        assert np.array_equal(r["profile"][f].astype(np.int64), w["profile"][f].astype(np.int64)), (i, f)
    assert not r["profile"]["reserved"].any(), i


def corpus_messages():
    rng = np.random.default_rng(11)
    return ["short", None, "x", "a message that does not fit into five frames " * 40, "", "ab", None, "héllo wörld ✓",
            "".join(chr(int(c)) for c in rng.integers(32, 127, size=400)), "m" * 50, None, "hidden in silence"]


@pytest.fixture(scope="module")
def corpus(ctx, golden_dir):
    """the file list of tests/test_capacity.py (three (rate, bitrate) groups of 1 .. 260 frames, the 257- and the 513-frame stream, the
    silent file), its clear and its hide re-encode, and numpy's answer for that pair of lists"""
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
    msgs = corpus_messages()
    assert len(msgs) == len(files)
    clear, hidden = ctx.hide_messages(files, [None] * len(files)), ctx.hide_messages(files, msgs)
    assert not any(isinstance(x, Exception) for x in clear + hidden)
    a, b = [x["data"] for x in hidden], [x["data"] for x in clear]
    return {"files": files, "msgs": msgs, "clear": clear, "hidden": hidden, "a": a, "b": b, "want": expect_pairs(ctx, a, b)}


@gpu
def test_hide_against_clear_matches_numpy(ctx, mlib, corpus):
    want, msgs = corpus["want"], corpus["msgs"]
    # judged on numpy's side: something was changed somewhere, and nothing where nothing was hidden
    assert any(w["err2"] > 0 for w in want), "no message changed a sample: longer messages are needed"
    assert any(m is None and w["err2"] == 0 for m, w in zip(msgs, want))
    assert all(w["err2"] == 0 for m, w in zip(msgs, want) if m is None)
    out = ctx.pcm_distortions(corpus["a"], corpus["b"], profile=True)
    assert len(out) == len(want)
    for i, (r, w) in enumerate(zip(out, want)):
        check_pair(i, r, w)
    assert [r["n_frames"] for r in out[:8]] == [60, 35, 1, 90, 260, 2, 17, 5] and out[9]["n_frames"] == 257 and out[10]["n_frames"] == 513
    assert all(r["rows_a"] == r["rows_b"] == 1152 * r["n_frames"] and r["channels"] == 2 for r in out)
    changed = [r for r in out if r["err2"]]
    assert changed and all(math.isfinite(r["snr_db"]) and r["psnr_db"] > r["snr_db"] and 0 <= r["first_diff"] < r["n_samples"] for r in changed)
    assert all(math.isinf(r["snr_db"]) and math.isinf(r["psnr_db"]) and r["first_diff"] == -1 and r["max_abs"] == 0 for r in out if not r["err2"])
    # without the profile nothing else changes
    plain = ctx.pcm_distortions(corpus["a"], corpus["b"])
    for i, (r, w) in enumerate(zip(plain, want)):
        check_pair(i, r, w, profile=False)
    del out
    assert int(plain[0]["err2"]) == want[0]["err2"]


@gpu
def test_a_file_against_itself(ctx, mlib, corpus):
    files = corpus["files"][:4]
    for r in ctx.pcm_distortions(files, files, profile=True):
        assert not isinstance(r, Exception), r
        assert (r["err2"], r["n_diff"], r["max_abs"], r["first_diff"]) == (0, 0, 0, -1) and r["sig2"] > 0
        assert math.isinf(r["snr_db"]) and r["snr_db"] > 0 and math.isinf(r["psnr_db"]) and r["psnr_db"] > 0
        assert (r["profile"]["first_diff"] == NO_DIFF).all() and not r["profile"]["err2"].any()


def mono_streams():
    import frame_synth as F
    kw = F.CORPUS["mono_crc_32"]
    return F.make_stream(**kw), F.make_stream(**dict(kw, seed=kw["seed"] + 100))


@gpu
def test_mono_and_stereo_pairs_in_one_call(ctx, mlib, corpus):
    """two groups in one call: the mono stream against itself and against a stream of other content, between stereo pairs"""
    mono, other = mono_streams()
    a = [corpus["a"][0], mono, corpus["a"][5], mono, other]
    b = [corpus["b"][0], mono, corpus["b"][5], other, mono]
    want = expect_pairs(ctx, a, b)
    assert [w["channels"] for w in want] == [2, 1, 2, 1, 1] and want[3]["err2"] > 0 and want[1]["err2"] == 0
    out = ctx.pcm_distortions(a, b, profile=True)
    for i, (r, w) in enumerate(zip(out, want)):
        check_pair(i, r, w)
    assert out[1]["n_samples"] == out[1]["n_frames"] * 1152 and out[1]["sampling_rate"] == 32000
    assert out[3]["err2"] == want[3]["err2"] > 0 and out[3]["max_abs"] == out[4]["max_abs"] and out[3]["err2"] == out[4]["err2"]


@gpu
def test_every_failing_pair_gets_its_code(ctx, mlib, corpus):
    mono, _ = mono_streams()
    f44, f48 = corpus["files"][0], corpus["files"][1]
    garbage, no_sync = b"\xff\xfb\x90", b"not an mp3 file at all" * 10   # a sync with no header behind it: refused; no sync at all: a stream of 0 frames
    a = [corpus["a"][0], mono, f44, garbage, corpus["a"][3], f44, no_sync]
    b = [corpus["b"][0], f44, f48, f44, corpus["b"][3], garbage, f44]
    dec = ctx.decode_streams([garbage, f44, no_sync], per_file=True)
    assert isinstance(dec[0], mlib.Mp3sError) and not isinstance(dec[1], Exception) and dec[2]["n_frames"] == 0 and len(dec[2]["pcm"]) == 0
    out = ctx.pcm_distortions(a, b, profile=True)
    r = out[6]                                                       # nothing to compare: the record of a pair of 0 frames
    assert not isinstance(r, Exception), r
    assert (r["n_frames"], r["n_samples"], r["err2"], r["sig2"], r["n_diff"], r["max_abs"], r["first_diff"]) == (0, 0, 0, 0, 0, 0, -1)
    assert (r["rows_a"], r["rows_b"]) == (0, len(dec[1]["pcm"])) and math.isinf(r["snr_db"]) and r["profile"] is None
    for i in (1, 2):
        assert isinstance(out[i], mlib.Mp3sError) and out[i].code == mlib.E_UNSUPPORTED, (i, out[i])
    for i in (3, 5):
        assert isinstance(out[i], mlib.Mp3sError) and out[i].code == dec[0].code, (i, out[i], dec[0])
    want = expect_pairs(ctx, [a[0], a[4]], [b[0], b[4]])
    check_pair(0, out[0], want[0])
    check_pair(4, out[4], want[1])
    # status == NULL in the C call: the first failing pair fails the call with its code and its text, no owner
    L = mlib.lib()

    def raw(xa, xb):
        n, _ka, pa, la = mlib._file_list(xa)
        _, _kb, pb, lb = mlib._file_list(xb)
        res, owner = (mlib.PcmDistortion * n)(), C.c_void_p()
        rc = L.mp3s_pcm_distortion_files(ctx.handle, pa, la, pb, lb, n, 0, C.byref(owner), res, None)
        assert not owner.value
        return rc, L.mp3s_last_error().decode()
    rc, why = raw(a[:2], b[:2])
    assert rc == mlib.E_UNSUPPORTED and "pair 1" in why and "1 channel" in why and "2 channel" in why, why
    rc, why = raw(a[2:4], b[2:4])
    assert rc == mlib.E_UNSUPPORTED and "pair 0" in why and "44100" in why and "48000" in why, why
    rc, why = raw([f44, garbage], [f44, f44])
    assert rc == dec[0].code and "pair 1" in why and "file a" in why, why
    rc, why = raw([f44, f44], [f44, garbage])
    assert rc == dec[0].code and "pair 1" in why and "file b" in why, why


@gpu
def test_unequal_lengths_compare_the_common_prefix(ctx, mlib, corpus):
    """a stream against its own first k frames (cut where walk_stream says frame k begins), and against itself with a bad header behind
    it: the decoder repeats that stream's last frame, which rows_* count as decode_streams does"""
    full, other = corpus["a"][0], corpus["b"][0]                     # 60 frames each, hide and clear re-encode of one input
    refs = mlib.walk_stream(full)["refs"]
    k = 23
    cut = full[:int(refs["file_off"][k])]
    dup = other + b"\x00" * 700
    assert mlib.walk_stream(cut)["n_frames"] == k and mlib.walk_stream(dup)["dup_last_frame"] == 1
    a, b = [other, cut, full, dup], [cut, other, dup, dup]
    want = expect_pairs(ctx, a, b)
    assert [(w["n_frames"], w["rows_a"], w["rows_b"]) for w in want] == [(k, 60 * 1152, k * 1152), (k, k * 1152, 60 * 1152),
                                                                         (60, 60 * 1152, 61 * 1152), (61, 61 * 1152, 61 * 1152)]
    out = ctx.pcm_distortions(a, b, profile=True)
    for i, (r, w) in enumerate(zip(out, want)):
        check_pair(i, r, w)
    assert out[0]["n_frames"] == k and out[0]["rows_a"] != out[0]["rows_b"] and len(out[0]["profile"]) == k


@gpu
def test_hide_distortions_is_the_two_step_way(ctx, mlib, corpus):
    files, msgs = corpus["files"], corpus["msgs"]
    garbage = b"not an mp3 file at all" * 10
    out = ctx.hide_distortions(files[:6] + [garbage], msgs[:6] + ["x"], profile=True)
    refused = ctx.hide_messages([garbage], ["x"])[0]
    assert isinstance(refused, mlib.Mp3sError) and isinstance(out[6], mlib.Mp3sError) and out[6].code == refused.code
    # the two-step way: corpus["a"] is the hide re-encode, corpus["b"] the clear one; hide_distortions compares clear against hidden
    want = expect_pairs(ctx, corpus["b"][:6], corpus["a"][:6])
    for i, (r, w, h) in enumerate(zip(out, want, corpus["hidden"])):
        check_pair(i, r, w)
        assert r["too_long"] == h["too_long"] and r["hide_offset"] == h["hide_offset"], (i, r["too_long"], r["hide_offset"], h["too_long"], h["hide_offset"])
    assert out[3]["too_long"] and not out[0]["too_long"] and any(r["err2"] > 0 for r in out[:6])
