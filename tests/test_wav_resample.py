"""The "wav_resample" option (MP3S_OPT_WAV_RESAMPLE): WAV files of any sampling rate, resampled on the device (k_wav_resample) to one of
the encoder's three rates before they are encoded.

The oracle is wav_resample_model: the rules of include/mp3s.h (mp3s_wav_resample_info) restated in numpy.  The kernel is compared
bit for bit with the model's integer sums over the tap table the library exports; every entry point is compared byte for byte with
what the option-OFF path makes of the canonical 16-bit stereo WAV at out_rate that holds the model's rows."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import wav_import_files as W
import wav_resample_model as R
from test_encode_batch import _drain, _same, wav_bytes
from test_wav_import import BITRATE, RATE, from_int16, header_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_EXIT = -8
# rate -> (target in auto mode, L, M, T) by the auto rule of mp3s_wav_resample_info
AUTO = {384000: (48000, 1, 8, 256), 8000: (32000, 4, 1, 32), 11025: (44100, 4, 1, 32), 16000: (32000, 2, 1, 32), 22050: (44100, 2, 1, 32), 24000: (48000, 2, 1, 32),
        37800: (44100, 7, 6, 32), 88200: (44100, 1, 2, 64), 96000: (48000, 1, 2, 64), 192000: (48000, 1, 4, 128)}
FORCED = {(48000, 44100): (147, 160, 36), (44100, 32000): (320, 441, 46), (11025, 32000): (1280, 441, 32), (44100, 48000): (160, 147, 32),
          (22050, 48000): (320, 147, 32)}
RATIOS = sorted({v[1:3] for v in AUTO.values()} | {v[:2] for v in FORCED.values()})
# sine test: the largest deviation of the MODEL's output from the analytically sampled 997 Hz full-scale sine, away from the ends
# (docs/LOG.md, computed once on the CPU); asserted with a factor of 2, which covers the +-1 LSB table differences between libms
SINE_DEVIATION = {(22050, 44100): 3.50, (96000, 48000): 1.05}


def stereo16(n, seed, kind="noise"):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return rng.integers(-32768, 32768, size=(n, 2), dtype=np.int64)
    k = np.arange(n)
    sq = np.where((k // 37) % 2 == 0, 32767, -32768)                    # a full-scale square wave: the overshoot reaches the clamp
    return np.stack([sq, -1 - sq], axis=1).astype(np.int64)


# ------------------------------------------------------------------------------------------------ CPU
def test_resample_info_on_a_table_of_headers(mlib):
    s = stereo16(3000, 1)
    for rate, (out, L, M, T) in AUTO.items():
        assert R.plan(rate, 1) == dict(out_rate=out, L=L, M=M, taps=T, half=T // 2), rate
        for n, ch, fmt in ((3000, 2, W.S16), (1, 1, W.U8), (1153, 1, W.S24), (2999, 2, W.F32)):
            x = from_int16(s[:n] if ch == 2 else s[:n, 0], fmt, np.random.default_rng(2))
            got = mlib.wav_resample_info(W.wav_file(x, fmt, rate=rate, between=[W.list_chunk(3)], pad=False), 128, 1)
            n_out, n_frames = R.counts(n, L, M)
            assert n_out == -(-n * L // M) and n_frames == -(-n_out // 1152)
            want = dict(out_rate=out, L=L, M=M, taps=T, half=T // 2, n_out=n_out, n_frames=n_frames)
            assert {k: got[k] for k in want} == want, (rate, n, got)
            assert got["in"] == dict(format=fmt, channels=ch, samplerate=rate, bits_per_sample=8 * W.BYTES[fmt], block_align=ch * W.BYTES[fmt],
                                     bitrate=128, data_offset=55, n_samples=n, n_frames=-(-n // 1152)), (rate, got)
    for (rate, mode), (L, M, T) in FORCED.items():
        got = mlib.wav_resample_info(W.wav_file(s, W.S16, rate=rate), 128, mode)
        assert R.plan(rate, mode) == dict(out_rate=mode, L=L, M=M, taps=T, half=T // 2), (rate, mode)
        assert (got["out_rate"], got["L"], got["M"], got["taps"], got["half"], got["n_out"]) == (mode, L, M, T, T // 2, -(-3000 * L // M)), (rate, mode, got)
    for rate in R.RATES:                                                   # a supported rate: auto leaves it, forcing it to itself too
        for mode in (1, rate):
            got = mlib.wav_resample_info(W.wav_file(s, W.S16, rate=rate), 128, mode)
            assert (got["out_rate"], got["L"], got["M"], got["n_out"], got["n_frames"]) == (rate, 1, 1, 3000, 3), (rate, mode, got)
    # refused rates: the reference's text
    for rate, mode in ((11127, 1), (0, 1), (0, 44100), (11127, 48000), (400000, 1), (500000, 1)):
        assert R.plan(rate, mode) is None
        with pytest.raises(mlib.Mp3sError) as e:
            mlib.wav_resample_info(W.wav_file(s, W.S16, rate=rate), 128, mode)
        assert (e.value.code, e.value.text) == (E_EXIT, RATE), (rate, mode, e.value)
    # the bitrate is checked against out_rate
    with pytest.raises(mlib.Mp3sError) as e:
        mlib.wav_resample_info(W.wav_file(s, W.S16, rate=22050), 100, 1)
    assert (e.value.code, e.value.text) == (E_EXIT, BITRATE)
    # arguments
    Lb = mlib.lib()
    w = mlib.WavResample()
    buf = np.frombuffer(W.wav_file(s, W.S16, rate=22050), dtype=np.uint8)
    assert Lb.mp3s_wav_resample_info(None, 100, 128, 1, C.byref(w)) == mlib.E_ARG
    assert Lb.mp3s_wav_resample_info(buf.ctypes.data, 0, 128, 1, C.byref(w)) == mlib.E_ARG
    assert Lb.mp3s_wav_resample_info(buf.ctypes.data, len(buf), 128, 1, None) == mlib.E_ARG
    for mode in (0, 2, -1, 22050, 44101, 96000):
        assert Lb.mp3s_wav_resample_info(buf.ctypes.data, len(buf), 128, mode, C.byref(w)) == mlib.E_ARG, mode
    assert Lb.mp3s_wav_resample_info(buf.ctypes.data, len(buf), 128, 1, C.byref(w)) == 0 and w.out_rate == 44100 and w.n_out == 6000


def test_what_the_import_rules_refuse_is_refused_identically(mlib):
    n_ok = 0
    for name, data, kbps, want in header_cases():
        if name == "rate_22050":                                            # the one refusal the option lifts
            assert mlib.wav_resample_info(data, kbps, 1)["out_rate"] == 44100
            continue
        for mode in (1, 44100):
            if isinstance(want, dict) and mode == 1:
                got = mlib.wav_resample_info(data, kbps, mode)
                assert {k: got["in"][k] for k in want} == want and (got["L"], got["M"]) == (1, 1), (name, got)
                n_ok += 1
            elif not isinstance(want, dict):
                with pytest.raises(mlib.Mp3sError) as e:
                    mlib.wav_resample_info(data, kbps, mode)
                assert (e.value.code, e.value.text) == want, (name, mode, e.value.code, e.value.text)
    assert n_ok >= 25


def test_the_tap_tables(mlib):
    for L, M in RATIOS:
        c = mlib.wav_resample_taps(L, M).astype(np.int64)
        H = 16 if L >= M else -(-16 * M // L)
        T = 2 * H
        assert c.shape == (L, T), (L, M, c.shape)
        assert (c.sum(axis=1) == 32768).all(), (L, M)
        # sum |c| <= 65535 over a phase would prove that one int32 sum cannot overflow, but this filter does not meet it: sum |c| is
        # 69 292 for L / M = 2 / 1 (58 080 for 1 / 2).  The device therefore adds the taps below 2 (H / 2) and the rest apart and
        # joins the sums in 64 bits; the bound is asserted for each part, where it proves the same thing
        # (test_the_clamp_is_reached has the input that overflows a single int32 sum).
        cut = 2 * (H // 2)
        assert (np.abs(c[:, :cut]).sum(axis=1) <= 65535).all() and (np.abs(c[:, cut:]).sum(axis=1) <= 65535).all(), (L, M)
        assert np.abs(c).sum(axis=1).max() <= 2 * 65535
        assert np.abs(c).max() < 32768                                      # every tap is an int16: the device packs pairs of them
        m, where, residual = R.model_taps(L, M)
        assert (np.abs(residual) <= T // 2).all()
        # within +-1 of the model's own double-precision table; where the phase's residual went to the tap, +-1 plus that residual
        bound = np.ones_like(c)
        bound[np.arange(L), where] += np.abs(residual)
        assert (np.abs(c - m) <= bound).all(), (L, M, np.argwhere(np.abs(c - m) > bound)[:4])
        # the symmetry of h: c[p][k] = c[L - p][T - 1 - k] for p > 0 and c[0][k] = c[0][T - 2 - k] (c[0][T - 1] = h(H) rounds to 0), up to the residual taps
        for p in range(L):
            q = (L - p) % L
            mirror = c[q][::-1] if p else np.concatenate([c[0][:T - 1][::-1], c[0][T - 1:]])
            same = c[p] == mirror
            same[where[p]] = True
            if p:
                same[T - 1 - where[q]] = True
            elif where[0] < T - 1:
                same[T - 2 - where[0]] = True
            assert same.all(), (L, M, p, np.argwhere(~same)[:4].tolist())
        assert c[0][T - 1] == 0
    Lb = mlib.lib()
    t = C.c_int32()
    buf = np.zeros(64, dtype=np.int32)
    assert Lb.mp3s_wav_resample_taps(2, 1, buf.ctypes.data, 64, C.byref(t)) == 0 and t.value == 32
    assert Lb.mp3s_wav_resample_taps(2, 1, buf.ctypes.data, 63, C.byref(t)) == mlib.E_ARG and t.value == 32
    assert Lb.mp3s_wav_resample_taps(2, 1, None, 64, C.byref(t)) == mlib.E_ARG
    assert Lb.mp3s_wav_resample_taps(2, 1, buf.ctypes.data, 64, None) == mlib.E_ARG
    for L, M in ((0, 1), (1, 0), (1281, 1), (1, 9)):
        assert Lb.mp3s_wav_resample_taps(L, M, buf.ctypes.data, 64, C.byref(t)) == mlib.E_ARG, (L, M)


def test_the_model_resamples_a_constant_to_itself():
    """DC gain is exactly 1: away from the ends a constant input comes out as it went in, at every ratio"""
    for L, M in RATIOS:
        c, _, _ = R.model_taps(L, M)
        for v in (32767, -32768, 12345):
            y = R.resample(np.full(600, v, dtype=np.int16), L, M, c)
            edge = c.shape[1] * max(1, -(-L // M))
            assert (y[edge:len(y) - edge] == v).all(), (L, M, v)


def test_the_option_table_names_it(mlib):
    assert mlib.Context.OPTIONS["wav_resample"] == 21 and mlib.Context.KERNELS[-1] == "k_wav_resample"
    assert mlib.wav_resample_default() in (0, 1, 32000, 44100, 48000)
    text = open(os.path.join(ROOT, "include", "mp3s.h")).read()
    assert re.search(r"#define MP3S_OPT_WAV_RESAMPLE 21\b", text) and re.search(r"#define MP3S_OPT_COUNT 22\b", text)
    assert "(no resampling)" not in text


def test_wav_resample_kernel_listing():
    """the compiler's listing of k_wav_resample: no scratch, no spill, dot products of int16 pairs; and the assembly of the device code
    holds no scalar store to memory, no scalar atomic and no scalar cache write-back"""
    from test_build_resources import HIPCC, PKG, resource_usage
    usage = resource_usage()
    hits = [k for k in usage if k.startswith("mp3s::k_wav_resample")]
    assert len(hits) == 1, sorted(usage)
    u = usage[hits[0]]
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, u
    assert u["Occupancy [waves/SIMD]"] >= 4 and u["VGPRs"] <= 64, u
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "--cuda-device-only",
                        "-S", "-o", "-", os.path.join(PKG, "csrc", "mp3s_device.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = r.stdout
    start = asm.index("\n_ZN4mp3s14k_wav_resample")
    body = asm[start:asm.index(".end_amdhsa_kernel", start)]
    assert "v_dot2" in body and "scratch_" not in body and "flat_load" not in body and "flat_store" not in body
    assert not re.search(r"(global|buffer|flat)_(load|store)_(u|s)?(byte|short)", body)
    s = "s" + "_"
    banned = [s + "store" + "_", s + "buffer_" + "store", s + "scratch_" + "store", s + "atomic" + "_", s + "buffer_" + "atomic", s + "dcache_" + "wb", s + "dcache_" + "discard"]
    for word in banned:
        assert not re.search(r"\b" + word, asm, re.I), word


# ------------------------------------------------------------------------------------------------ GPU
def make_file(x16, fmt, ch, rate, rng, k=0):
    """int16 [n, 2] -> (file of that format / channel count at `rate` with a chunk of k bytes in front of the samples, the int16 rows the import rules make)"""
    s = from_int16(x16 if ch == 2 else x16[:, 0], fmt, rng)
    f = W.wav_file(s, fmt, rate=rate, between=[W.list_chunk(k)] if k else [], pad=False)
    return f, W.stereo_frames(s, fmt)[:len(x16)]


def model_rows(mlib, rows, rate, mode):
    p = R.plan(rate, mode)
    if p["L"] == p["M"]:
        return rows, p
    return R.resample(rows, p["L"], p["M"], mlib.wav_resample_taps(p["L"], p["M"])), p


@pytest.mark.gpu
@pytest.mark.parametrize("channels", (1, 2))
@pytest.mark.parametrize("fmt", W.FORMATS)
def test_the_resample_kernel_against_numpy(mlib, fmt, channels):
    """debug_wav_gather with the option on, bit for bit: every rate of the table + the forced pairs, lengths that end inside a frame and
    inside a tile, data offsets of every residue mod 4 and odd ones, full-scale noise and square waves, the files of a call side by side"""
    rng = np.random.default_rng(3000 + 10 * fmt + channels)
    ctx = mlib.Context(0)
    try:
        for mode, rates in ((1, list(AUTO) + [44100]), (44100, [48000, 44100, 22050]), (32000, [44100, 11025]), (48000, [44100, 22050])):
            assert ctx.set_option("wav_resample", mode) in (0, 1, 32000, 44100, 48000)
            files, want = [], []
            for i, rate in enumerate(rates):
                p = R.plan(rate, mode)
                per_out = p["M"] / p["L"]
                for j, n_out_about in enumerate((1, 700, 1152 + 575, 2 * 1024 + 3, 3 * 1152 + 1)):
                    n = max(1, int(n_out_about * per_out) + (j & 1))
                    x = stereo16(n, 100 * i + j, "square" if j == 2 else "noise")
                    f, rows = make_file(x, fmt, channels, rate, rng, k=(i + 3 * j) % 16)
                    info = mlib.wav_resample_info(f, 128, mode)
                    assert info["in"]["n_samples"] == n and info["in"]["channels"] == channels and info["in"]["format"] == fmt
                    y, _ = model_rows(mlib, rows, rate, mode)
                    assert len(y) == info["n_out"]
                    files.append(f)
                    want.append(R.frames_of(y))
            order = rng.permutation(len(files))
            got = ctx.debug_wav_gather([files[o] for o in order])
            assert got.shape[0] == sum(len(want[o]) for o in order) // 1152
            at = 0
            for o in order:
                e = want[o]
                g = got[at:at + len(e) // 1152].reshape(-1, 2)
                if not np.array_equal(g, e):
                    bad = np.argwhere(g != e)
                    raise AssertionError((W.NAMES[fmt], channels, "mode", mode, "file", int(o), "rate", rates[o // 5], "rows", len(e), "first bad (row, channel)",
                                          bad[0].tolist(), "got", g[bad[0][0]].tolist(), "want", e[bad[0][0]].tolist(), "bad values", len(bad)))
                at += len(e) // 1152
            assert np.array_equal(ctx.debug_wav_gather([files[2]]).reshape(-1, 2), want[2])          # a file alone
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rate", (22050, 96000))
def test_a_stream_longer_than_the_grid(mlib, rate):
    """the launch has 2 048 tiles of 1 024 output rows along x at most: a stream of more than 2 097 152 output rows (48 s at 44.1 kHz) sends
    its workgroups round the tile loop a second time -- the barrier at its top, the span's LDS used again, tile numbers beyond 2 047 --
    once up (L > M) and once down (M > L); a short file in front and behind, so that the long stream is not the batch's first"""
    p = R.plan(rate, 1)
    n = (2048 * 1024 + 3 * 1024 + 77) * p["M"] // p["L"]
    rng = np.random.default_rng(rate)
    x = rng.integers(-32768, 32768, size=n, dtype=np.int64)
    short = stereo16(1500, 9)
    taps = mlib.wav_resample_taps(p["L"], p["M"])
    want = [R.frames_of(R.resample(short, p["L"], p["M"], taps)), None, None]
    y = R.resample(x, p["L"], p["M"], taps)
    assert len(y) > 2049 * 1024
    want[1] = R.frames_of(np.stack([y, y], axis=1))
    want[2] = want[0]
    files = [W.wav_file(short, W.S16, rate=rate), W.wav_file(x, W.S16, rate=rate), W.wav_file(short, W.S16, rate=rate)]
    ctx = mlib.Context(0)
    try:
        ctx.set_option("wav_resample", 1)
        got = ctx.debug_wav_gather(files).reshape(-1, 2)
    finally:
        ctx.close()
    e = np.concatenate(want)
    assert got.shape == e.shape
    if not np.array_equal(got, e):
        bad = np.argwhere(got != e)
        raise AssertionError((rate, "first bad (row, channel)", bad[0].tolist(), "last", bad[-1].tolist(), "bad values", len(bad)))


@pytest.mark.gpu
def test_the_clamp_is_reached(mlib):
    """a square wave whose overshoot leaves int16, and the worst input there is: full scale with the sign of every tap of a phase, left
    with it and right against it -- the sum of that row is beyond +-2^31, what ONE int32 accumulator would wrap to the other sign"""
    x = stereo16(4000, 0, "square")
    taps = mlib.wav_resample_taps(2, 1).astype(np.int64)
    p_bad = int(np.abs(taps).sum(axis=1).argmax())
    assert p_bad == 1 and np.abs(taps[p_bad]).sum() > 65535
    for m in (1000, 2000):                                                # output row 2 m + p: i0 = m, taps on x[m - 15 .. m + 16]
        sign = np.where(taps[p_bad] >= 0, 32767, -32768)
        x[m - 15:m + 17, 0], x[m - 15:m + 17, 1] = sign, -1 - sign
        assert abs(int((taps[p_bad] * x[m - 15:m + 17, 0]).sum())) > 1 << 31
    g, p = R._gathered(x, 2, 1, 32)
    s = ((g * taps[p][:, :, None]).sum(axis=1) + (1 << 14)) >> 15
    assert s.max() > 32767 and s.min() < -32768                           # the model's sums leave int16: the clamp decides
    ctx = mlib.Context(0)
    try:
        ctx.set_option("wav_resample", 1)
        got = ctx.debug_wav_gather([W.wav_file(x, W.S16, rate=22050)]).reshape(-1, 2)
    finally:
        ctx.close()
    assert np.array_equal(got, R.frames_of(R.resample(x, 2, 1, taps))) and got.max() == 32767 and got.min() == -32768
    assert got[2001].tolist() == [32767, -32768] and got[4001].tolist() == [32767, -32768]


def resample_list(mlib):
    """-> [(file, bitrate, hide bits or None, (int16 rows, rate) or None for a refused file)]"""
    from synth_pcm import synth_pcm
    rng = np.random.default_rng(88)
    bits = lambda m: np.array(mlib.message_frame(m), dtype=np.uint8)
    out = []

    def add(frames, cut, fmt, ch, rate, kbps, hide, seed, k=0):
        pcm = synth_pcm(frames, seed=seed, rate=rate if rate in R.RATES else 44100)
        pcm = pcm[:len(pcm) - cut].astype(np.int64)
        f, rows = make_file(pcm, fmt, ch, rate, rng, k)
        out.append((f, kbps, hide, (rows, rate)))

    add(20, 3, W.S16, 2, 22050, 128, bits("half rate"), 600)                # 0
    add(30, 0, W.S16, 1, 16000, 64, None, 601, k=3)                         # 1: a voice recording, mono -> 32 000 Hz
    add(12, 100, W.U8, 1, 8000, 64, bits("telephone"), 602)                 # 2
    add(90, 7, W.S24, 2, 96000, 192, bits("studio"), 603, k=5)              # 3: -> 48 000 Hz
    add(40, 0, W.S16, 2, 44100, 128, bits("native"), 604)                   # 4: native and canonical: k_wav_gather
    add(41, 577, W.F32, 2, 44100, 128, None, 605)                           # 5: native, k_wav_import
    add(25, 1, W.S32, 2, 11025, 128, bits("x" * 300), 606)                  # 6: too long for its frames
    add(60, 0, W.S16, 2, 37800, 192, None, 607)                             # 7: L = 7, M = 6
    add(50, 11, W.F32, 1, 192000, 192, bits("quarter"), 608, k=1)           # 8
    add(33, 0, W.S16, 2, 48000, 192, bits("native 48"), 609)                # 9
    add(70, 2, W.S24, 1, 88200, 128, None, 610)                             # 10
    out.append((W.wav_file(stereo16(3000, 5), W.S16, rate=11127), 128, None, None))      # 11: refused
    return out


def resample_oracle(ctx, mlib, files, mode=1):
    assert ctx.get_option("wav_resample") == 0 and ctx.get_option("wav_import") == 0
    want = []
    for f, kbps, hide, src in files:
        if src is None:
            with pytest.raises(mlib.Mp3sError) as e:
                mlib.wav_resample_info(f, kbps, mode)
            want.append(e.value)
            continue
        y, p = model_rows(mlib, src[0], src[1], mode)
        w = ctx.encode_file(wav_bytes(R.frames_of(y), p["out_rate"]), kbps, hide)
        assert w["sampling_rate"] == p["out_rate"] and w["n_frames"] == -(-len(y) // 1152) and w["channels"] == 2
        want.append(w)
    return want


@pytest.mark.gpu
def test_every_entry_point_equals_the_strict_path_on_the_models_rows(mlib):
    files = resample_list(mlib)
    ctx = mlib.Context(0)
    try:
        want = resample_oracle(ctx, mlib, files)
        assert [w["sampling_rate"] for w in want[:11]] == [44100, 32000, 32000, 48000, 44100, 44100, 44100, 44100, 48000, 48000, 44100]
        assert want[6]["too_long"] and not want[0]["too_long"] and want[11].code == E_EXIT and want[11].text == RATE
        assert ctx.set_option("wav_resample", 1) == 0 and ctx.get_option("wav_resample") == 1
        for i, (f, kbps, hide, _) in enumerate(files):                      # (a) encode_file
            try:
                got = ctx.encode_file(f, kbps, hide)
            except mlib.Mp3sError as e:
                got = e
                assert e.text == want[i].text
            _same(mlib, got, want[i], ("encode_file", i))
        got = ctx.encode_files([f[0] for f in files], [f[1] for f in files], hide_bits=[f[2] for f in files])      # (b) one mixed list
        assert len(got) == len(files)
        for i, (a, b) in enumerate(zip(got, want)):
            _same(mlib, a, b, ("encode_files", i))
        assert isinstance(got[11], mlib.Mp3sError) and got[11].code == E_EXIT
        job = lambda idx: ("enc", ([files[i][0] for i in idx], [files[i][1] for i in idx], [files[i][2] for i in idx]))      # (c) the pipe
        index = [[4], [0], [4, 5], [0, 4, 5, 10], [3, 9, 8], [1, 2], [6, 11], [7, 3]]
        pipe = mlib.Pipe(ctx, depth=3, max_job_bytes=4 << 20, scan_threads=2)
        ctx.set_option("wav_resample", 0)                                   # a pipe keeps the value of its creation
        try:
            res = _drain(pipe, [job(idx) for idx in index])
            st = pipe.stats()
        finally:
            pipe.close()
        assert st["collected"] == len(index), st
        for k, (r, idx) in enumerate(zip(res, index)):
            assert len(r) == len(idx)
            for a, i in zip(r, idx):
                _same(mlib, a, want[i], ("pipe", k, i))
        # forced modes: everything to one rate
        for mode in (32000, 44100, 48000):
            some = [files[i] for i in (0, 4, 9, 3)]
            w = resample_oracle(ctx, mlib, some, mode)
            assert all(x["sampling_rate"] == mode for x in w)
            ctx.set_option("wav_resample", mode)
            g = ctx.encode_files([f[0] for f in some], [f[1] for f in some], hide_bits=[f[2] for f in some])
            ctx.set_option("wav_resample", 0)
            for i, (a, b) in enumerate(zip(g, w)):
                _same(mlib, a, b, ("forced", mode, i))
    finally:
        ctx.close()


FACADE_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
from mp3stego import Steganography
Steganography(quiet=True).encode_wav_to_mp3(sys.argv[2], sys.argv[3], 128)
"""


@pytest.mark.gpu
def test_the_facade_gets_the_option_from_the_environment(ctx, mlib, tmp_path):
    from synth_pcm import synth_pcm
    rng = np.random.default_rng(10)
    f, rows = make_file(synth_pcm(20, seed=630)[:20 * 1152 - 300].astype(np.int64), W.S16, 1, 16000, rng)
    y, p = model_rows(mlib, rows, 16000, 1)
    want = ctx.encode_file(wav_bytes(R.frames_of(y), 32000), 128)
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.mp3")
    with open(src, "wb") as fh:
        fh.write(f)
    env = {k: v for k, v in os.environ.items() if k not in ("MP3S_WAV_IMPORT", "MP3S_WAV_RESAMPLE")}
    run = lambda e: subprocess.run([sys.executable, "-c", FACADE_CHILD, os.path.join(ROOT, "mp3-steganography-lib_amd"), src, dst],
                                   env=e, capture_output=True, text=True, timeout=300)
    r = run(env)                                                           # off: today's refusal
    assert r.returncode == 1 and r.stderr.strip().splitlines()[-1] == RATE and not os.path.exists(dst), (r.returncode, r.stderr[-2000:])
    r = run(dict(env, MP3S_WAV_RESAMPLE="1"))
    assert r.returncode == 0, r.stderr[-4000:]
    with open(dst, "rb") as fh:
        assert fh.read() == bytes(want["data"])


@pytest.mark.gpu
def test_off_means_off(mlib):
    from synth_pcm import synth_pcm
    low = W.wav_file(synth_pcm(4, seed=640), W.S16, rate=22050)
    native = [wav_bytes(synth_pcm(n, seed=641 + n, rate=r), r) for n, r in ((40, 44100), (3, 48000), (17, 44100), (9, 32000))]
    kbps = [128, 192, 128, 64]
    c = mlib.Context(0)
    try:
        assert c.get_option("wav_resample") == 0
        for v in (2, 22050, 96000, 44101):
            with pytest.raises(mlib.Mp3sError) as e:
                c.set_option("wav_resample", v)
            assert e.value.code == mlib.E_ARG
        for v in (1, 32000, 44100, 48000, 0):
            c.set_option("wav_resample", v)
            assert c.get_option("wav_resample") == v
        for imp in (0, 1):                                                  # with and without the import reader: today's text
            c.set_option("wav_import", imp)
            with pytest.raises(mlib.Mp3sError) as e:
                c.encode_file(low, 128)
            assert (e.value.code, e.value.text) == (E_EXIT, RATE)
            got = c.encode_files([low, native[0]], 128)
            assert isinstance(got[0], mlib.Mp3sError) and got[0].code == E_EXIT and not isinstance(got[1], Exception)
            # (a list's entry carries the code; the text is the call's when status == NULL: the first refused file fails it)
            buf = np.frombuffer(low, dtype=np.uint8)
            ptr, lens, kb = (C.c_void_p * 1)(buf.ctypes.data), (C.c_size_t * 1)(len(buf)), (C.c_int32 * 1)(128)
            out, owner = (mlib.File * 1)(), C.c_void_p()
            assert mlib.lib().mp3s_encode_files(c.handle, ptr, lens, 1, kb, None, None, C.byref(owner), out, None) == E_EXIT
            assert mlib.lib().mp3s_last_error().decode() == RATE and owner.value is None
            pipe = mlib.Pipe(c, depth=2, max_job_bytes=1 << 20, scan_threads=1)
            try:
                r = _drain(pipe, [("enc", ([low], [128], [None]))])
            finally:
                pipe.close()
            assert isinstance(r[0][0], mlib.Mp3sError) and r[0][0].code == E_EXIT
        c.set_option("wav_import", 0)
        off = c.encode_files(native, kbps)
        c.set_option("wav_resample", 1)
        c.profile_select(None); c.profile_enable(True)
        on = c.encode_files(native, kbps)
        pr = c.profile_collect()
        assert pr["k_wav_resample"][1] == 0 and sum(v[1] for v in pr.values()) > 0, pr      # a batch of native files never launches the resampler
        for i, (a, b) in enumerate(zip(on, off)):
            _same(mlib, a, b, ("native", i))
        c.encode_files(native + [low], kbps + [128])
        pr = c.profile_collect()
        c.profile_enable(False)
        assert pr["k_wav_resample"][1] == 1, pr                              # ... and a batch with one file to resample launches it once
    finally:
        c.close()


def sine(rate, n):
    return np.rint(32767.0 * np.sin(2 * np.pi * 997.0 * np.arange(n) / rate)).astype(np.int64)


def sine_deviation(y, L, M, T, out_rate):
    """largest distance of y (one channel) from the analytically sampled sine, the filter's length away from both ends"""
    edge = T * max(1, -(-L // M))
    n = np.arange(len(y))
    ideal = 32767.0 * np.sin(2 * np.pi * 997.0 * n / out_rate)
    return float(np.abs(y - ideal)[edge:len(y) - edge].max())


def test_the_models_deviation_from_the_sine_is_the_recorded_one():
    for (rate, out), recorded in SINE_DEVIATION.items():
        p = R.plan(rate, 1)
        c, _, _ = R.model_taps(p["L"], p["M"])
        y = R.resample(sine(rate, rate // 4), p["L"], p["M"], c)
        d = sine_deviation(y.astype(np.float64), p["L"], p["M"], p["taps"], out)
        assert abs(d - recorded) <= 0.01, (rate, d, recorded)


@pytest.mark.gpu
@pytest.mark.parametrize("rate", (22050, 96000))
def test_a_sine_stays_a_sine(mlib, rate):
    """numeric sanity: against the ideal float64 filter of the same input the device is within T + 0.5 LSB (+-0.5 per rounded tap, a
    residual of at most T / 2, the final rounding); against the analytic sine within twice the model's recorded deviation"""
    p = R.plan(rate, 1)
    x = sine(rate, rate // 4)
    ctx = mlib.Context(0)
    try:
        ctx.set_option("wav_resample", 1)
        got = ctx.debug_wav_gather([W.wav_file(x, W.S16, rate=rate)]).reshape(-1, 2)
    finally:
        ctx.close()
    n_out, _ = R.counts(len(x), p["L"], p["M"])
    y = got[:n_out, 0].astype(np.float64)
    assert np.array_equal(got[:, 0], got[:, 1]) and not got[n_out:].any()
    ideal = np.clip(R.resample_ideal(x, p["L"], p["M"]), -32768, 32767)
    worst = float(np.abs(y - ideal).max())
    dev = sine_deviation(y, p["L"], p["M"], p["taps"], p["out_rate"])
    print("rate", rate, "device - ideal filter:", worst, "LSB; device - analytic sine:", dev, "LSB")
    assert worst <= p["taps"] + 0.5, worst
    assert dev <= 2 * SINE_DEVIATION[(rate, p["out_rate"])], dev
