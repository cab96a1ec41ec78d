"""The "wav_import" option (MP3S_OPT_WAV_IMPORT): the WAV files people have -- mono, 8/24/32-bit, float, extensible headers, chunks
anywhere, any length -- through mp3s_wav_import_info on the host and k_wav_import on the device.

The oracle of every GPU comparison is built here from numpy and the reference-pinned strict path: the samples are converted by the
rules of include/mp3s.h in numpy (wav_import_files.to_int16), mono is duplicated, the last frame zero-filled, a canonical 16-bit
stereo WAV is written with test_encode_batch.wav_bytes and THAT is encoded with the option off.  Equality = bytes and the fields
kbps, sampling_rate, channels, n_frames, too_long, hide_offset."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import wav_import_files as W
from test_encode_batch import _drain, _same, mixed_list, wav_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD, COMPRESSED, NOT_INT = "Bad WAVE file.", "Unsupported WAVE file, compression used instead of PCM.", "Unsupported WAVE file, samples not int8, int16 or int32 type."
RATE, BITRATE = "Unsupported sampling frequency.", "Unsupported bitrate configuration."
E_MALFORMED, E_UNSUPPORTED, E_EXIT = -4, -5, -8


def ramp(n, channels, fmt):
    """n deterministic samples per channel of the format's own range"""
    i = np.arange(n * channels, dtype=np.int64)
    v = {W.U8: (i * 37 + 5) % 256, W.S16: (i * 7919) % 65536 - 32768, W.S24: (i * 7919 * 251) % (1 << 24) - (1 << 23),
         W.S32: (i * 2654435761) % (1 << 32) - (1 << 31), W.F32: (((i * 7919) % 65536 - 32768) / 32768.0).astype(np.float32)}[fmt]
    return v if channels == 1 else v.reshape(n, channels)


def header_cases():
    """-> [(name, file, bitrate, what the import rules say)]: dict(format, channels, data_offset, n_samples, n_frames) or (code, text)"""
    cases = []
    ok = lambda fmt, ch, off, n: dict(format=fmt, channels=ch, data_offset=off, n_samples=n, n_frames=(n + 1151) // 1152)
    for fmt in W.FORMATS:                                                   # each format x mono / stereo, plain 16-byte fmt
        for ch in (1, 2):
            cases.append((f"{W.NAMES[fmt]}_{ch}ch", W.wav_file(ramp(1200, ch, fmt), fmt), 128, ok(fmt, ch, 44, 1200)))
    s16, s24, s32, f32 = ramp(1152, 2, W.S16), ramp(100, 2, W.S24), ramp(100, 1, W.S32), ramp(100, 2, W.F32)
    cases.append(("fmt18_s16", W.wav_file(s16, W.S16, fmt_size=18), 128, ok(W.S16, 2, 46, 1152)))
    cases.append(("fmt18_f32", W.wav_file(f32, W.F32, fmt_size=18), 128, ok(W.F32, 2, 46, 100)))
    cases.append(("ext_pcm24", W.wav_file(s24, W.S24, fmt_size=40), 128, ok(W.S24, 2, 68, 100)))
    cases.append(("ext_f32", W.wav_file(f32, W.F32, fmt_size=40), 128, ok(W.F32, 2, 68, 100)))
    cases.append(("ext_valid20_in24", W.wav_file(s24, W.S24, fmt_size=40, valid_bits=20), 128, ok(W.S24, 2, 68, 100)))
    cases.append(("ext_valid20_in32", W.wav_file(s32, W.S32, fmt_size=40, valid_bits=20), 128, ok(W.S32, 1, 68, 100)))
    for k in (1, 2, 200, 70000):                                            # a LIST chunk between fmt and data (odd sizes with their pad byte)
        off = W.data_offset_of(between=[W.list_chunk(k)])
        assert off == 44 + 8 + k + (k & 1)
        cases.append((f"list{k}", W.wav_file(s16, W.S16, between=[W.list_chunk(k)]), 128, ok(W.S16, 2, off, 1152)))
    for k in (1, 3, 7):                                                     # ... and an odd one whose writer left the pad byte out: an ODD offset
        cases.append((f"list{k}_unpadded", W.wav_file(s16, W.S16, between=[W.list_chunk(k)], pad=False), 128, ok(W.S16, 2, 52 + k, 1152)))
    cases.append(("list5_unpadded_s24_mono", W.wav_file(ramp(100, 1, W.S24), W.S24, between=[W.list_chunk(5)], pad=False), 128, ok(W.S24, 1, 57, 100)))
    cases.append(("chunk_in_front_of_fmt", W.wav_file(s16, W.S16, before=[(b"JUNK", b"\0" * 28)]), 128, ok(W.S16, 2, 44 + 36, 1152)))
    cases.append(("bext_and_list", W.wav_file(s24, W.S24, before=[(b"bext", b"x" * 603)], between=[W.list_chunk(9)]), 128,
                  ok(W.S24, 2, 12 + 8 + 604 + 24 + 8 + 10 + 8, 100)))
    cases.append(("chunk_behind_data", W.wav_file(ramp(1151, 1, W.U8), W.U8, after=[W.list_chunk(300, fill=0x55)]), 128, ok(W.U8, 1, 44, 1151)))
    cases.append(("declared_too_large", W.wav_file(s16, W.S16, declared=1 << 20), 128, ok(W.S16, 2, 44, 1152)))
    cases.append(("declared_0", W.wav_file(s16, W.S16, declared=0), 128, ok(W.S16, 2, 44, 1152)))
    cases.append(("declared_all_ones", W.wav_file(s24, W.S24, declared=0xFFFFFFFF), 128, ok(W.S24, 2, 44, 100)))
    cases.append(("declared_smaller", W.wav_file(s16, W.S16, declared=400, after=[W.list_chunk(8)]), 128, ok(W.S16, 2, 44, 100)))
    cases.append(("cut_last_sample", W.wav_file(s24, W.S24, cut=2), 128, ok(W.S24, 2, 44, 99)))
    cases.append(("block_align_field_wrong", W.wav_file(s24, W.S24, block_align=4), 128, ok(W.S24, 2, 44, 100)))
    cases.append(("rate_32000_bitrate_64", W.wav_file(s16, W.S16, rate=32000), 64, ok(W.S16, 2, 44, 1152)))
    cases.append(("rate_48000_bitrate_320", W.wav_file(f32, W.F32, rate=48000), 320, ok(W.F32, 2, 44, 100)))
    # refusals, code and text
    good = W.wav_file(s16, W.S16)
    cases.append(("no_riff", b"RIFX" + good[4:], 128, (E_EXIT, BAD)))
    cases.append(("no_wave", good[:8] + b"WAVX" + good[12:], 128, (E_EXIT, BAD)))
    cases.append(("too_short", good[:11], 128, (E_EXIT, BAD)))
    data = W.sample_bytes(s16, W.S16)
    body = b"WAVE" + b"data" + struct.pack("<I", len(data)) + data + W.fmt_chunk(W.S16, 2, 44100)
    cases.append(("data_in_front_of_fmt", b"RIFF" + struct.pack("<I", len(body)) + body, 128, (E_EXIT, BAD)))
    cases.append(("no_data", good[:36], 128, (E_EXIT, BAD)))
    cases.append(("no_fmt", good[:12] + b"JUNK" + good[16:], 128, (E_EXIT, BAD)))
    cases.append(("tag_2", W.wav_file(s16, W.S16, tag=2), 128, (E_EXIT, COMPRESSED)))
    cases.append(("fmt_size_20", good[:16] + struct.pack("<I", 20) + good[20:36] + b"\0" * 4 + good[36:], 128, (E_EXIT, COMPRESSED)))
    cases.append(("ext_tag_in_16_bytes", W.wav_file(s16, W.S16, tag=0xFFFE), 128, (E_EXIT, COMPRESSED)))
    cases.append(("float64", W.wav_file(s16, W.S16, tag=3, bits=64), 128, (E_EXIT, NOT_INT)))
    cases.append(("bits_12", W.wav_file(s16, W.S16, bits=12), 128, (E_EXIT, NOT_INT)))
    cases.append(("float16", W.wav_file(s16, W.S16, tag=3, bits=16), 128, (E_EXIT, NOT_INT)))
    cases.append(("channels_3", W.wav_file(s16, W.S16, channels=3), 128, (E_UNSUPPORTED, "more than two channels")))
    cases.append(("channels_0", W.wav_file(s16, W.S16, channels=0, block_align=4), 128,
                  (E_MALFORMED, "WAVE header with zero channels (ZeroDivisionError in the reference)")))
    cases.append(("rate_22050", W.wav_file(s16, W.S16, rate=22050), 128, (E_EXIT, RATE)))
    cases.append(("bitrate_100", good, 100, (E_EXIT, BITRATE)))
    cases.append(("bitrate_64_at_44100_is_fine", good, 64, ok(W.S16, 2, 44, 1152)))
    cases.append(("no_samples", W.wav_file(s16[:0], W.S16, channels=2), 128, (E_UNSUPPORTED, "no samples")))
    cases.append(("less_than_one_sample", W.wav_file(s24[:1], W.S24, cut=1), 128, (E_UNSUPPORTED, "no samples")))
    return cases


# what mp3s_wav_parse -- the reference's reader, the default -- says to the same files: recorded from the parent commit's build.
# dict: (channels, samplerate, bits_per_sample, num_of_samples, data_offset, n_values); tuple: (code, text)
STRICT = {
    'list1_unpadded': {'channels': 2, 'samplerate': 44100, 'bits_per_sample': 16, 'num_of_samples': 1152, 'data_offset': 53, 'n_values': 2304},
    'list3_unpadded': {'channels': 2, 'samplerate': 44100, 'bits_per_sample': 16, 'num_of_samples': 1152, 'data_offset': 55, 'n_values': 2304},
    'list7_unpadded': {'channels': 2, 'samplerate': 44100, 'bits_per_sample': 16, 'num_of_samples': 1152, 'data_offset': 59, 'n_values': 2304},
    'list5_unpadded_s24_mono': (-8, 'Unsupported WAVE file, samples not int8, int16 or int32 type.'),
    'u8_1ch': {'channels': 1, 'samplerate': 44100, 'bits_per_sample': 8, 'num_of_samples': 1200, 'data_offset': 44, 'n_values': 600},
    'u8_2ch': {'channels': 2, 'samplerate': 44100, 'bits_per_sample': 8, 'num_of_samples': 1200, 'data_offset': 44, 'n_values': 1200},
    's16_1ch': {'channels': 1, 'samplerate': 44100, 'bits_per_sample': 16, 'num_of_samples': 1200, 'data_offset': 44, 'n_values': 1200},
    's16_2ch': {'channels': 2, 'samplerate': 44100, 'bits_per_sample': 16, 'num_of_samples': 1200, 'data_offset': 44, 'n_values': 2400},
    's24_1ch': (-8, 'Unsupported WAVE file, samples not int8, int16 or int32 type.'),
    's24_2ch': (-8, 'Unsupported WAVE file, samples not int8, int16 or int32 type.'),
    's32_1ch': {'channels': 1, 'samplerate': 44100, 'bits_per_sample': 32, 'num_of_samples': 1200, 'data_offset': 44, 'n_values': 2400},
    's32_2ch': {'channels': 2, 'samplerate': 44100, 'bits_per_sample': 32, 'num_of_samples': 1200, 'data_offset': 44, 'n_values': 4800},
    'f32_1ch': (-8, 'Unsupported WAVE file, compression used instead of PCM.'),
    'f32_2ch': (-8, 'Unsupported WAVE file, compression used instead of PCM.'),
    'fmt18_s16': (-8, 'Unsupported WAVE file, compression used instead of PCM.'),
    'fmt18_f32': (-8, 'Unsupported WAVE file, compression used instead of PCM.'),
    'ext_pcm24': (-8, 'Unsupported WAVE file, compression used instead of PCM.'),
    'ext_f32': (-8, 'Unsupported WAVE file, compression used instead of PCM.'),
    'ext_valid20_in24': (-8, 'Unsupported WAVE file, compression used instead of PCM.'),
    'ext_valid20_in32': (-8, 'Unsupported WAVE file, compression used instead of PCM.'),
    'list1': {'channels': 2, 'samplerate': 44100, 'bits_per_sample': 16, 'num_of_samples': 1152, 'data_offset': 54, 'n_values': 2304},
    'list2': {'channels': 2, 'samplerate': 44100, 'bits_per_sample': 16, 'num_of_samples': 1152, 'data_offset': 54, 'n_values': 2304},
    'list200': (-8, 'Bad WAVE file.'),
    'list70000': (-8, 'Bad WAVE file.'),
    'chunk_in_front_of_fmt': {'channels': 2, 'samplerate': 44100, 'bits_per_sample': 16, 'num_of_samples': 1152, 'data_offset': 80, 'n_values': 2304},
    'bext_and_list': (-8, 'Bad WAVE file.'),
    'chunk_behind_data': {'channels': 1, 'samplerate': 44100, 'bits_per_sample': 8, 'num_of_samples': 1151, 'data_offset': 44, 'n_values': 730},
    'declared_too_large': {'channels': 2, 'samplerate': 44100, 'bits_per_sample': 16, 'num_of_samples': 262144, 'data_offset': 44, 'n_values': 2304},
    'declared_0': {'channels': 2, 'samplerate': 44100, 'bits_per_sample': 16, 'num_of_samples': 0, 'data_offset': 44, 'n_values': 0},
    'declared_all_ones': (-8, 'Unsupported WAVE file, samples not int8, int16 or int32 type.'),
    'declared_smaller': {'channels': 2, 'samplerate': 44100, 'bits_per_sample': 16, 'num_of_samples': 100, 'data_offset': 44, 'n_values': 400},
    'cut_last_sample': (-8, 'Unsupported WAVE file, samples not int8, int16 or int32 type.'),
    'block_align_field_wrong': (-8, 'Unsupported WAVE file, samples not int8, int16 or int32 type.'),
    'rate_32000_bitrate_64': {'channels': 2, 'samplerate': 32000, 'bits_per_sample': 16, 'num_of_samples': 1152, 'data_offset': 44, 'n_values': 2304},
    'rate_48000_bitrate_320': (-8, 'Unsupported WAVE file, compression used instead of PCM.'),
    'no_riff': (-8, 'Bad WAVE file.'),
    'no_wave': (-8, 'Bad WAVE file.'),
    'too_short': (-8, 'Bad WAVE file.'),
    'data_in_front_of_fmt': (-8, 'Bad WAVE file.'),
    'no_data': (-8, 'Bad WAVE file.'),
    'no_fmt': (-8, 'Bad WAVE file.'),
    'tag_2': (-8, 'Unsupported WAVE file, compression used instead of PCM.'),
    'fmt_size_20': (-8, 'Unsupported WAVE file, compression used instead of PCM.'),
    'ext_tag_in_16_bytes': (-8, 'Unsupported WAVE file, compression used instead of PCM.'),
    'float64': (-8, 'Unsupported WAVE file, compression used instead of PCM.'),
    'bits_12': (-8, 'Unsupported WAVE file, samples not int8, int16 or int32 type.'),
    'float16': (-8, 'Unsupported WAVE file, compression used instead of PCM.'),
    'channels_3': {'channels': 3, 'samplerate': 44100, 'bits_per_sample': 16, 'num_of_samples': 768, 'data_offset': 44, 'n_values': 2304},
    'channels_0': (-4, 'WAVE header with zero channels (ZeroDivisionError in the reference)'),
    'rate_22050': (-8, 'Unsupported sampling frequency.'),
    'bitrate_100': (-8, 'Unsupported bitrate configuration.'),
    'bitrate_64_at_44100_is_fine': {'channels': 2, 'samplerate': 44100, 'bits_per_sample': 16, 'num_of_samples': 1152, 'data_offset': 44, 'n_values': 2304},
    'no_samples': {'channels': 2, 'samplerate': 44100, 'bits_per_sample': 16, 'num_of_samples': 0, 'data_offset': 44, 'n_values': 0},
    'less_than_one_sample': (-8, 'Unsupported WAVE file, samples not int8, int16 or int32 type.'),
}


# ------------------------------------------------------------------------------------------------ CPU
def test_import_info_on_a_table_of_headers(mlib):
    cases = header_cases()
    assert len(cases) >= 45 and len({c[0] for c in cases}) == len(cases)
    for name, data, kbps, want in cases:
        if isinstance(want, dict):
            got = mlib.wav_import_info(data, kbps)
            assert {k: got[k] for k in want} == want, (name, got)
            assert got["bitrate"] == kbps and got["block_align"] == got["channels"] * W.BYTES[got["format"]], (name, got)
            assert got["bits_per_sample"] == 8 * W.BYTES[got["format"]], (name, got)
        else:
            with pytest.raises(mlib.Mp3sError) as e:
                mlib.wav_import_info(data, kbps)
            assert (e.value.code, e.value.text) == want, (name, e.value.code, e.value.text)


def strict_says(mlib, data, kbps):
    try:
        r = mlib.wav_parse(data, kbps)
        return {k: r[k] for k in ("channels", "samplerate", "bits_per_sample", "num_of_samples", "data_offset", "n_values")}
    except mlib.Mp3sError as e:
        return (e.code, e.text)


def test_the_strict_reader_says_what_it_said_before(mlib):
    """the default is untouched: mp3s_wav_parse on the same files, codes and texts as recorded on the parent commit"""
    cases = header_cases()
    assert sorted(STRICT) == sorted(c[0] for c in cases)
    for name, data, kbps, _ in cases:
        assert strict_says(mlib, data, kbps) == STRICT[name], name
    # ... and most of what the import rules read, the strict reader refuses or misreads: that is why the option exists
    assert sum(isinstance(v, tuple) for v in STRICT.values()) > sum(isinstance(c[3], tuple) for c in cases)


def test_wav_import_kernel_keeps_everything_in_registers():
    """the compiler's listing of k_wav_import (one kernel for every format: a uniform switch inside): no scratch, no spill, no LDS,
    eight waves per SIMD -- and its name is no existing kernel's prefix, nor the other way round"""
    from test_build_resources import OTHER_KERNELS, STEP_KERNELS, resource_usage
    usage = resource_usage()
    hits = [k for k in usage if k.startswith("mp3s::k_wav_import")]
    assert hits, sorted(usage)
    for h in hits:
        u = usage[h]
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (h, u)
        assert u["LDS Size [bytes/block]"] == 0 and u["Occupancy [waves/SIMD]"] >= 8, (h, u)
    for k in STEP_KERNELS + OTHER_KERNELS + ["mp3s::k_wav_gather"]:
        assert not "mp3s::k_wav_import".startswith(k) and not k.startswith("mp3s::k_wav_import"), k
    assert len([k for k in usage if k.startswith("mp3s::k_wav_gather")]) == 1


def test_import_info_checks_its_arguments_without_a_gpu(mlib):
    L = mlib.lib()
    w = mlib.WavImport()
    buf = np.frombuffer(W.wav_file(ramp(10, 2, W.S16), W.S16), dtype=np.uint8)
    assert L.mp3s_wav_import_info(None, 100, 128, C.byref(w)) == mlib.E_ARG
    assert L.mp3s_wav_import_info(buf.ctypes.data, 0, 128, C.byref(w)) == mlib.E_ARG
    assert L.mp3s_wav_import_info(buf.ctypes.data, len(buf), 128, None) == mlib.E_ARG
    assert L.mp3s_wav_import_info(buf.ctypes.data, len(buf), 128, C.byref(w)) == 0 and w.n_samples == 10
    assert mlib.Context.OPTIONS["wav_import"] == 20
    with pytest.raises(mlib.Mp3sError) as e:
        mlib.wav_import_info(b"", 128)
    assert e.value.code == mlib.E_ARG


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture
def ictx(mlib):
    """a context of its own with the option on (the session's context stays as every other test expects it)"""
    c = mlib.Context(0)
    assert c.set_option("wav_import", 1) == 0 and c.get_option("wav_import") == 1
    yield c
    c.close()


COUNTS = (1, 1151, 1152, 1153, 2304 + 7, 40 * 1152 + 575)


@pytest.mark.gpu
@pytest.mark.parametrize("channels", (1, 2))
@pytest.mark.parametrize("fmt", W.FORMATS)
def test_the_import_kernel_against_numpy(ictx, mlib, fmt, channels):
    """debug_wav_gather with the option on, int16 for int16: data offsets on all 16 residues mod 16 (odd ones: an odd chunk without its pad byte) x the sample counts around a
    frame's end, the files of one call side by side in the image so that a stream's over-read falls into its neighbour's bytes
    (files of 0x55 among them: a leak shows as 0x5555 or (0x55 - 128) << 8 where zeros belong), the values a conversion gets wrong first"""
    rng = np.random.default_rng(2000 + 10 * fmt + channels)
    special = W.special_samples(fmt)
    neighbour = W.wav_file(np.full(700, 0x55), W.U8, between=[(b"JUNK", b"\x55" * 21)], after=[W.list_chunk(40, fill=0x55)])
    files, want, residues = [], [], set()
    for k in range(16):
        for n in COUNTS:
            s = W.random_samples(rng, n, channels, fmt)
            flat = s.reshape(-1)
            m = min(len(flat), len(special))
            at = int(rng.integers(0, len(flat) - m + 1))
            flat[at:at + m] = special[:m]
            if n > len(special):
                flat[-m:] = special[:m][::-1]                # ... and at the very end, in front of the zero fill
            between = [W.list_chunk(k)]                  # 0 .. 15 bytes; the odd ones without their pad byte: the samples at an odd offset
            size = 16 if k % 2 == 0 or n % 2 else 40     # (every residue with a 16-byte fmt, some of them with other sizes too)
            if k % 2 == 0 and n % 3 == 0:
                size = 18
            f = W.wav_file(s, fmt, rate=(32000, 44100, 48000)[k % 3], fmt_size=size, between=between, pad=False, after=[W.list_chunk(33, fill=0x55)] if n % 2 else [])
            info = mlib.wav_import_info(f, 128)
            assert info["n_samples"] == n and info["format"] == fmt and info["channels"] == channels
            assert info["data_offset"] == W.data_offset_of(between=between, fmt_size=size, pad=False)
            if size == 16:
                residues.add(info["data_offset"] % 16)
            files.append(f)
            want.append(W.stereo_frames(s, fmt))
    assert sorted(residues) == list(range(16))
    order = rng.permutation(len(files))
    batch, expect = [], []
    for i, o in enumerate(order):
        batch.append(files[o])
        expect.append(want[o])
        if i % 5 == 0:
            batch.append(neighbour)
            expect.append(W.stereo_frames(np.full(700, 0x55), W.U8))
    got = ictx.debug_wav_gather(batch)
    assert got.shape == (sum(len(e) for e in expect) // 1152, 1152, 2)
    at = 0
    for i, e in enumerate(expect):
        n = len(e) // 1152
        g = got[at:at + n].reshape(-1, 2)
        if not np.array_equal(g, e):
            bad = np.argwhere(g != e)
            raise AssertionError((W.NAMES[fmt], channels, "stream", i, "of", len(e), "rows; first bad (row, channel)", bad[0].tolist(),
                                  "got", g[bad[0][0]].tolist(), "want", e[bad[0][0]].tolist(), "bad values", len(bad)))
        at += n
    # a file alone (the slack behind the image instead of a neighbour), the specials alone
    for o in (0, 5, len(files) - 1):
        assert np.array_equal(ictx.debug_wav_gather([files[o]]).reshape(-1, 2), want[o]), o
    alone = special if channels == 1 else np.stack([special, special[::-1]], axis=1)
    assert np.array_equal(ictx.debug_wav_gather([W.wav_file(alone, fmt)]).reshape(-1, 2), W.stereo_frames(alone, fmt))


def from_int16(pcm, fmt, rng):
    """int16 audio in the format's own range, with low bits the conversion has to drop"""
    p = pcm.astype(np.int64)
    if fmt == W.U8:
        return (p >> 8) + 128
    if fmt == W.S16:
        return p
    if fmt == W.S24:
        return (p << 8) | rng.integers(0, 256, size=p.shape, dtype=np.int64)
    if fmt == W.S32:
        return (p << 16) | rng.integers(0, 65536, size=p.shape, dtype=np.int64)
    return ((p + rng.random(size=p.shape) * 0.8 - 0.4) / 32768.0).astype(np.float32)


def import_list(mlib):
    """-> [(file, bitrate, hide bits or None, (samples, format, rate) or None for a file both readers refuse)]: all formats, mono and
    stereo, three rates, several bitrates, fmt of 16 / 18 / 40 bytes, chunks in front of the samples, lengths that are no whole frames,
    messages short / too long / beyond 1 024 bits, canonical files among them"""
    from synth_pcm import synth_pcm
    rng = np.random.default_rng(77)
    bits = lambda m: np.array(mlib.message_frame(m), dtype=np.uint8)
    out = []

    def add(frames, cut, fmt, ch, rate, kbps, hide, seed, **kw):
        pcm = synth_pcm(frames, seed=seed, rate=rate)
        pcm = pcm[:len(pcm) - cut]
        s = from_int16(pcm if ch == 2 else pcm[:, 0], fmt, rng)
        out.append((W.wav_file(s, fmt, rate=rate, **kw), kbps, hide, (s, fmt, rate)))

    add(40, 0, W.S16, 2, 44100, 128, None, 500)                                                       # 0: canonical
    add(41, 577, W.S16, 2, 44100, 128, bits("hello"), 501, between=[W.list_chunk(3)])                 # 1: 16-bit stereo, a partial last frame
    add(60, 1, W.S16, 1, 44100, 128, bits("mono"), 502)                                               # 2: mono
    add(300, 100, W.S24, 2, 48000, 192, bits("a longer file"), 503, fmt_size=40, between=[W.list_chunk(200)])   # 3: what most tools write for 24-bit
    add(25, 0, W.S24, 1, 44100, 320, bits("x" * 200), 504, before=[(b"bext", b"b" * 601)])           # 4: too long for 25 frames
    add(33, 1151, W.S32, 2, 32000, 64, None, 505, fmt_size=18)                                        # 5
    add(500, 3, W.S32, 1, 44100, 128, bits("long " * 60), 506, between=[W.list_chunk(70000)])         # 6: > 1 024 bits: the variants
    add(80, 200, W.F32, 2, 44100, 128, bits("float"), 507, fmt_size=40, valid_bits=32)                # 7
    add(1, 1000, W.F32, 1, 48000, 192, np.zeros(0, dtype=np.uint8), 508, between=[W.list_chunk(1)])   # 8: 152 samples, an empty bit string
    add(50, 7, W.U8, 2, 44100, 128, bits("eight"), 509, between=[W.list_chunk(2)])                    # 9
    add(120, 0, W.U8, 1, 32000, 64, None, 510, after=[W.list_chunk(500, fill=0x55)])                  # 10: bytes behind the samples are never audio
    add(30, 0, W.S16, 2, 48000, 192, bits("canonical too"), 511, between=[W.list_chunk(6)])           # 11: canonical, in a group with 3 and 8
    add(70, 0, W.S32, 2, 44100, 320, None, 512, fmt_size=40, valid_bits=20)                           # 12
    ok = from_int16(synth_pcm(4, seed=513), W.S24, rng)
    out.append((W.wav_file(ok, W.S24, rate=22050), 128, bits("no"), None))                            # 13: a rate both refuse
    out.append((W.wav_file(ok, W.S24), 100, None, None))                                              # 14: a bitrate both refuse
    out.append((W.wav_file(ok, W.S24, channels=3), 128, None, None))                                  # 15: three channels
    return out


def oracle(ctx, mlib, files):
    """what the strict path, option off, makes of the canonical 16-bit stereo WAV of the converted samples; the Mp3sError both readers raise"""
    assert ctx.get_option("wav_import") == 0
    want = []
    for f, kbps, hide, src in files:
        if src is None:
            with pytest.raises(mlib.Mp3sError) as e:
                mlib.wav_import_info(f, kbps)
            want.append(e.value)
        else:
            want.append(ctx.encode_file(wav_bytes(W.stereo_frames(src[0], src[1]), src[2]), kbps, hide))
    return want


def _same_or_refused(mlib, a, b, what, text=None):
    _same(mlib, a, b, what)
    if isinstance(b, Exception) and text is not None:
        assert text == b.text, (what, text, b.text)


@pytest.mark.gpu
def test_every_entry_point_with_the_option_on_equals_the_oracle(mlib):
    files = import_list(mlib)
    ctx = mlib.Context(0)
    try:
        want = oracle(ctx, mlib, files)
        assert [w.code for w in want if isinstance(w, Exception)] == [E_EXIT, E_EXIT, E_UNSUPPORTED]
        assert want[4]["too_long"] and not want[1]["too_long"] and len(files[6][2]) > 1024
        assert all(w["channels"] == 2 for w in want if not isinstance(w, Exception))            # mono in: a stereo MP3 out
        assert [w["n_frames"] for w in want[:3]] == [40, 41, 60] and want[8]["n_frames"] == 1
        # the strict reader takes none of 1 .. 10 and 12 as they are (refused, or read as something else)
        ctx.set_option("wav_import", 1)
        # (a) encode_file, one by one; the refused ones with the import rules' code AND text
        for i, (f, kbps, hide, _) in enumerate(files):
            try:
                got = ctx.encode_file(f, kbps, hide)
            except mlib.Mp3sError as e:
                got = e
            _same_or_refused(mlib, got, want[i], ("encode_file", i), getattr(got, "text", None))
        # (b) encode_files: one mixed list, one call
        got = ctx.encode_files([f[0] for f in files], [f[1] for f in files], hide_bits=[f[2] for f in files])
        assert len(got) == len(files)
        for i, (a, b) in enumerate(zip(got, want)):
            _same(mlib, a, b, ("encode_files", i))
        # ... status == NULL: the first refused file fails the call with its own code and text
        L = mlib.lib()
        bufs = [np.frombuffer(files[i][0], dtype=np.uint8) for i in (2, 15, 13)]
        ptr = (C.c_void_p * 3)(*[b.ctypes.data for b in bufs])
        lens = (C.c_size_t * 3)(*[len(b) for b in bufs])
        kb = (C.c_int32 * 3)(128, 128, 128)
        out, owner = (mlib.File * 3)(), C.c_void_p()
        assert L.mp3s_encode_files(ctx.handle, ptr, lens, 3, kb, None, None, C.byref(owner), out, None) == E_UNSUPPORTED
        assert L.mp3s_last_error().decode() == "more than two channels" and owner.value is None
        # (c) the pipe, created with the option on: jobs of one group that fit the slot take the stages, the rest goes the other way
        job = lambda idx: ("enc", ([files[i][0] for i in idx], [files[i][1] for i in idx], [files[i][2] for i in idx]))
        fits = [job([0, 1, 2, 9]), job([3, 11]), job([6]), job([5]), job([7]), job([4]), job([8, 3]), job([10])]
        other = [job([1, 3]), job([13]), job([2, 14, 0]), job([15, 12])]          # two groups; refused files
        pipe = mlib.Pipe(ctx, depth=3, max_job_bytes=4 << 20, scan_threads=2)
        try:
            res = _drain(pipe, fits)
            st = pipe.stats()
            assert st["slow"] == 0 and st["fast"] + st["resolved"] == st["collected"] == len(fits), st
            res += _drain_more(pipe, other, len(fits))
            st = pipe.stats()
            assert st["slow"] == len(other), st
        finally:
            pipe.close()
        index = [[0, 1, 2, 9], [3, 11], [6], [5], [7], [4], [8, 3], [10], [1, 3], [13], [2, 14, 0], [15, 12]]
        for k, (r, idx) in enumerate(zip(res, index)):
            assert len(r) == len(idx)
            for a, i in zip(r, idx):
                _same(mlib, a, want[i], ("pipe", k, i))
        # A slot is made for max_job_bytes of MP3 and has an image of 48 x that: at 32 kHz and 32 kbit/s a frame is 144 bytes of MP3, so
        # 5 800 frames (0.8 MB) fit a 1 MB slot whatever they are made of -- as 8-bit mono (6.7 MB of WAV) and as 16-bit stereo they
        # fit its image of 50.6 MB too, as 32-bit stereo (53.5 MB) they do not: that job goes the other way, same bytes
        from synth_pcm import synth_pcm
        rng = np.random.default_rng(5)
        pcm = synth_pcm(5800, seed=520, rate=32000)
        u8, s16, s32 = from_int16(pcm[:5800 * 1152 - 9, 0], W.U8, rng), pcm[:3000 * 1152 - 1], from_int16(pcm[:5800 * 1152 - 5], W.S32, rng)
        trio = [(W.wav_file(u8, W.U8, rate=32000), (u8, W.U8)), (W.wav_file(s32, W.S32, rate=32000), (s32, W.S32)), (W.wav_file(s16, W.S16, rate=32000), (s16, W.S16))]
        ctx.set_option("wav_import", 0)
        w3 = [ctx.encode_file(wav_bytes(W.stereo_frames(*src), 32000), 32) for _, src in trio]
        ctx.set_option("wav_import", 1)
        pipe = mlib.Pipe(ctx, depth=2, max_job_bytes=1 << 20, scan_threads=1)
        try:
            r3 = _drain(pipe, [("enc", ([f], [32], [None])) for f, _ in trio])
            st = pipe.stats()
        finally:
            pipe.close()
        assert st["slow"] == 1 and st["collected"] == 3, st
        for k, (r, w) in enumerate(zip(r3, w3)):
            _same(mlib, r[0], w, ("1 MB pipe", k))
        # a pipe keeps the value its context had when it was created
        pipe = mlib.Pipe(ctx, depth=2, max_job_bytes=1 << 20, scan_threads=1)
        ctx.set_option("wav_import", 0)
        try:
            r4 = _drain(pipe, [job([2, 0]), job([2, 13])])
        finally:
            pipe.close()
        _same(mlib, r4[0][0], want[2], "kept, fast")
        _same(mlib, r4[1][0], want[2], "kept, slow")
        assert isinstance(r4[1][1], mlib.Mp3sError) and r4[1][1].code == E_EXIT
        # option off on the same context afterwards: mono and 24-bit are refused again with today's codes
        for i, code in ((2, E_UNSUPPORTED), (3, E_EXIT), (4, E_EXIT), (7, E_EXIT)):
            with pytest.raises(mlib.Mp3sError) as e:
                ctx.encode_file(files[i][0], files[i][1], files[i][2])
            assert e.value.code == code, (i, e.value)
        assert e.value.text == COMPRESSED
        back = ctx.encode_files([files[2][0], files[0][0], files[3][0]], 128)
        assert isinstance(back[0], mlib.Mp3sError) and back[0].code == E_UNSUPPORTED and isinstance(back[2], mlib.Mp3sError) and back[2].code == E_EXIT
        _same(mlib, back[1], want[0], "off again")
        pipe = mlib.Pipe(ctx, depth=2, max_job_bytes=1 << 20, scan_threads=1)
        try:
            r5 = _drain(pipe, [job([2])])
        finally:
            pipe.close()
        assert isinstance(r5[0][0], mlib.Mp3sError) and r5[0][0].code == E_UNSUPPORTED
    finally:
        ctx.close()


def _drain_more(pipe, jobs, first_ticket):
    """_drain for a pipe that has handed out tickets before"""
    out, nxt = [], 0
    while len(out) < len(jobs):
        while nxt < len(jobs):
            a = jobs[nxt][1]
            t = pipe.submit_encode(a[0], a[1], hide_bits=a[2])
            if t is None:
                break
            assert t == first_ticket + nxt
            nxt += 1
        t, res = pipe.collect()
        assert t == first_ticket + len(out)
        out.append(res)
    assert pipe.collect() is None
    return out


@pytest.mark.gpu
def test_strict_files_give_the_same_bytes_with_the_option_on(mlib):
    """the compatibility rule: what the strict reader accepts of test_encode_batch.mixed_list is 16-bit stereo in whole frames -- the
    same bytes and fields with the option on as with it off, alone, as a list and through the pipe"""
    files = mixed_list(mlib)
    ctx = mlib.Context(0)
    try:
        off = []
        for f in files:
            try:
                off.append(ctx.encode_file(*f))
            except mlib.Mp3sError as e:
                off.append(e)
        keep = [i for i, w in enumerate(off) if not isinstance(w, Exception)]
        assert len(keep) == 10
        ctx.set_option("wav_import", 1)
        for i in keep:
            info = mlib.wav_import_info(files[i][0], files[i][1])
            assert info["format"] == W.S16 and info["channels"] == 2 and info["n_samples"] % 1152 == 0, i
            _same(mlib, ctx.encode_file(*files[i]), off[i], ("alone", i))
        got = ctx.encode_files([files[i][0] for i in keep], [files[i][1] for i in keep], hide_bits=[files[i][2] for i in keep])
        for i, a in zip(keep, got):
            _same(mlib, a, off[i], ("list", i))
        pipe = mlib.Pipe(ctx, depth=2, max_job_bytes=4 << 20, scan_threads=1)
        try:
            res = _drain(pipe, [("enc", ([files[i][0]], [files[i][1]], [files[i][2]])) for i in keep])
            st = pipe.stats()
        finally:
            pipe.close()
        assert st["slow"] == 0, st
        for i, r in zip(keep, res):
            _same(mlib, r[0], off[i], ("pipe", i))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_canonical_files_keep_the_gather(mlib):
    """with the option on, 16-bit stereo files of whole frames still run k_wav_gather and only the rest k_wav_import: the traced
    child says which kernel took how many streams of each batch"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wav_import_trace_child.py")],
                       env=dict(os.environ, MP3S_TRACE="1", MP3S_WAV_IMPORT="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("batch ") or "k_wav_import" in ln]
    say = lambda g, i: f"mp3s:   encode_files: {g} streams through k_wav_gather, {i} through k_wav_import"
    assert lines == ["batch canonical", say(2, 0), "batch mixed", say(2, 3), "batch other", say(0, 3)], lines


FACADE_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
from mp3stego import Steganography
Steganography(quiet=True).encode_wav_to_mp3(sys.argv[2], sys.argv[3], 128)
"""


@pytest.mark.gpu
def test_the_facade_gets_the_option_from_the_environment(ctx, mlib, tmp_path):
    from synth_pcm import synth_pcm
    rng = np.random.default_rng(9)
    s = from_int16(synth_pcm(20, seed=530)[:20 * 1152 - 300, 0], W.S24, rng)
    wav = W.wav_file(s, W.S24, fmt_size=40, between=[W.list_chunk(201)])
    assert ctx.get_option("wav_import") == 0
    want = ctx.encode_file(wav_bytes(W.stereo_frames(s, W.S24), 44100), 128)
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.mp3")
    with open(src, "wb") as f:
        f.write(wav)
    env = {k: v for k, v in os.environ.items() if k != "MP3S_WAV_IMPORT"}
    run = lambda e: subprocess.run([sys.executable, "-c", FACADE_CHILD, os.path.join(ROOT, "mp3-steganography-lib_amd"), src, dst],
                                   env=e, capture_output=True, text=True, timeout=300)
    r = run(env)
    assert r.returncode == 1 and r.stderr.strip().splitlines()[-1] == COMPRESSED and not os.path.exists(dst), (r.returncode, r.stderr[-2000:])
    r = run(dict(env, MP3S_WAV_IMPORT="1"))
    assert r.returncode == 0, r.stderr[-4000:]
    with open(dst, "rb") as f:
        assert f.read() == bytes(want["data"])
    # what both refuse keeps the reference's exit text with the variable set
    with open(src, "wb") as f:
        f.write(W.wav_file(s, W.S24, rate=22050))
    os.remove(dst)
    r = run(dict(env, MP3S_WAV_IMPORT="1"))
    assert r.returncode == 1 and r.stderr.strip().splitlines()[-1] == RATE and not os.path.exists(dst), (r.returncode, r.stderr[-2000:])
