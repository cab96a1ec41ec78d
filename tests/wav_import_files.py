"""Helpers of tests/test_wav_import.py: a WAV writer that takes sample format, channel count, `fmt ` size and a chunk list, and
the conversion rules of the "wav_import" option (include/mp3s.h, mp3s_wav_import_info) as numpy lines -- the oracle."""
import struct

import numpy as np

U8, S16, S24, S32, F32 = 1, 2, 3, 4, 5
FORMATS = (U8, S16, S24, S32, F32)
NAMES = {U8: "u8", S16: "s16", S24: "s24", S32: "s32", F32: "f32"}
BYTES = {U8: 1, S16: 2, S24: 3, S32: 4, F32: 4}
PCM_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")     # KSDATAFORMAT_SUBTYPE_*: the tag, then these 14 bytes


def sample_bytes(samples, fmt):
    """samples: [n] or [n, ch]; u8: 0..255, s16/s24/s32: signed values of that width, f32: float32 -> little-endian bytes"""
    a = np.asarray(samples)
    if fmt == U8:
        return a.astype(np.uint8).tobytes()
    if fmt == S16:
        return a.astype("<i2").tobytes()
    if fmt == S24:
        b = a.astype("<i4").reshape(-1).view(np.uint8).reshape(-1, 4)
        return np.ascontiguousarray(b[:, :3]).tobytes()
    if fmt == S32:
        return a.astype("<i4").tobytes()
    return a.astype("<f4").tobytes()


def to_int16(samples, fmt):
    """the rules of section "samples to int16", one numpy line each"""
    a = np.asarray(samples)
    if fmt == U8:
        return ((a.astype(np.int32) - 128) << 8).astype(np.int16)
    if fmt == S16:
        return a.astype(np.int16)
    if fmt == S24:
        return (a.astype(np.int32) >> 8).astype(np.int16)
    if fmt == S32:
        return (a.astype(np.int32) >> 16).astype(np.int16)
    x = a.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.clip(np.rint(x * np.float32(32768.0)), np.float32(-32768.0), np.float32(32767.0))
    return np.where(np.isnan(x), np.float32(0), y).astype(np.int16)


def stereo_frames(samples, fmt):
    """-> int16 [frames * 1152, 2]: converted, mono in both channels, the last frame filled with zeros"""
    v = to_int16(samples, fmt)
    if v.ndim == 1 or v.shape[1] == 1:
        v = np.stack([v.reshape(-1), v.reshape(-1)], axis=1)
    n = v.shape[0]
    out = np.zeros(((n + 1151) // 1152 * 1152, 2), dtype=np.int16)
    out[:n] = v
    return out


def chunk(cid, payload, pad=True):
    """a RIFF chunk: id, size, payload, pad byte after an odd size (pad=False: left out, as some writers do)"""
    return cid + struct.pack("<I", len(payload)) + payload + (b"\0" if pad and len(payload) & 1 else b"")


def fmt_chunk(fmt, channels, rate, size=16, tag=None, bits=None, valid_bits=None, block_align=None):
    bits = BYTES[fmt] * 8 if bits is None else bits
    real = 3 if fmt == F32 else 1
    tag = (0xFFFE if size == 40 else real) if tag is None else tag
    align = channels * (bits // 8) if block_align is None else block_align
    body = struct.pack("<HHIIHH", tag, channels, rate, rate * align, align, bits)
    if size == 18:
        body += struct.pack("<H", 0)
    elif size == 40:
        body += struct.pack("<HHIH", 22, bits if valid_bits is None else valid_bits, 3 if channels == 2 else 4, real) + PCM_GUID_TAIL
    assert len(body) == size, (len(body), size)
    return b"fmt " + struct.pack("<I", size) + body


def wav_file(samples, fmt, rate=44100, channels=None, fmt_size=16, before=(), between=(), after=(), declared=None, cut=0, pad=True, **fmt_args):
    """a WAV file: RIFF WAVE [before...] fmt [between...] data [after...]; before / between / after = [(id, payload)], declared =
    the size the data chunk states (None: the truth), cut = bytes taken off the end of the file, pad=False = the chunks between fmt and
    data without the pad byte of an odd size"""
    a = np.asarray(samples)
    channels = (1 if a.ndim == 1 else a.shape[1]) if channels is None else channels
    data = sample_bytes(a, fmt)
    body = b"WAVE" + b"".join(chunk(*c) for c in before) + fmt_chunk(fmt, channels, rate, fmt_size, **fmt_args) + b"".join(chunk(*c, pad=pad) for c in between)
    body += b"data" + struct.pack("<I", len(data) if declared is None else declared) + data + (b"\0" if len(data) & 1 else b"")
    body += b"".join(chunk(*c) for c in after)
    out = b"RIFF" + struct.pack("<I", len(body)) + body
    return out[:len(out) - cut] if cut else out


def data_offset_of(before=(), between=(), fmt_size=16, pad=True):
    size = lambda c, p: 8 + len(c[1]) + (len(c[1]) & 1 if p else 0)
    return 12 + sum(size(c, True) for c in before) + 8 + fmt_size + sum(size(c, pad) for c in between) + 8


def list_chunk(k, fill=None):
    return (b"LIST", bytes(range(1, k + 1)) if fill is None else bytes([fill]) * k) if k < 256 else (b"LIST", bytes((i * 7 + 1) & 0xFF for i in range(k)))


def random_samples(rng, n, channels, fmt):
    shape = (n,) if channels == 1 else (n, channels)
    if fmt == U8:
        return rng.integers(0, 256, size=shape, dtype=np.int64)
    if fmt == S16:
        return rng.integers(-32768, 32768, size=shape, dtype=np.int64)
    if fmt == S24:
        return rng.integers(-(1 << 23), 1 << 23, size=shape, dtype=np.int64)
    if fmt == S32:
        return rng.integers(-(1 << 31), 1 << 31, size=shape, dtype=np.int64)
    return (rng.random(size=shape) * 2.4 - 1.2).astype(np.float32)       # beyond +-1 now and then


def special_samples(fmt):
    """the values a conversion gets wrong first"""
    if fmt == U8:
        return np.array([0, 127, 128, 255, 1, 129, 254, 64], dtype=np.int64)
    if fmt == S16:
        return np.array([-32768, 32767, 0, -1, 1, 255, 256, -256], dtype=np.int64)
    if fmt == S24:
        return np.array([-(1 << 23), (1 << 23) - 1, 0, -1, 255, 256, -256, -257, 0x7FFF00, 0x0000FF, -0x800000 + 255], dtype=np.int64)
    if fmt == S32:
        return np.array([-(1 << 31), (1 << 31) - 1, 0, -1, 65535, 65536, -65536, -65537, 0x7FFF0000, 0x0000FFFF], dtype=np.int64)
    k = np.array([0, 1, 2, 3, 100, 101, 32766, -1, -2, -3, -32768, -32767], dtype=np.float32)
    ties = np.concatenate([(k + np.float32(0.5)) / np.float32(32768), (k - np.float32(0.5)) / np.float32(32768)]).astype(np.float32)
    tiny = np.array([1e-45, -1e-45, 1e-39, -1e-39, 1.17549435e-38], dtype=np.float32)       # denormals and the smallest normal
    other = np.array([1.0, -1.0, 0.0, -0.0, 1.5, -1.5, 1e30, -1e30, np.inf, -np.inf, np.nan, -np.nan,
                      32767.0 / 32768, 32767.5 / 32768, 0.99999, -0.99999, 1.0 / 32768, 0.49 / 32768, 0.51 / 32768], dtype=np.float32)
    return np.concatenate([ties, tiny, other])
