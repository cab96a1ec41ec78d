"""Helper of tests/test_wav_resample.py: the resampler of the "wav_resample" option (include/mp3s.h, mp3s_wav_resample_info) restated
in numpy -- target rate, ratio, filter, tap table and the integer output rule -- the oracle of every comparison there."""
from math import gcd

import numpy as np

RATES = (32000, 44100, 48000)
BH = (0.35875, 0.48829, 0.14128, 0.01168)          # 4-term Blackman-Harris


def target_rate(rate, mode):
    """mode 1: a supported rate stays; else the supported rates >= the file's (all three above 48 000), smallest L, ties to the highest"""
    if mode != 1:
        return mode
    if rate in RATES:
        return rate
    cand = [r for r in RATES if r >= rate] or list(RATES)
    return min(cand, key=lambda r: (r // gcd(r, rate), -r))


def plan(rate, mode):
    """-> dict(out_rate, L, M, taps, half) or None where the resampler refuses the rate"""
    if rate <= 0:
        return None
    out = target_rate(rate, mode)
    g = gcd(out, rate)
    L, M = out // g, rate // g
    H = 16 if L >= M else -(-16 * M // L)                # ceil(16 / rho), rho = min(1, L / M)
    if L > 1280 or 2 * H > 256:
        return None
    return dict(out_rate=out, L=L, M=M, taps=2 * H, half=H)


def counts(n_in, L, M):
    n_out = -(-n_in * L // M)
    return n_out, -(-n_out // 1152)


def prototype(L, M):
    """h(t) at every tap of every phase, float64 [L][T]: t = k - H + 1 - p / L"""
    H = 16 if L >= M else -(-16 * M // L)
    rho = 1.0 if L >= M else L / M
    fc = 0.95 * rho
    k = np.arange(2 * H, dtype=np.float64)[None, :]
    p = np.arange(L, dtype=np.float64)[:, None]
    t = (k - H + 1) - p / L
    u = t / H
    w = BH[0] + BH[1] * np.cos(np.pi * u) + BH[2] * np.cos(2 * np.pi * u) + BH[3] * np.cos(3 * np.pi * u)
    w = np.where((u > -1.0) & (u <= 1.0), w, 0.0)
    return fc * np.sinc(fc * t) * w                        # np.sinc(x) = sin(pi x) / (pi x)


def model_taps(L, M):
    """-> (c int64 [L][T], where int [L] = the tap of each phase that took the residual, residual int64 [L])"""
    c = np.rint(prototype(L, M) * 32768.0).astype(np.int64)
    where = np.argmax(c, axis=1)                           # the first of equal taps
    residual = 32768 - c.sum(axis=1)
    c[np.arange(L), where] += residual
    return c, where, residual


def _gathered(x, L, M, T, lo=0, hi=None):
    """the T input rows under every output row lo .. hi - 1 (all of them by default), and the rows' phases"""
    x = np.asarray(x)
    H = T // 2
    n_out, _ = counts(len(x), L, M)
    n = np.arange(lo, n_out if hi is None else min(hi, n_out), dtype=np.int64)
    i0, p = n * M // L, n * M % L
    pad = np.zeros((H + 1,) + x.shape[1:], dtype=x.dtype)
    xp = np.concatenate([pad, x, pad])                     # xp[i + H + 1] = x[i], zeros outside
    idx = (i0 + 2)[:, None] + np.arange(T, dtype=np.int64)[None, :]      # i0 - H + 1 + k, + H + 1
    return xp[idx], p


def resample(x, L, M, taps):
    """x int16 [n] or [n, 2] -> int16 of ceil(n L / M) rows by the output rule, int64 sums, with the tap table given (the library's)"""
    taps = np.asarray(taps, dtype=np.int64)
    x = np.asarray(x, dtype=np.int64)
    n_out, _ = counts(len(x), L, M)
    out = []
    for lo in range(0, n_out, 1 << 17):                    # (in pieces: the gathered rows of a long stream are T times its size)
        g, p = _gathered(x, L, M, taps.shape[1], lo, lo + (1 << 17))
        c = taps[p]
        s = (g * (c if g.ndim == 2 else c[:, :, None])).sum(axis=1)
        out.append(np.clip((s + (1 << 14)) >> 15, -32768, 32767).astype(np.int16))
    return np.concatenate(out)


def resample_ideal(x, L, M):
    """the same sums with the float64 prototype instead of the rounded taps, unrounded and unclamped"""
    h = prototype(L, M)
    g, p = _gathered(np.asarray(x, dtype=np.float64), L, M, h.shape[1])
    c = h[p]
    return (g * (c if g.ndim == 2 else c[:, :, None])).sum(axis=1)


def frames_of(rows):
    """int16 [n, 2] -> the stream's frames of the PCM buffer: zero-filled to a whole frame"""
    out = np.zeros((-(-len(rows) // 1152) * 1152, 2), dtype=np.int16)
    out[:len(rows)] = rows
    return out
