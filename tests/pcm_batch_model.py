"""numpy's side of the PCM batch calls (include/mp3s.h section vi-f): what k_pcm_batch and k_pcm_unbatch must leave, written from the
rules of the header alone.  Nothing here runs the library."""
import numpy as np

DTYPES = {"i16": np.int16, "f32": np.float32}


def plane_rows(x, channels, fmt):
    """int16 rows [n][nch] -> the batch's planes [channels][n] of fmt.  The downmix is computed in int64."""
    x = np.asarray(x, dtype=np.int16).astype(np.int64)
    nch = x.shape[1]
    if nch == channels:
        p, scale = x.T, 32768
    elif nch == 1:
        p, scale = np.repeat(x.T, 2, axis=0), 32768
    else:
        s = x[:, 0] + x[:, 1]
        p, scale = (s[None, :] >> 1, 32768) if fmt == "i16" else (s[None, :], 65536)   # >> on int64: arithmetic, so floor
    if fmt == "i16":
        assert p.min(initial=0) >= -32768 and p.max(initial=0) <= 32767
        return p.astype(np.int16)
    out = p.astype(np.float32) / np.float32(scale)       # (|p| < 2^17: exact in float32, and so is the division by a power of two)
    assert np.array_equal(out.astype(np.float64) * scale, p)
    return out


def batch(streams, first_rows, T, channels, fmt, n_slots=None, slots=None):
    """streams: per item int16 [rows][nch], or None (a failed file: a zero slot) -> (batch [n_slots][channels][T], valid rows per item)"""
    slots = list(range(len(streams))) if slots is None else list(slots)
    out = np.zeros((len(streams) if n_slots is None else n_slots, channels, T), dtype=DTYPES[fmt])
    valid = []
    for x, first, b in zip(streams, first_rows, slots):
        if x is None:
            valid.append(0)
            continue
        v = int(min(max(len(x) - first, 0), T))
        valid.append(v)
        if v:
            out[b, :, :v] = plane_rows(x[first:first + v], channels, fmt)
    return out, valid


def float_to_i16(x):
    """the encoder's int16 of a float32 sample: clamp(rint(x * 32768)), half to even, NaN -> 0"""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.rint(x * np.float32(32768))
        y = np.clip(y, np.float32(-32768), np.float32(32767))
    return np.where(np.isnan(x), np.float32(0), y).astype(np.int16)


def frames(item, n_rows):
    """one item [C][T] of a batch and its length -> the encoder's rows [ceil(n_rows / 1152) * 1152][2] int16: mono into both channels,
    zeros from n_rows on whatever the item holds there"""
    item = np.asarray(item)
    v = item[:, :n_rows]
    v = float_to_i16(v) if item.dtype == np.float32 else v.astype(np.int16)
    out = np.zeros(((n_rows + 1151) // 1152 * 1152, 2), dtype=np.int16)
    out[:n_rows, 0] = v[0]
    out[:n_rows, 1] = v[-1]
    return out


# the edge values of the two rules, with what they must give
DOWNMIX_EDGES = [((-32768, -32768), -32768, -1.0), ((32767, 32767), 32767, 32767 / 32768), ((-1, 0), -1, -1 / 65536), ((1, 0), 0, 1 / 65536),
                 ((32767, -32768), -1, -1 / 65536)]
FLOAT_EDGES = [((2 + 0.5) / 32768, 2), ((3 + 0.5) / 32768, 4), ((-2 - 0.5) / 32768, -2), ((-3 - 0.5) / 32768, -4), (1.0, 32767), (-1.0, -32768),
               (np.inf, 32767), (-np.inf, -32768), (np.nan, 0), (1e-40, 0), (-1e-40, 0), (0.999984, 32767), (32766.5 / 32768, 32766)]
