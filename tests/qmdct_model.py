"""The QMDCT features and batches of include/mp3s.h, section (vi-g), restated in numpy: the yardstick of tests/test_qmdct.py.  Its
input is host arrays -- for a file, parse_stream(data)["is"] -- and it runs no code of the feature."""
import numpy as np

T = 4                        # MP3S_QMDCT_T
B = 2 * T + 1


def rows_of(is_, nch):
    """int16 [n_frames][2 gr][2 ch][576] -> a = |q| as int64 [nch][G = 2 n_frames][576], q[c][g][k] = is[g >> 1][g & 1][c][k]"""
    return np.abs(spectra(is_, nch).astype(np.int64))


def spectra(is_, nch):
    """q itself, int16 [nch][G][576]"""
    is_ = np.asarray(is_, dtype=np.int16)
    n = is_.size // 2304
    return is_.reshape(n, 2, 2, 576).transpose(2, 0, 1, 3).reshape(2, 2 * n, 576)[:nch]


def pair_table(d0, d1):
    """the 9 x 9 counts of the pairs (d0, d1) of clipped differences, both already in -T .. T"""
    return np.bincount(((d0 + T) * B + (d1 + T)).reshape(-1), minlength=B * B).reshape(B, B).astype(np.int64)


def channel_features(a, K):
    """a: int64 [G][576] -> dict(hist [16], intra [9][9], inter [9][9], max_abs, bandwidth) over the lines k < K"""
    a = a[:, :K]
    G = a.shape[0]
    hist = np.bincount(np.minimum(a, 15).reshape(-1), minlength=16).astype(np.int64)
    dh = np.clip(a[:, :-1] - a[:, 1:], -T, T)                        # [G][K - 1]
    intra = pair_table(dh[:, :-1], dh[:, 1:]) if K >= 3 and G else np.zeros((B, B), dtype=np.int64)
    dv = np.clip(a[:-1] - a[1:], -T, T) if G >= 2 else np.zeros((0, K), dtype=np.int64)   # [G - 1][K]
    inter = pair_table(dv[:-1], dv[1:]) if G >= 3 else np.zeros((B, B), dtype=np.int64)
    nz = np.nonzero(a.any(axis=0))[0] if G else np.zeros(0, dtype=np.int64)
    return {"hist": hist, "intra": intra, "inter": inter, "max_abs": int(a.max()) if a.size else 0, "bandwidth": int(nz[-1]) + 1 if len(nz) else 0}


def features(is_, nch, K=576):
    """the dict Context.qmdct_features gives for one stream, without the header fields of a file (sampling_rate, kbps)"""
    a = rows_of(is_, nch)
    per = [channel_features(a[c], K) for c in range(nch)]
    out = {k: np.stack([np.asarray(p[k], dtype=np.int64) for p in per]) for k in ("hist", "intra", "inter", "max_abs", "bandwidth")}
    out.update(n_frames=a.shape[1] // 2, n_granules=a.shape[1], channels=nch, n_lines=K)
    return out


def record(is_, nch, K, dtype):
    """the mp3s_qmdct_features record (numpy `dtype`) k_qmdct_features writes for the stream: sampling_rate and kbps 0, ch[1] of mono zero"""
    f = features(is_, nch, K)
    r = np.zeros((), dtype=dtype)
    for c in range(nch):
        for k in ("hist", "intra", "inter", "max_abs", "bandwidth"):
            r["ch"][c][k] = f[k][c]
    r["n_frames"], r["channels"], r["n_lines"] = f["n_frames"], nch, K
    return r


def identities(f, K):
    """the three sums that follow from the definitions"""
    G = f["n_granules"]
    for c in range(f["channels"]):
        assert int(f["hist"][c].sum()) == G * K, (c, "hist")
        assert int(f["intra"][c].sum()) == G * max(K - 2, 0), (c, "intra")
        assert int(f["inter"][c].sum()) == max(G - 2, 0) * K, (c, "inter")


def batch_slot(is_, nch, C, Gt, first_granule):
    """int16 [C][Gt][576]: rows first_granule .. of the stream, zeros behind them and in plane 1 of a mono stream"""
    q = spectra(is_, nch)
    out = np.zeros((C, Gt, 576), dtype=np.int16)
    valid = int(min(max(q.shape[1] - first_granule, 0), Gt))
    out[:nch, :valid] = q[:, first_granule:first_granule + valid]
    return out, valid
