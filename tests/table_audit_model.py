"""The table audit's rule (include/mp3s.h, section vi-e) restated in numpy and plain Python: the yardstick of tests/test_table_audit.py.

It runs no code of the feature.  Samples and side records come from the host-only calls parse_stream (`is`) and scan_stream (side
records); the tables from tests/golden/g1_tables.npz (enc_hlen_*, enc_huff_meta = [xlen, ylen, linbits, linmax] per book,
idx_to_transform_huf [book][bit], bi_long_* per sampling rate)."""
import os

import numpy as np

NONE, NATURAL, FORCED, FOREIGN, EMPTY = 0, 1, 2, 3, 4
UNIT_DTYPE = np.dtype([("cls", "u1", (3,)), ("forced_bits", "u1"), ("nat", "u1", (3,)), ("window", "u1"), ("excess", "<i2", (3,)), ("reserved", "<u2")])
COUNTERS = ("regions", "natural", "forced", "forced_ones", "foreign", "empty", "excess_bits", "first_forced", "last_forced", "window_units")

_T = None


def tables():
    global _T
    if _T is None:
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g1_tables.npz"))
        meta = g["enc_huff_meta"]
        _T = {"hlen": {t: g[f"enc_hlen_{t}"].astype(np.int64) for t in [13] + list(range(15, 32))},
              "linbits": [int(meta[t][2]) for t in range(32)], "linmax": [int(meta[t][3]) for t in range(32)],
              "transform": g["idx_to_transform_huf"].astype(np.int64),
              "sfb_long": [g["bi_long_44"].astype(np.int64), g["bi_long_48"].astype(np.int64), g["bi_long_32"].astype(np.int64)]}   # by sr_idx
        assert all(len(_T["hlen"][t]) == 256 for t in _T["hlen"]) and _T["transform"].shape == (32, 2)
    return _T


def count_bit(v, t):
    """the reference's count_bit (encoder/MP3_Encoder.py:234-261) over the absolute values v (an even count of lines) under book t"""
    T = tables()
    x, y = v[0::2].copy(), v[1::2].copy()
    total = 0
    if t > 15:
        total += T["linbits"][t] * (int((x > 14).sum()) + int((y > 14).sum()))
        x[x > 14] = 15
        y[y > 14] = 15
    return total + int(T["hlen"][t][x * 16 + y].sum()) + int((x != 0).sum()) + int((y != 0).sum())


def first_book(lo, hi, v):
    """the first book of lo .. hi whose linmax reaches v (hi when none does: a value no stream can hold)"""
    T = tables()
    for i in range(lo, hi + 1):
        if T["linmax"][i] >= v:
            return i
    return hi


def audit_unit(spec, u, sr_idx):
    """one unit: spec = int16 [576], u = its UNIT_SIDE_DTYPE record -> a UNIT_DTYPE record"""
    T = tables()
    rec = np.zeros((), dtype=UNIT_DTYPE)
    t = [int(x) for x in u["table_select"]]
    if u["window_switching"]:
        rec["window"] = 1
        for r in (0, 1):
            rec["cls"][r] = FOREIGN if t[r] else NONE
        return rec
    bv = min(int(u["big_values"]), 288)
    sfb = T["sfb_long"][min(int(sr_idx), 2)]
    r0, r1 = int(u["region0_count"]), int(u["region1_count"])
    a3 = 2 * bv
    e1, e2 = int(sfb[min(r0 + 1, 22)]), int(sfb[min(r0 + r1 + 2, 22)])   # where the encoder's regions 0 and 1 end: not cut at a3
    a1, a2 = min(e1, a3), min(e2, a3)
    bounds = [(0, a1), (a1, a2), (a2, a3)]
    unseen = [e1 > a3, e2 > a3, False]                             # the region reaches behind the big values
    v_all = np.abs(spec.astype(np.int64))
    for r, (lo, hi) in enumerate(bounds):
        if t[r] == 0:
            continue
        if unseen[r]:
            rec["cls"][r] = EMPTY
            continue
        v = v_all[lo:hi] if hi > lo else v_all[:0]
        m = int(v.max()) if len(v) else 0
        if m == 0:
            rec["cls"][r] = EMPTY
            continue
        if m < 15:
            b13, b15 = count_bit(v, 13), count_bit(v, 15)
            nat, nat_bits = (15, b15) if b15 <= b13 else (13, b13)
        else:
            c0, c1 = first_book(15, 23, m - 15), first_book(24, 31, m - 15)
            s0, s1 = count_bit(v, c0), count_bit(v, c1)
            nat, nat_bits = (c1, s1) if s1 < s0 else (c0, s0)
        rec["nat"][r] = nat
        if t[r] == nat:
            rec["cls"][r] = NATURAL
            continue
        named = t[r] == 13 or 15 <= t[r] <= 31
        bit = None
        if named:
            for b in (0, 1):
                if t[r] == int(T["transform"][nat][b]):
                    bit = b
                    break
        if bit is None:
            rec["cls"][r] = FOREIGN
            continue
        rec["cls"][r] = FORCED
        rec["forced_bits"] |= bit << r
        rec["excess"][r] = count_bit(v, t[r]) - nat_bits
    return rec


def audit_units(is_, side, nch, sr_idx=None):
    """int16 [n][2 gr][2 ch][576], FRAME_SIDE records [n] -> UNIT_DTYPE [n][4], unit ch * 2 + gr (zeros for ch 1 of a mono batch);
    sr_idx: each frame's rate index from somewhere else than the side records (None: theirs)"""
    n = len(side)
    rates = side["sr_idx"] if sr_idx is None else sr_idx
    assert len(rates) == n
    is_ = np.asarray(is_).reshape(n, 2, 2, 576)
    out = np.zeros((n, 4), dtype=UNIT_DTYPE)
    for f in range(n):
        for ch in range(nch):
            for gr in range(2):
                out[f, ch * 2 + gr] = audit_unit(is_[f, gr, ch], side[f]["unit"][gr][ch], rates[f])
    return out


def audit_stream(units):
    """UNIT_DTYPE [n][4] of one stream -> (the counters as a dict, uint32 [n] profile)"""
    r = {k: 0 for k in COUNTERS}
    r["first_forced"] = r["last_forced"] = -1
    profile = np.zeros(len(units), dtype=np.uint32)
    names = {NATURAL: "natural", FORCED: "forced", FOREIGN: "foreign", EMPTY: "empty"}
    for f in range(len(units)):
        per = {NATURAL: 0, FORCED: 0, FOREIGN: 0, EMPTY: 0}
        for u in units[f]:
            r["window_units"] += int(u["window"])
            for g in range(3):
                cl = int(u["cls"][g])
                if cl == NONE:
                    continue
                per[cl] += 1
                r[names[cl]] += 1
                if cl == FORCED:
                    r["forced_ones"] += (int(u["forced_bits"]) >> g) & 1
                    r["excess_bits"] += int(u["excess"][g])
                    if r["first_forced"] < 0:
                        r["first_forced"] = r["regions"]
                    r["last_forced"] = r["regions"]
                r["regions"] += 1
        profile[f] = per[NATURAL] | per[FORCED] << 4 | per[FOREIGN] << 8 | per[EMPTY] << 12
    return r, profile


def audit_file(mlib, data, sr_idx=None):
    """the whole answer for one MP3 file: the counters, n_frames, channels, sampling_rate, kbps, payload_bits, verdict, profile;
    sr_idx: each frame's rate index where the caller knows it from the way the stream was built (None: the scan's)"""
    p, s = mlib.parse_stream(data), mlib.scan_stream(data)
    assert p["n_frames"] == s["n_frames"]
    n = p["n_frames"]
    if n == 0:
        r, profile = audit_stream(np.zeros((0, 4), dtype=UNIT_DTYPE))
    else:
        r, profile = audit_stream(audit_units(p["is"], s["side"], p["channels"], sr_idx))
    r.update(n_frames=n, channels=p["channels"], sampling_rate=p["sampling_rate"], kbps=p["bit_rate"] // 1000)
    r["payload_bits"] = r["last_forced"] + 1
    r["verdict"] = "foreign" if r["foreign"] > 0 else ("carries" if r["forced"] > 0 else "clean")
    r["profile"] = profile
    return r
