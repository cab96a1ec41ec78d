"""The encode transform (analysis filter bank, MDCT, alias butterflies: k_enc_analysis / k_enc_mdct / k_enc_fused, csrc/k_encode.hpp) where the
reference's int32 arithmetic wraps, and where the kernels' tiles and workgroups end: the streams, an exact model of the arithmetic, and the batches.

Streams (streams()): int16 stereo PCM from closed formulas, two frames each.  Full-scale cosines in every band, cosines just below a band
edge whose alias butterfly leaves int32 although no MDCT sum does, DC, squares, an impulse, and the 512 samples that drive the filter bank
to its largest subband sample.

Model (model()): MP3_Encoder.py:322-370 and :681-744 in int64 without wrapping, from the reference's own tables as tests/golden/g1_tables.npz
holds them.  Per line the exact MDCT sum, the exact butterfly result, whether either lies outside int32, and the value after the wraps.  It
is a census: what the oracle and the kernels are held to is the reference's record, tests/golden/g17_encode_edges.npz
(tests/golden/gen_encode_edges_golden.py), and tests/test_encode_edges.py first shows that model and record agree.

Batches (batches(), batch_census()): lists of (stream, k) -- the first k frames of a stream are a stream whose records are the first k frames
of the fixture's -- that reach every remainder and boundary the three kernels distinguish."""
import functools
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FRAMES = 2                                  # frames of every stream
SAMPLES = FRAMES * 1152
KBPS, KBPS_LOW = 128, 32
SR_IDX = {44100: 0, 48000: 1, 32000: 2}     # mp3s_frame_hdr.sr_idx (the transform must not read it)
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
EF_GR = 13                                  # granules of a workgroup of k_enc_fused (csrc/k_encode.hpp)

# the grid of the band-edge search: frequency (b - delta) * pi / 32, amplitude A * 32767, phase p * pi / 2; the first entry is a hit at b = 1
EDGE_START = (0.04, 0.9, 0)
EDGE_DELTAS = (0.04, -0.04, 0.02, -0.02, 0.01, -0.01, 0.0)
EDGE_AMPS = (0.9, 1.0, 0.95, 0.85, 0.8, 0.75, 0.7, 0.65, 0.6, 0.55)
EDGE_PHASES = (0, 1, 2, 3)
EDGE_BANDS = (1, 16, 31)
# what edge_search finds (test_edge_streams_are_the_first_hits_of_the_grid makes the search again); None: the grid holds no hit at that edge.
# The grid's first point turned out to be a hit at all three edges, so the search ends at once and its other 279 points are never visited:
# the grid stays as the recipe by which the three streams were chosen, and as the way to choose others if the samples ever have to change.
EDGE_HITS = {1: (0.04, 0.9, 0), 16: (0.04, 0.9, 0), 31: (0.04, 0.9, 0)}

LOW_RATE_STREAMS = ("tone/b03", "tone/b12", "edge/b01", "dc+", "square14", "analysis_max")    # also encoded at KBPS_LOW
OTHER_RATES = (("tone/b05", 48000), ("square14", 48000), ("tone/b05", 32000), ("square14", 32000))


def sha256(b):
    return np.frombuffer(hashlib.sha256(bytes(b)).digest(), dtype=np.uint8)


@functools.lru_cache(None)
def tables():
    """enwindow [512], fl [32][64], cos_l [18][36], the butterflies' cs / ca [8] as the reference evaluates them, int64"""
    g = np.load(os.path.join(GOLDEN, "g1_tables.npz"))
    return {k: g[n].astype(np.int64) for k, n in (("enwindow", "enwindow"), ("fl", "enc_fl"), ("cos_l", "enc_cos_l"), ("cs", "mdct_cs"), ("ca", "mdct_ca"))}


# ------------------------------------------------------------------------------------------------------------------------ the model
def wrap32(v):
    return ((np.asarray(v, dtype=np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def outside(v):
    return (v < I32_MIN) | (v > I32_MAX)


def window_sums(x):
    """tmp[i] of every slot of ONE channel, exact: sum_k ((x[32 t + 31 - (i + 64 k)] << 16) * enwindow[i + 64 k]) >> 32, the ring empty in
    front of the stream (MP3_Encoder.py:336-354, 751-758)"""
    ew = tables()["enwindow"]
    n = len(x) // 32
    xp = np.concatenate([np.zeros(512, dtype=np.int64), np.asarray(x, dtype=np.int64)]) << 16
    idx = 512 + 32 * np.arange(n)[:, None] + 31 - np.arange(512)[None, :]
    return ((xp[idx] * ew[None, :]) >> 32).reshape(n, 8, 64).sum(axis=1)


def subband_samples(y):
    """s[i] of every slot, exact, with the inversion of odd bands in odd slots (:358-368, :676-679)"""
    fl = tables()["fl"]
    s = ((y[:, None, :] * fl[None, :, :]) >> 32).sum(axis=2)
    s[1::2, 1::2] *= -1
    return s


def channel_model(x):
    """one channel of one stream -> exact MDCT sums and exact butterfly results [granule][576] (the butterflies read the WRAPPED sums, as
    the reference's do), and the largest |window sum| and |subband sample|"""
    T = tables()
    y = window_sums(x)
    s = subband_samples(y)
    g = s.reshape(-1, 18, 32)
    mdct_in = np.concatenate([np.concatenate([np.zeros((1, 18, 32), dtype=np.int64), g[:-1]]), g], axis=1)      # [granule][36][band]
    total = ((mdct_in[:, None, :, :] * T["cos_l"][None, :, :, None]) >> 32).sum(axis=2).transpose(0, 2, 1)       # [granule][band][k]
    w = wrap32(total)
    i = np.arange(8)
    a, b = w[:, 1:, :8], w[:, :-1, 17 - i]                                                                    # X[band][i], X[band - 1][17 - i]
    out = w.copy()
    out[:, 1:, :8] = (a * T["cs"] - b * T["ca"]) >> 31
    out[:, :-1, 17 - i] = (a * T["ca"] + b * T["cs"]) >> 31
    n = len(g)
    return total.reshape(n, 576), out.reshape(n, 576), int(np.abs(y).max()), int(np.abs(s).max())


def model(pcm):
    """a stream [samples][2] -> {"sum", "bfly": exact int64 [frame][ch][gr][576] (bfly: the line's last exact value -- the butterfly's
    result where one is applied, the wrapped sum elsewhere), "sum_out", "bfly_out": outside int32, "value": what the reference stores,
    "y_max", "sb_max": largest |window sum| and |subband sample|}"""
    per = [channel_model(pcm[:, ch]) for ch in range(2)]
    n = len(pcm) // 1152
    shape = lambda k: np.stack([p[k].reshape(n, 2, 576) for p in per], axis=1)                                 # noqa: E731
    m = {"sum": shape(0), "bfly": shape(1), "y_max": max(p[2] for p in per), "sb_max": max(p[3] for p in per)}
    m["sum_out"], m["bfly_out"] = outside(m["sum"]), outside(m["bfly"])
    m["value"] = wrap32(m["bfly"]).astype(np.int32)
    return m


def band_edge(line):
    """the band edge b whose butterfly writes this line of a granule (X[b][0..7] and X[b - 1][17..10]), or -1"""
    band, k = divmod(int(line), 18)
    return band if k < 8 and band >= 1 else band + 1 if k >= 10 and band <= 30 else -1


# ------------------------------------------------------------------------------------------------------------------------ the streams
def _i16(v):
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


def cosine(freq, amp=1.0, phase=0.0, n=SAMPLES):
    return _i16(32767.0 * amp * np.cos(freq * np.arange(n) + phase))


def tone(b):
    """channel 0: band b at line 9.5, channel 1: band 31 - b at line 4.5"""
    return np.stack([cosine((b + 9.5 / 18) * np.pi / 32), cosine((31 - b + 4.5 / 18) * np.pi / 32)], axis=1)


def edge(b, delta, amp, phase):
    """a cosine just off the edge between bands b - 1 and b; channel 1 is its negative"""
    f = (b - delta) * np.pi / 32
    return np.stack([cosine(f, amp, phase * np.pi / 2), cosine(f, amp, phase * np.pi / 2 + np.pi)], axis=1)


def is_edge_hit(pcm, b):
    """a granule of channel 0 with no MDCT sum outside int32 and a result of the butterfly at band edge b outside it"""
    m = channel_model(pcm[:, 0])
    for total, out in zip(m[0], m[1]):
        if not outside(total).any() and any(band_edge(l) == b for l in np.nonzero(outside(out))[0]):
            return True
    return False


def edge_grid():
    return [EDGE_START] + [(d, a, p) for d in EDGE_DELTAS for a in EDGE_AMPS for p in EDGE_PHASES if (d, a, p) != EDGE_START]


def edge_search(b):
    """the first point of the grid that is a hit at band edge b, or None"""
    for d, a, p in edge_grid():
        if is_edge_hit(edge(b, d, a, p), b):
            return d, a, p
    return None


def analysis_max():
    """one slot whose 512 samples carry the signs of enwindow[m] * fl[i][m % 64] for the band i with the largest bound, at full scale: in
    channel 0 at slot 20, in channel 1 with the other polarity at slot 47; zeros elsewhere -> (pcm, band)"""
    T = tables()
    coef = T["enwindow"][None, :] * T["fl"][:, np.arange(512) % 64]                                          # of x[32 t + 31 - m] in s[i]
    band = int(np.abs(coef).sum(axis=1).argmax())
    c = coef[band]
    pos, neg = int(c[c > 0].sum()), int(-c[c < 0].sum())
    sign = 1 if neg >= pos else -1                                                                         # the heavier side gets -32768
    x = np.where(sign * c > 0, 32767, np.where(sign * c < 0, -32768, 0))
    pcm = np.zeros((SAMPLES, 2), dtype=np.int16)
    for ch, slot, v in ((0, 20, x), (1, 47, np.where(x > 0, -32768, np.where(x < 0, 32767, 0)))):
        pcm[32 * slot + 31 - np.arange(512), ch] = v
    return pcm, band


class Stream:
    def __init__(self, pcm, rate=44100):
        self.pcm, self.rate = np.ascontiguousarray(pcm, dtype=np.int16), rate
        assert self.pcm.shape == (SAMPLES, 2)


@functools.lru_cache(None)
def streams():
    """name -> Stream, in the fixture's order"""
    t = np.arange(SAMPLES)
    S = {"tone/b%02d" % b: Stream(tone(b)) for b in range(16)}
    for b in EDGE_BANDS:
        if EDGE_HITS[b] is not None:
            S["edge/b%02d" % b] = Stream(edge(b, *EDGE_HITS[b]))
    S["dc+"] = Stream(np.full((SAMPLES, 2), 32767))
    S["dc-"] = Stream(np.full((SAMPLES, 2), -32768))
    sq14, sq100 = np.where((t // 7) % 2, 32767, -32768), np.where((t // 50) % 2, -32768, 32767)           # tests/test_fuzz.py's two channels
    S["square14"] = Stream(np.stack([sq14, np.where(sq14 > 0, -32768, 32767)], axis=1))
    S["square100"] = Stream(np.stack([sq100, np.where(sq100 > 0, -32768, 32767)], axis=1))
    imp = np.zeros((SAMPLES, 2), dtype=np.int16)
    imp[600, 0], imp[1700, 1] = 32767, -32768
    S["impulse_fullscale"] = Stream(imp)
    S["analysis_max"] = Stream(analysis_max()[0])
    for name, rate in OTHER_RATES:                                    # the same samples under another rate: the transform does not read it
        S["%s@%d" % (name, rate)] = Stream(S[name].pcm, rate)
    return S


def runs():
    """(stream, kbit/s) of every encode the fixture records, in its order"""
    return [(n, KBPS) for n in streams()] + [(n, KBPS_LOW) for n in LOW_RATE_STREAMS]


@functools.lru_cache(None)
def stream_model(name):
    return model(streams()[name].pcm)


# ------------------------------------------------------------------------------------------------------------------------ the batches
def _fill(names, ks, total):
    """(stream, k) from the two cycles until `total` frames are reached, the last stream cut to fit"""
    out, have, i = [], 0, 0
    while have < total:
        k = min(ks[i % len(ks)], total - have)
        out.append((names[i % len(names)], k))
        have, i = have + k, i + 1
    return out


def batches():
    """name -> [(stream, k)]: every length from 1 to 16 frames from the loud streams in turn, sixteen one-frame streams (a stream start at
    every offset of a 13-granule workgroup), a stream that ends with a workgroup's last granule and one that starts with the next one's
    first, and 32 frames (five workgroups)"""
    S = list(streams())
    loud = [n for n in S if not n.startswith(("impulse", "analysis"))]
    B = {}
    for n in range(1, 17):
        B["len%02d" % n] = _fill(loud[n:] + loud[:n], (2, 1, 2, 2), n)
    B["ones16"] = [(loud[(3 * i) % len(loud)], 1) for i in range(16)]
    # frames 0..12 in seven streams, the last of them one frame long: it ends with granule 25, the last of workgroup 1; the next starts with 26
    B["wg_edge16"] = [("dc+", 2), ("tone/b00", 2), ("square14", 2), ("tone/b15", 2), ("edge/b01", 2), ("tone/b07", 2), ("dc-", 1), ("square100", 2), ("tone/b09", 1)]
    B["wg_edge13"] = [("tone/b04", 1), ("dc-", 2), ("tone/b11", 2), ("square100", 2), ("analysis_max", 2), ("impulse_fullscale", 2), ("dc+", 2)]
    B["len32"] = _fill(S, (2, 2, 1), 32)
    return B


def batch_census(batch_list, wrapped):
    """what a set of batches reaches.  wrapped(stream, frame) -> does that frame of the stream hold a line the model flags.
    -> {"n_gran % 13", "n_frames % 4", "Ts % 64", "start offset", "g0 parity": sets, "ends at workgroup end", "starts at workgroup start",
    "loud places": counts, "max frames"}; n_gran % 13 counts batches of 1..13 frames only and Ts % 64 those of 1..16, as the kernels' shapes
    are stated.  A place is a stream boundary inside a batch or a workgroup boundary inside a batch; it is loud if the frame in front of
    it or behind it holds a flagged line -- behind a stream boundary that is the granule whose lead-in rows (k_enc_fused: 18 rows in front of
    g0; k_enc_mdct: the frame in front) belong to the stream before it."""
    c = {"n_gran % 13": set(), "n_frames % 4": set(), "Ts % 64": set(), "start offset": set(), "g0 parity": set(), "ends at workgroup end": 0,
         "starts at workgroup start": 0, "loud places": 0, "max frames": 0}
    for b in batch_list:
        frames = [(s, f) for s, k in b for f in range(k)]
        n = len(frames)
        n_gran = 2 * n
        c["max frames"] = max(c["max frames"], n)
        if n <= 13:
            c["n_gran % 13"].add(n_gran % EF_GR)
        c["n_frames % 4"].add(n % 4)
        if n <= 16:
            c["Ts % 64"].add(36 * n % 64)
        for g0 in range(0, n_gran, EF_GR):
            c["g0 parity"].add(g0 & 1)
        first, places = 0, set()
        for s, k in b:
            c["start offset"].add(2 * first % EF_GR)
            c["starts at workgroup start"] += first > 0 and 2 * first % EF_GR == 0
            c["ends at workgroup end"] += first + k < n and 2 * (first + k) % EF_GR == 0       # (the batch's own end is no stream boundary)
            if first:
                places.add(first)                                  # the boundary in front of frame `first`
            first += k
        places |= {g0 // 2 + (g0 & 1) for g0 in range(EF_GR, n_gran, EF_GR) if not g0 & 1}   # a workgroup boundary on a frame boundary ...
        inside = {g0 // 2 for g0 in range(EF_GR, n_gran, EF_GR) if g0 & 1}                   # ... or inside frame g0 // 2
        c["loud places"] += sum(1 for f in places if wrapped(*frames[f - 1]) or wrapped(*frames[f]))
        c["loud places"] += sum(1 for f in inside if wrapped(*frames[f]))
    return c


def batch_inputs(b, hdr_dtype):
    """-> (pcm [frames * 1152][2], hdr with nch, sr_idx and stream_first per stream)"""
    S = streams()
    pcm = np.concatenate([S[s].pcm[:k * 1152] for s, k in b])
    hdr = np.zeros(len(pcm) // 1152, dtype=hdr_dtype)
    hdr["nch"] = 2
    first = 0
    for s, k in b:
        hdr["stream_first"][first:first + k] = first
        hdr["sr_idx"][first:first + k] = SR_IDX[S[s].rate]
        first += k
    return pcm, hdr
