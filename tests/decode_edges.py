"""Case builders and the chain model for the decode transform at its parameter edges (tests/test_decode_edges.py,
tests/golden/gen_decode_edges_golden.py): Huffman-decoded lines and side records that put the requantisation front end of
k_dec_stream / k_dec_prepare on the boundaries of its branches -- the quick path's table boundary (-512 <= is < 512), both ends
of the gain tables (exp1 in [-266, 45], 2 * exp2 up to 36), every pair of per-channel cases (long / block_type 2 / mixed flag),
every block-type transition, one loud granule among quiet ones.  Everything is built from fixed seeds: the fixture pins digests of
these very arrays.

A case is (isv int16 [n][2][2][576], si GRANULE_SI_DTYPE [n][2][2], hdr FRAME_HDR_DTYPE [n], nch); hdr["stream_first"] marks the
streams of its batch.  |is| <= 8206, scale_fac_l[21] = 0 and scale_fac_s[:, 12] = 0, as the parser leaves them."""
import collections
import hashlib
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE_TAB = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 3, 2, 0)     # per long band (decoder/tables.py pre_tab; band 21: none)
BOUNDARY_VALUES = (-513, -512, -511, 511, 512, 513)
KINDS = [(bt, mixed) for bt in range(4) for mixed in range(2)]                    # what a channel of a granule can be
IS_MAX = 8206


def project_lib():
    """the project's mp3stego/_lib.py (record layouts).  Where another package of that name is in front -- the generator imports the
    reference, which is called mp3stego as well -- it is loaded from its file under a name of its own."""
    try:
        from mp3stego import _lib
        if hasattr(_lib, "GRANULE_SI_DTYPE"):
            return _lib
    except ImportError:
        pass
    if "mp3s_project_lib" not in sys.modules:
        spec = importlib.util.spec_from_file_location("mp3s_project_lib", os.path.join(ROOT, "mp3-steganography-lib_amd", "mp3stego", "_lib.py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules["mp3s_project_lib"] = m
        spec.loader.exec_module(m)
    return sys.modules["mp3s_project_lib"]


# ---------------------------------------------------------------------------------------------------------------- the chain model
def case_of(bt, mixed):
    """0 long, 1 block_type 2, 2 mixed flag with another block type (Frame.py:186, :277)"""
    return 1 if bt == 2 else (2 if mixed else 0)


def oracle_chain(orc, isv, si, hdr, nch):
    """float64 PCM [n * 1152][nch]: the oracle's stage functions chained as Frame.init_frame_params chains the reference's
    (Frame.py:265-286); the overlap and the fifo start as zeros where hdr["stream_first"] starts a new stream"""
    L = orc.lib()
    n = len(hdr)
    out = np.zeros((n * 1152, nch))
    first = np.asarray(hdr["stream_first"]).astype(np.int64)
    sbg = np.ascontiguousarray(si["sub_block_gain"], dtype=np.int32)
    sfl = np.ascontiguousarray(si["scale_fac_l"], dtype=np.int32)
    sfs = np.ascontiguousarray(si["scale_fac_s"], dtype=np.int32).reshape(n, 2, 2, 39)
    smp_all = np.ascontiguousarray(isv[:, :, :nch], dtype=np.float64)
    prev = fifo = None
    for f in range(n):
        if f == 0 or first[f] == f:
            prev = np.zeros((2, 32 * 18))
            fifo = np.zeros((2, 1024))
        sr_idx = int(hdr["sr_idx"][f])
        ms = nch == 2 and bool(hdr["ms_stereo"][f])
        for gr in range(2):
            rows = [smp_all[f, gr, ch] for ch in range(nch)]                      # contiguous views: the stages work in place
            for ch in range(nch):
                r = si[f, gr, ch]
                L.orc_requantize(rows[ch], int(r["global_gain"]), int(r["scalefac_scale"]), int(r["block_type"]), int(r["mixed_block_flag"]),
                                 int(r["preflag"]), sbg[f, gr, ch], sfl[f, gr, ch], sfs[f, gr, ch], sr_idx)
            if ms:
                L.orc_ms_stereo(rows[0], rows[1])
            for ch in range(nch):
                s = rows[ch]
                bt, mx = int(si["block_type"][f, gr, ch]), int(si["mixed_block_flag"][f, gr, ch])
                if bt == 2 or mx:
                    L.orc_reorder(s, sr_idx)
                else:
                    L.orc_alias_reduction(s)
                L.orc_imdct(s, bt, prev[ch])
                L.orc_frequency_inversion(s)
                L.orc_synth_filter_bank(s, fifo[ch])
                out[f * 1152 + gr * 576:f * 1152 + (gr + 1) * 576, ch] = s
    return out


def g4_batch(g, name):
    """a case of tests/golden/g4_decode_chain.npz as (isv, si, hdr, nch)"""
    P = project_lib()
    hdr_b, isv = g[name + "__hdr"], g[name + "__is"]
    n = isv.shape[0]
    mode = int(hdr_b[3] >> 6)
    nch = 1 if mode == 3 else 2
    si = np.zeros((n, 2, 2), dtype=P.GRANULE_SI_DTYPE)
    for field, key in (("global_gain", "gg"), ("scalefac_scale", "sfs"), ("block_type", "bt"), ("mixed_block_flag", "mixed"), ("preflag", "pre"),
                       ("sub_block_gain", "sbg"), ("scale_fac_l", "sfl"), ("scale_fac_s", "sfsh")):
        si[field] = g[name + "__" + key]
    hdr = np.zeros(n, dtype=P.FRAME_HDR_DTYPE)
    hdr["sr_idx"] = (hdr_b[2] >> 2) & 3
    hdr["nch"] = nch
    hdr["ms_stereo"] = 1 if (mode == 1 and (hdr_b[3] & 0x20)) else 0
    return isv, si, hdr, nch


def digest64(b):
    return int.from_bytes(hashlib.blake2b(b, digest_size=8).digest(), "little")


def input_digest(case):
    """the builder's arrays of a case: a fixture made from other inputs than the builders give now is told apart"""
    isv, si, hdr, nch = case
    return digest64(np.ascontiguousarray(isv, dtype="<i2").tobytes() + np.ascontiguousarray(si).tobytes() + np.ascontiguousarray(hdr).tobytes() +
                    bytes([nch]))


def frame_digests(pcm):
    """per frame a 64-bit blake2b of the float64 PCM bytes"""
    pcm = np.ascontiguousarray(pcm, dtype="<f8")
    return np.array([digest64(pcm[f * 1152:(f + 1) * 1152].tobytes()) for f in range(len(pcm) // 1152)], dtype=np.uint64)


# ---------------------------------------------------------------------------------------------------------------- what a case reaches
def quick(isv_g, si_g, nch):
    """k_dec_stream's rule for a granule (isv_g [2][576], si_g [2]): the quick path takes it when every channel is a long block without
    the mixed flag and every line of every channel satisfies -512 <= is < 512"""
    for ch in range(nch):
        if int(si_g["block_type"][ch]) == 2 or int(si_g["mixed_block_flag"][ch]) != 0:
            return False
        x = isv_g[ch].astype(np.int64)
        if not ((x >= -512) & (x < 512)).all():
            return False
    return True


def boundary_pairs(case, lo, hi):
    """granule pairs of a case that are identical (side records, every other line) but for one line, which is `lo` in one and `hi` in the
    other: [((frame, gr), (frame, gr), channel, line)]"""
    isv, si, _, nch = case
    n = len(isv)
    flat_is = isv.reshape(n * 2, 2, 576)
    flat_si = si.reshape(n * 2, 2)
    out = []
    has_lo = [a for a in range(n * 2) if (flat_is[a, :nch] == lo).any()]
    has_hi = [b for b in range(n * 2) if (flat_is[b, :nch] == hi).any()]
    for a in has_lo:
        for b in has_hi:
            if flat_si[a].tobytes() != flat_si[b].tobytes():
                continue
            d = np.argwhere(flat_is[a] != flat_is[b])
            if len(d) == 1 and flat_is[a][tuple(d[0])] == lo and flat_is[b][tuple(d[0])] == hi:
                out.append((divmod(a, 2), divmod(b, 2), int(d[0][0]), int(d[0][1])))
    return out


def exp1_values(case):
    """the indices of pow2q a case reads, as exp1 = global_gain - 210 - 8 * sub_block_gain (Frame.py:196, :204)"""
    _, si, _, nch = case
    out = set()
    for r in si[:, :, :nch].reshape(-1):
        gg, c = int(r["global_gain"]), case_of(int(r["block_type"]), int(r["mixed_block_flag"]))
        if c != 1:
            out.add(gg - 210)
        if c != 0:
            out.update(gg - 210 - 8 * int(s) for s in r["sub_block_gain"])
    return out


def k2_values(case):
    """the indices of pow2h a case reads, 2 * exp2 (Frame.py:198, :207-208), from its long channels' 21 long bands and its block_type 2
    channels' 3 x 12 short bands"""
    _, si, _, nch = case
    out = set()
    for r in si[:, :, :nch].reshape(-1):
        c, mult = case_of(int(r["block_type"]), int(r["mixed_block_flag"])), 2 if r["scalefac_scale"] else 1
        if c == 0:
            out.update(mult * (int(r["scale_fac_l"][b]) + (1 if r["preflag"] else 0) * PRE_TAB[b]) for b in range(21))
        elif c == 1:
            out.update(mult * int(v) for v in r["scale_fac_s"][:, :12].reshape(-1))
    return out


# every value 2 * exp2 can take with 4-bit scalefactors: exp2 = mult * (sf + preflag * pre_tab), mult 1/2 | 1, sf <= 15, pre_tab <= 3
K2_REACHABLE = frozenset(range(0, 19)) | frozenset(range(0, 37, 2))


def case_pair_census(case):
    """Counter of (case of ch 0, case of ch 1, ms, sr_idx, any |is| >= 512 in the granule) over a two-channel case's granules"""
    isv, si, hdr, nch = case
    assert nch == 2
    c = collections.Counter()
    for f in range(len(hdr)):
        for gr in range(2):
            a, b = (case_of(int(si["block_type"][f, gr, ch]), int(si["mixed_block_flag"][f, gr, ch])) for ch in range(2))
            c[(a, b, int(hdr["ms_stereo"][f]), int(hdr["sr_idx"][f]), bool((np.abs(isv[f, gr].astype(np.int32)) >= 512).any()))] += 1
    return c


# ---------------------------------------------------------------------------------------------------------------- builders
class _Batch:
    """frames of one case in the making"""

    def __init__(self, nch):
        self.nch, self.isv, self.si, self.hdr, self.first = nch, [], [], [], 0

    def stream(self):
        self.first = len(self.hdr)

    def frame(self, grans, sr=0, ms=0):
        """grans: two granules, each a list of nch (lines [576], side record)"""
        P = project_lib()
        isv = np.zeros((2, 2, 576), dtype=np.int16)
        si = np.zeros((2, 2), dtype=P.GRANULE_SI_DTYPE)
        assert len(grans) == 2
        for gr, chans in enumerate(grans):
            assert len(chans) == self.nch
            for ch, (x, r) in enumerate(chans):
                assert np.abs(np.asarray(x, dtype=np.int64)).max(initial=0) <= IS_MAX
                assert not r["scale_fac_l"][21] and not r["scale_fac_s"][:, 12].any()
                isv[gr, ch] = x
                si[gr, ch] = r
        h = np.zeros((), dtype=P.FRAME_HDR_DTYPE)
        h["sr_idx"], h["nch"], h["ms_stereo"], h["stream_first"] = sr, self.nch, 1 if (ms and self.nch == 2) else 0, self.first
        self.isv.append(isv)
        self.si.append(si)
        self.hdr.append(h)

    def granules(self, grans, sr=0, ms=0):
        """a run of granules as frames of one stream setting; an odd run repeats its last granule"""
        grans = list(grans)
        if len(grans) % 2:
            grans.append(grans[-1])
        for i in range(0, len(grans), 2):
            self.frame(grans[i:i + 2], sr, ms)

    def done(self):
        return np.stack(self.isv), np.stack(self.si), np.stack(self.hdr), self.nch


def _side(rng, gg, bt=0, mixed=0, sfs=None, pre=None, sbg=None, sf_l=None, sf_s=None):
    """one side record: what is not given is drawn"""
    r = np.zeros((), dtype=project_lib().GRANULE_SI_DTYPE)
    r["global_gain"], r["block_type"], r["mixed_block_flag"] = gg, bt, mixed
    r["scalefac_scale"] = int(rng.integers(0, 2)) if sfs is None else sfs
    r["preflag"] = int(rng.integers(0, 2)) if pre is None else pre
    r["sub_block_gain"] = rng.integers(0, 8, size=3) if sbg is None else sbg
    l = np.zeros(22, dtype=np.uint8)
    l[:21] = rng.integers(0, 16, size=21) if sf_l is None else sf_l
    s = np.zeros((3, 13), dtype=np.uint8)
    s[:, :12] = rng.integers(0, 16, size=(3, 12)) if sf_s is None else sf_s
    r["scale_fac_l"], r["scale_fac_s"] = l, s
    return r


def _noise(rng, max_abs=40):
    """lines as a Huffman decode leaves them: values up to max_abs in front, zeros behind"""
    x = np.zeros(576, dtype=np.int16)
    n_big = int(rng.integers(64, 577))
    x[:n_big] = rng.integers(-max_abs, max_abs + 1, size=n_big)
    return x


def _with(x, line, v):
    y = x.copy()
    y[line] = v
    return y


def _with_big(rng, x, n=4):
    """a few lines beyond the small table"""
    y = x.copy()
    for line in rng.integers(0, 576, size=n):
        y[line] = int(rng.choice([-1, 1])) * int(rng.choice([512, 513, 600, 1000, 4000, IS_MAX]))
    return y


def _quiet(rng, bt=0, mixed=0):
    return _noise(rng), _side(rng, int(rng.integers(150, 181)), bt, mixed)


def _table_boundary(seed, nch, ms):
    """long granules of |is| <= 40 with exactly one line on or next to the quick path's boundary"""
    rng = np.random.default_rng(seed)
    B = _Batch(nch)
    positions = [(0, 0), (0, 575), (1, 0), (1, 575), (1, 288)][:5 if nch == 2 else 2]
    grans = []
    for ch, line in positions:
        base = [_quiet(rng, bt=int(rng.choice([0, 1, 3]))) for _ in range(nch)]
        for v in BOUNDARY_VALUES:
            grans.append([(_with(x, line, v), r) if c == ch else (x, r) for c, (x, r) in enumerate(base)])
    B.granules(grans, 0, ms)
    for sr in (1, 2):
        B.stream()
        base = [_quiet(rng) for _ in range(nch)]
        ch = nch - 1
        B.frame([[(_with(x, 575, v), r) if c == ch else (x, r) for c, (x, r) in enumerate(base)] for v in (512, 511)], sr, ms)
    return B.done()


def _sparse(rng, exp1_top, m_max):
    """six lines, as large as leaves the requantised value below 1500 at the granule's largest gain (and at least 1)"""
    m = int(min(m_max, max(1.0, (1500.0 / 2.0 ** (exp1_top / 4.0)) ** 0.75)))
    x = np.zeros(576, dtype=np.int16)
    for line in rng.choice(576, size=6, replace=False):
        x[line] = int(rng.choice([-1, 1])) * int(rng.integers(max(1, m // 2), m + 1))
    return x


def _gain_range(seed):
    """every global_gain in long granules (small lines: the quick path's own look-up), every exp1 in [-266, 45] and every
    (window, sub_block_gain) in block_type 2 granules (dec_requant_tables)"""
    rng = np.random.default_rng(seed)
    B = _Batch(2)
    longs = [(_sparse(rng, gg - 210, 500), _side(rng, gg, bt=int(rng.choice([0, 1, 3])))) for gg in range(256)]
    B.granules([longs[i:i + 2] for i in range(0, 256, 2)])
    shorts, seen = [], set()
    for res in range(8):
        top = 45 - (45 - res) % 8                              # the residue class's largest exp1
        vals = list(range(top, -267, -8))
        assert len(vals) == 39 and vals[-1] >= -266
        for k in range(0, 39, 3):
            e0 = vals[k]
            a = 0
            while e0 + 210 + 8 * a < 0:
                a += 1
            gg = e0 + 210 + 8 * a
            assert 0 <= gg <= 255 and a + 2 <= 7
            rot = (len(shorts) + res) % 3
            sbg = [a + (w - rot) % 3 for w in range(3)]
            seen.update((w, s) for w, s in enumerate(sbg))
            shorts.append((_sparse(rng, gg - 210 - 8 * a, IS_MAX), _side(rng, gg, bt=2, mixed=len(shorts) % 4 == 3, sbg=sbg)))
    # the rotation above leaves some (window, sub_block_gain) out: granules at the corners bring them, (gg 0, sbg 7) and (gg 255, sbg 0) among them
    for gg, sbg in ((0, (7, 7, 7)), (255, (0, 0, 0)), (0, (6, 7, 6)), (255, (7, 6, 7)), (120, (6, 0, 1)), (130, (1, 6, 0))):
        seen.update((w, s) for w, s in enumerate(sbg))
        shorts.append((_sparse(rng, gg - 210 - 8 * min(sbg), IS_MAX), _side(rng, gg, bt=2, sbg=sbg)))
    assert seen == {(w, s) for w in range(3) for s in range(8)}, sorted(seen)
    B.stream()
    B.granules([shorts[i:i + 2] for i in range(0, len(shorts), 2)])
    return B.done()


def _exponent_top(seed):
    """the top of pow2h: scalefactor 15 everywhere, with and without preflag and scalefac_scale, in long, short and mixed granules, ramps
    that reach every value below it; the long ones with small lines (quick path) and with lines beyond the table (dec_requant_ms)"""
    rng = np.random.default_rng(seed)
    B = _Batch(2)
    ramp = np.arange(21) % 16
    for sr in range(3):
        chans = []
        for big in (False, True):
            for sfs in (0, 1):
                for pre in (0, 1):
                    for sf_l in (np.full(21, 15), ramp, ramp[::-1].copy()):
                        x = _noise(rng)
                        chans.append((_with_big(rng, x) if big else x, _side(rng, 170 + 20 * sfs, bt=int(rng.choice([0, 1, 3])), sfs=sfs, pre=pre, sf_l=sf_l)))
        for sfs in (0, 1):
            for sf_s in (np.full((3, 12), 15), (np.arange(36).reshape(3, 12) * 7) % 16):
                chans.append((_noise(rng), _side(rng, 170 + 20 * sfs, bt=2, sfs=sfs, sf_s=sf_s)))
        for sfs in (0, 1):
            for pre in (0, 1):
                for bt in (0, 1, 3):
                    chans.append((_noise(rng), _side(rng, 170 + 20 * sfs, bt=bt, mixed=1, sfs=sfs, pre=pre, sf_l=np.full(21, 15), sf_s=np.full((3, 12), 15))))
        assert len(chans) == 40
        if sr:
            B.stream()
        B.granules([chans[i:i + 2] for i in range(0, 40, 2)], sr)
    return B.done()


def _case_pairs(seed, nch, ms):
    """every pair of channel kinds (block_type x mixed flag), a stream per sampling rate; about half of the granules with lines beyond the table"""
    rng = np.random.default_rng(seed)
    B = _Batch(nch)
    per_rate, met = [[], [], []], collections.Counter()
    pairs = [(a, b) for a in KINDS for b in KINDS] if nch == 2 else [(a,) for a in KINDS]
    for p, kinds in enumerate(pairs):
        chans = [_quiet(rng, bt, mixed) for bt, mixed in kinds]
        cp = tuple(case_of(bt, mixed) for bt, mixed in kinds)
        met[cp] += 1
        if met[cp] % 2 == 0:                                   # every other granule of a case pair
            chans = [(_with_big(rng, x, 3), r) if rng.random() < 0.7 or c == 0 else (x, r) for c, (x, r) in enumerate(chans)]
        per_rate[p % 3].append(chans)
    for sr in range(3):
        if sr:
            B.stream()
        B.granules(per_rate[sr], sr, ms)
    case = B.done()
    if nch == 2:
        census = case_pair_census(case)
        for a in range(3):
            for b in range(3):
                assert all(any(census[(a, b, ms, sr, big)] for big in (False, True)) for sr in range(3)), (a, b, "rate")
                assert all(any(census[(a, b, ms, sr, big)] for sr in range(3)) for big in (False, True)), (a, b, "table side")
    return case


# a closed walk over the four block types that takes every ordered pair once (16 steps, 17 granules)
_WALK = (0, 0, 1, 0, 2, 0, 3, 1, 1, 2, 1, 3, 2, 2, 3, 3, 0)


def _transitions(seed, nch, ms):
    """consecutive granules walk all 16 ordered block_type pairs in every channel (ch 1 runs the walk backwards); a second lap carries
    the mixed flag on every other granule"""
    rng = np.random.default_rng(seed)
    assert {(a, b) for a, b in zip(_WALK, _WALK[1:])} == {(a, b) for a in range(4) for b in range(4)}
    B = _Batch(nch)
    grans = []
    for lap in range(2):
        for i in range(len(_WALK) + 1):                       # (18 granules a lap: the walk and its first step again)
            bts = (_WALK[i % 16], _WALK[::-1][i % 16])[:nch]
            grans.append([_quiet(rng, bt, mixed=1 if lap and (i + c) % 2 else 0) for c, bt in enumerate(bts)])
    B.granules(grans, 0, ms)
    return B.done()


def _loud_among_quiet(seed):
    """one granule at global_gain 255 with lines at +-8206 among quiet ones"""
    rng = np.random.default_rng(seed)
    B = _Batch(2)
    grans = [[_quiet(rng, bt=int(rng.choice([0, 0, 1, 2, 3]))) for _ in range(2)] for _ in range(12)]
    x = np.zeros(576, dtype=np.int16)
    x[[0, 5, 100, 287, 288, 400, 574, 575]] = [IS_MAX, -IS_MAX, IS_MAX, IS_MAX, -IS_MAX, IS_MAX, -IS_MAX, IS_MAX]
    grans[7][0] = (x, _side(rng, 255, sfs=0, pre=0, sf_l=np.zeros(21)))
    B.granules(grans)
    return B.done()


_cases = None


def cases():
    """name -> (isv, si, hdr, nch), in the fixture's order; built once"""
    global _cases
    if _cases is None:
        out = collections.OrderedDict()
        modes = (("stereo", 2, 0), ("ms", 2, 1), ("mono", 1, 0))
        for k, (mode, nch, ms) in enumerate(modes):
            out["table_boundary/" + mode] = _table_boundary(0x7AB1E + k, nch, ms)
        out["gain_range"] = _gain_range(0x6A17)
        out["exponent_top"] = _exponent_top(0xE2707)
        for k, (mode, nch, ms) in enumerate(modes):
            out["case_pairs/" + mode] = _case_pairs(0xCA5E + k, nch, ms)
        for k, (mode, nch, ms) in enumerate(modes):
            out["transitions/" + mode] = _transitions(0x7245 + k, nch, ms)
        out["loud_among_quiet"] = _loud_among_quiet(0x10BD)
        _cases = out
    return _cases


SWEEP_KINDS = (("long", 0, 0), ("short", 2, 0), ("mixed", 1, 1))
SWEEP_VALUES = (511, 512)


def line_sweep(sr, kind):
    """one frame per pair of lines, each a stream of its own: granule gr of frame j has +v at line l = 2 j + gr of ch 0 and -v at line
    575 - l of ch 1, v = 511 in the even frames and 512 in the odd ones.  Scalefactors and sub-block gains differ from band to band
    and window to window, so a line read with another band's factors shows.  No seed."""
    bt, mixed = {k: (b, m) for k, b, m in SWEEP_KINDS}[kind]
    P = project_lib()
    n = 288
    isv = np.zeros((n, 2, 2, 576), dtype=np.int16)
    si = np.zeros((n, 2, 2), dtype=P.GRANULE_SI_DTYPE)
    si["global_gain"], si["block_type"], si["mixed_block_flag"], si["preflag"] = 170, bt, mixed, 1
    si["sub_block_gain"] = (0, 3, 7)
    si["scale_fac_l"][..., :21] = (np.arange(21) * 5 + 1) % 16
    si["scale_fac_s"][..., :12] = (np.arange(36).reshape(3, 12) * 7 + 2) % 16
    hdr = np.zeros(n, dtype=P.FRAME_HDR_DTYPE)
    hdr["sr_idx"], hdr["nch"], hdr["stream_first"] = sr, 2, np.arange(n)
    j = np.arange(n)
    v = np.where(j % 2 == 0, SWEEP_VALUES[0], SWEEP_VALUES[1])
    for gr in range(2):
        isv[j, gr, 0, 2 * j + gr] = v
        isv[j, gr, 1, 575 - (2 * j + gr)] = -v
    return isv, si, hdr, 2
