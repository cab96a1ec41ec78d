"""QMDCT on the device (include/mp3s.h section vi-g): the Markov / histogram features of MP3 lists (mp3s_qmdct_features_files /
Context.qmdct_features), the spectra as a batch in device memory (mp3s_qmdct_batch_decode_files / Context.qmdct_batch /
tensors.qmdct) and the two kernels alone (Context.qmdct_features_dev, Context.qmdct_batch_dev).

The expected values come from tests/qmdct_model.py, the definitions restated in numpy over the host-only parse_stream; it runs no
code of the feature.  Every GPU test compares every field with the model exactly."""
import ctypes as C
import os

import numpy as np
import pytest

import qmdct_model as M

gpu = pytest.mark.gpu
ARRAYS = ("hist", "intra", "inter", "max_abs", "bandwidth")
SCALARS = ("n_frames", "n_granules", "channels", "n_lines")
KS = (1, 2, 3, 9, 575, 576)

# the model on tests/golden/test.mp3 (one CPU run; test_model_identities_and_literals repeats it)
TEST_MP3_HIST = [[21587, 2642, 2070, 1258, 956, 811, 980, 603, 742, 694, 582, 537, 477, 451, 371, 6711],
                 [21725, 2457, 2073, 1281, 1001, 785, 1038, 552, 756, 668, 626, 523, 497, 428, 427, 6635]]
TEST_MP3_MAX_ABS, TEST_MP3_BANDWIDTH = [978, 927], [576, 576]


def other_encoders(golden_dir):
    g = np.load(os.path.join(golden_dir, "g7_decode_corpus.npz"))
    files = {"test.mp3": open(os.path.join(golden_dir, "test.mp3"), "rb").read()}
    for n in sorted({k.split("__")[0] for k in g.files}):
        files[n] = g[n + "__mp3"].tobytes()
    return files


def same(got, want, where):
    """every field of an answer of qmdct_features against the model's (the header fields of a file apart)"""
    assert not isinstance(got, Exception), (where, got)
    for k in SCALARS:
        assert got[k] == want[k], (where, k, got[k], want[k])
    for k in ARRAYS:
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (where, k, got[k], want[k])


# ------------------------------------------------------------------------------------------------ no device
def test_qmdct_symbols_and_layout(mlib):
    L = mlib.lib()
    for s in ("mp3s_qmdct_features_dev", "mp3s_qmdct_features_files", "mp3s_qmdct_batch_dev", "mp3s_qmdct_batch_decode_files"):
        assert hasattr(L, s) and s in mlib.SYMBOLS, s
    ch, ft = mlib.QmdctChannel, mlib.QmdctFeatures
    assert [(n, getattr(ch, n).offset, getattr(ch, n).size) for n, _ in ch._fields_] == \
        [("hist", 0, 128), ("intra", 128, 648), ("inter", 776, 648), ("max_abs", 1424, 8), ("bandwidth", 1432, 8)]
    assert [(n, getattr(ft, n).offset, getattr(ft, n).size) for n, _ in ft._fields_] == \
        [("ch", 0, 2880), ("n_frames", 2880, 4), ("channels", 2884, 4), ("sampling_rate", 2888, 4), ("kbps", 2892, 4), ("n_lines", 2896, 4), ("reserved", 2900, 4)]
    assert C.sizeof(ch) == mlib.QMDCT_CHANNEL_DTYPE.itemsize == 1440 and C.sizeof(ft) == mlib.QMDCT_FEATURES_DTYPE.itemsize == 2904
    assert [(n, mlib.QMDCT_CHANNEL_DTYPE.fields[n][1]) for n in mlib.QMDCT_CHANNEL_DTYPE.names] == [(n, getattr(ch, n).offset) for n, _ in ch._fields_]
    assert [(n, mlib.QMDCT_FEATURES_DTYPE.fields[n][1]) for n in mlib.QMDCT_FEATURES_DTYPE.names] == [(n, getattr(ft, n).offset) for n, _ in ft._fields_]
    it, nf = mlib.QmdctBatchItem, mlib.QmdctBatchInfo
    assert [(n, getattr(it, n).offset) for n, _ in it._fields_] == [("src_frame", 0), ("n_frames", 8), ("first_granule", 16), ("slot", 24), ("reserved", 28)]
    assert [(n, getattr(nf, n).offset) for n, _ in nf._fields_] == \
        [("n_frames", 0), ("nch", 4), ("sampling_rate", 8), ("bit_rate", 12), ("n_granules", 16), ("first_granule", 24), ("valid_granules", 32)]
    assert C.sizeof(it) == mlib.QMDCT_BATCH_ITEM_DTYPE.itemsize == 32 and C.sizeof(nf) == mlib.QMDCT_BATCH_INFO_DTYPE.itemsize == 40
    assert [(n, mlib.QMDCT_BATCH_ITEM_DTYPE.fields[n][1]) for n in mlib.QMDCT_BATCH_ITEM_DTYPE.names] == [(n, getattr(it, n).offset) for n, _ in it._fields_]
    assert [(n, mlib.QMDCT_BATCH_INFO_DTYPE.fields[n][1]) for n in mlib.QMDCT_BATCH_INFO_DTYPE.names] == [(n, getattr(nf, n).offset) for n, _ in nf._fields_]
    assert mlib.QMDCT_T == M.T == 4 and mlib.QMDCT_SLICE >= 1 and mlib.QMDCT_SLICE * 576 < 2 ** 32
    # the header says the same
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "mp3s.h")).read()
    for decl in ("#define MP3S_QMDCT_T 4", "#define MP3S_QMDCT_SLICE %d" % mlib.QMDCT_SLICE,
                 "typedef struct { int64_t hist[16], intra[9][9], inter[9][9], max_abs, bandwidth; } mp3s_qmdct_channel;",
                 "typedef struct { mp3s_qmdct_channel ch[2]; int32_t n_frames, channels, sampling_rate, kbps, n_lines, reserved; } mp3s_qmdct_features;",
                 "} mp3s_qmdct_batch_item; /* 32 bytes */",
                 "typedef struct { int32_t n_frames, nch, sampling_rate, bit_rate; int64_t n_granules, first_granule, valid_granules; } mp3s_qmdct_batch_info;",
                 "int mp3s_qmdct_features_dev(mp3s_ctx *ctx, const int16_t *d_is, int n_frames, int nch, const mp3s_table_audit_seg *d_segs,",
                 "int mp3s_qmdct_features_files(mp3s_ctx *ctx, const uint8_t *const *mp3s, const size_t *lens, int n_files, int n_lines,",
                 "int mp3s_qmdct_batch_dev(mp3s_ctx *ctx, const int16_t *d_is, int nch, const mp3s_qmdct_batch_item *d_items,",
                 "int mp3s_qmdct_batch_decode_files(mp3s_ctx *ctx, const uint8_t *const *mp3s, const size_t *lens, int n_files, const int64_t *first_granules"):
        assert decl in txt, decl
    assert "#define MP3S_OPT_COUNT 22" in txt and "#define MP3S_N_KERNELS 9" in txt


def test_qmdct_bad_arguments(mlib):
    """argument checks need no device: a made-up context is never looked into"""
    L, E = mlib.lib(), mlib.E_ARG
    fake, p = C.c_void_p(64), C.c_void_p(4096)
    one, lens = (C.c_void_p * 1)(C.addressof(mlib._EMPTY)), (C.c_size_t * 1)(0)
    status = (C.c_int32 * 1)()
    # ---- mp3s_qmdct_features_dev
    segs = np.array([(0, 3), (3, 1)], dtype=mlib.TABLE_AUDIT_SEG_DTYPE)
    h = C.c_void_p(segs.ctypes.data)
    D = L.mp3s_qmdct_features_dev
    assert D(None, p, 4, 2, p, h, 2, 576, p) == E
    assert D(fake, None, 4, 2, p, h, 2, 576, p) == E
    assert D(fake, p, 4, 2, None, h, 2, 576, p) == E
    assert D(fake, p, 4, 2, p, None, 2, 576, p) == E
    assert D(fake, p, 4, 2, p, h, 2, 576, None) == E
    assert D(fake, p, 0, 2, p, h, 2, 576, p) == E and D(fake, p, -1, 2, p, h, 2, 576, p) == E
    assert D(fake, p, 4, 2, p, h, 0, 576, p) == E and D(fake, p, 4, 2, p, h, -2, 576, p) == E
    assert D(fake, p, 4, 0, p, h, 2, 576, p) == E and D(fake, p, 4, 3, p, h, 2, 576, p) == E
    assert D(fake, p, 4, 2, p, h, 2, 0, p) == E and D(fake, p, 4, 2, p, h, 2, 577, p) == E and D(fake, p, 4, 2, p, h, 2, -1, p) == E
    assert D(fake, C.c_void_p(4098), 4, 2, p, h, 2, 576, p) == E           # d_is not 4-byte aligned
    assert D(fake, p, 4, 2, p, h, 2, 576, C.c_void_p(4100)) == E           # d_out not 8-byte aligned
    assert D(fake, p, 3, 2, p, h, 2, 576, p) == E                          # the second segment ends behind the batch
    for bad in ([(0, 3), (-1, 1)], [(0, 3), (3, -1)], [(2, 3), (3, 1)], [(2 ** 31 - 1, 2 ** 31 - 1), (0, 1)]):
        b = np.array(bad, dtype=mlib.TABLE_AUDIT_SEG_DTYPE)
        assert D(fake, p, 4, 2, p, C.c_void_p(b.ctypes.data), 2, 576, p) == E, bad
    # ---- mp3s_qmdct_features_files
    out = (mlib.QmdctFeatures * 1)()
    F = L.mp3s_qmdct_features_files
    assert F(None, one, lens, 1, 576, out, status) == E
    assert F(fake, None, lens, 1, 576, out, status) == E
    assert F(fake, one, None, 1, 576, out, status) == E
    assert F(fake, one, lens, 1, 576, None, status) == E
    assert F(fake, one, lens, 0, 576, out, status) == E and F(fake, one, lens, -1, 576, out, status) == E
    assert F(fake, one, lens, 1, 0, out, status) == E and F(fake, one, lens, 1, 577, out, status) == E
    # ---- mp3s_qmdct_batch_dev
    items = np.zeros(2, dtype=mlib.QMDCT_BATCH_ITEM_DTYPE)
    items["n_frames"], items["slot"] = 2, [0, 1]
    hi = C.c_void_p(items.ctypes.data)
    Bd = L.mp3s_qmdct_batch_dev
    assert Bd(None, p, 2, p, hi, 2, 2, 4, p) == E
    assert Bd(fake, None, 2, p, hi, 2, 2, 4, p) == E
    assert Bd(fake, p, 2, None, hi, 2, 2, 4, p) == E
    assert Bd(fake, p, 2, p, None, 2, 2, 4, p) == E
    assert Bd(fake, p, 2, p, hi, 2, 2, 4, None) == E
    assert Bd(fake, p, 2, p, hi, 0, 2, 4, p) == E and Bd(fake, p, 2, p, hi, -1, 2, 4, p) == E
    assert Bd(fake, p, 0, p, hi, 2, 2, 4, p) == E and Bd(fake, p, 3, p, hi, 2, 2, 4, p) == E
    assert Bd(fake, p, 2, p, hi, 2, 0, 4, p) == E and Bd(fake, p, 2, p, hi, 2, 3, 4, p) == E
    assert Bd(fake, p, 2, p, hi, 2, 1, 4, p) == E                          # stereo into one channel: no downmix of quantised values
    assert Bd(fake, p, 2, p, hi, 2, 2, 0, p) == E and Bd(fake, p, 2, p, hi, 2, 2, -4, p) == E
    assert Bd(fake, C.c_void_p(4104), 2, p, hi, 2, 2, 4, p) == E           # d_is not 16-byte aligned
    assert Bd(fake, p, 2, p, hi, 2, 2, 4, C.c_void_p(4104)) == E           # d_out not 16-byte aligned
    for field in ("src_frame", "n_frames", "first_granule", "slot"):
        b = items.copy()
        b[field][1] = -1
        assert Bd(fake, p, 2, p, C.c_void_p(b.ctypes.data), 2, 2, 4, p) == E, field
    # ---- mp3s_qmdct_batch_decode_files
    info = (mlib.QmdctBatchInfo * 1)()
    first = (C.c_int64 * 1)(-1)
    G = L.mp3s_qmdct_batch_decode_files
    assert G(None, one, lens, 1, None, 4, 2, p, 1 << 20, info, status) == E
    assert G(fake, None, lens, 1, None, 4, 2, p, 1 << 20, info, status) == E
    assert G(fake, one, None, 1, None, 4, 2, p, 1 << 20, info, status) == E
    assert G(fake, one, lens, 1, None, 4, 2, p, 1 << 20, None, status) == E
    assert G(fake, one, lens, 0, None, 4, 2, p, 1 << 20, info, status) == E
    assert G(fake, one, lens, 1, None, 4, 0, p, 1 << 20, info, status) == E and G(fake, one, lens, 1, None, 4, 3, p, 1 << 20, info, status) == E
    assert G(fake, one, lens, 1, None, 0, 2, p, 1 << 20, info, status) == E
    assert G(fake, one, lens, 1, None, 4, 2, C.c_void_p(4104), 1 << 20, info, status) == E      # d_out not 16-byte aligned
    assert G(fake, one, lens, 1, None, 4, 2, p, 4 * 2 * 1152 - 1, info, status) == E            # out_bytes a byte short
    assert G(fake, one, lens, 1, first, 4, 2, p, 1 << 20, info, status) == E                    # a negative first granule


def test_model_identities_and_literals(mlib, golden_dir):
    data = open(os.path.join(golden_dir, "test.mp3"), "rb").read()
    p = mlib.parse_stream(data)
    f = M.features(p["is"], p["channels"])
    M.identities(f, 576)
    assert f["hist"].tolist() == TEST_MP3_HIST and f["max_abs"].tolist() == TEST_MP3_MAX_ABS and f["bandwidth"].tolist() == TEST_MP3_BANDWIDTH
    assert (f["n_frames"], f["n_granules"], f["channels"]) == (36, 72, 2)
    g = mlib.parse_stream(np.load(os.path.join(golden_dir, "g6_synth128.npz"))["mp3"].tobytes())
    for K in KS + (100,):
        M.identities(M.features(p["is"], 2, K), K)
        M.identities(M.features(g["is"], 2, K), K)
    assert M.features(g["is"], 2)["n_granules"] == 96


def hand_made():
    """2 frames of a mono stream, K = 4.  a = |q| of the four rows over the counted lines:
         row 0:  0  0  0  0        row 1:  1  0  3  0        row 2:  9  9  0  1        row 3:  0  2  2  32768
       hist: 0 x 8, 1 x 2, 2 x 2, 3 x 1, 9 x 2, 15 (32768 capped) x 1                                       -- 16 = G K
       dh (clipped to +-4), rows 0 .. 3: (0 0 0), (1 -3 3), (0 4 -1), (-2 0 -4); the pairs (dh[k], dh[k+1]) for k = 0, 1:
         (0,0) (0,0) | (1,-3) (-3,3) | (0,4) (4,-1) | (-2,0) (0,-4)
         intra[i][j] with i = d0 + 4, j = d1 + 4: [4][4] = 2, [5][1] = [1][7] = [4][8] = [8][3] = [2][4] = [4][0] = 1   -- 8 = G (K - 2)
       dv, g = 0 .. 2: (-1 0 -3 0), (-4 -4 3 -1), (4 4 -2 -4); the pairs (dv[g][k], dv[g+1][k]) for g = 0, 1:
         g = 0: (-1,-4) (0,-4) (-3,3) (0,-1)      g = 1: (-4,4) (-4,4) (3,-2) (-1,-4)
         inter: [3][0] = 2, [0][8] = 2, [4][0] = [1][7] = [4][3] = [7][2] = 1                                   -- 8 = (G - 2) K
       max_abs = 32768, bandwidth = 4.  Lines 4 .. 575 and channel 1 hold values that must not count."""
    is_ = np.full((2, 2, 2, 576), 77, dtype=np.int16)
    rows = [[0, 0, 0, 0], [-1, 0, 3, 0], [9, -9, 0, 1], [0, 2, -2, -32768]]
    for g, r in enumerate(rows):
        is_[g >> 1, g & 1, 0, :4] = r
    want = {"hist": np.zeros((1, 16), dtype=np.int64), "intra": np.zeros((1, 9, 9), dtype=np.int64), "inter": np.zeros((1, 9, 9), dtype=np.int64),
            "max_abs": np.array([32768], dtype=np.int64), "bandwidth": np.array([4], dtype=np.int64), "n_frames": 2, "n_granules": 4, "channels": 1, "n_lines": 4}
    for v, n in ((0, 8), (1, 2), (2, 2), (3, 1), (9, 2), (15, 1)):
        want["hist"][0, v] = n
    for (i, j), n in {(4, 4): 2, (5, 1): 1, (1, 7): 1, (4, 8): 1, (8, 3): 1, (2, 4): 1, (4, 0): 1}.items():
        want["intra"][0, i, j] = n
    for (i, j), n in {(3, 0): 2, (0, 8): 2, (4, 0): 1, (1, 7): 1, (4, 3): 1, (7, 2): 1}.items():
        want["inter"][0, i, j] = n
    return is_, want


def test_model_on_the_hand_made_case():
    is_, want = hand_made()
    got = M.features(is_, 1, 4)
    same(got, want, "hand-made")
    M.identities(got, 4)


# ------------------------------------------------------------------------------------------------ GPU, the kernels alone
def made_row(rng, n):
    """n rows of a decaying random spectrum with a long zero tail"""
    k = np.arange(576)
    cut = rng.integers(0, 577, size=(n, 1))
    mag = np.floor(rng.exponential(1.0, size=(n, 576)) * 40.0 * np.exp(-k / rng.integers(8, 200, size=(n, 1)))).astype(np.int64)
    mag[k[None, :] >= cut] = 0
    return (mag * rng.choice(np.array([-1, 1]), size=(n, 576))).astype(np.int16)


@pytest.fixture(scope="module")
def made(mlib):
    """one batch of adjacent streams: 0, 1 and 2 frames; the frame counts that give G in {S - 2, S, S + 2, 2 S, 2 S + 2}; an all-zero
    stream that crosses a slice; a constant non-zero stream.  Extreme values at line 0, at the last counted line of every K of KS and
    on both sides of row ends.  With the model's records for every K, stereo."""
    S = mlib.QMDCT_SLICE
    assert S % 2 == 0
    lengths = [0, 1, 2, S // 2 - 1, S // 2, S // 2 + 1, S, S + 1, S // 2 + 1, 5]
    n = sum(lengths)
    rng = np.random.default_rng(2024)
    is_ = made_row(rng, n * 4).reshape(n, 2, 2, 576)
    first = np.cumsum([0] + lengths[:-1])
    extremes = [8206, -8206, 32767, -32767, -32768]
    flat = is_.reshape(n * 4, 576)                                   # (row order frame, gr, ch: a row's neighbour down the channel is 2 further)
    for s, (f0, cnt) in enumerate(zip(first, lengths)):
        for t in range(min(cnt * 4, 24)):
            r = f0 * 4 + (t * 7) % (cnt * 4)
            flat[r, [0, 1, 2, 8, 574, 575][t % 6]] = extremes[(t + s) % 5]
        if cnt:                                                      # both sides of a row end, and of the stream's last row end
            flat[f0 * 4, 575], flat[f0 * 4 + 2, 0] = -32768, 32767
            flat[(f0 + cnt) * 4 - 1, 575] = 8206
    zero, const = 8, 9
    is_[first[zero]:first[zero] + lengths[zero]] = 0
    is_[first[const]:first[const] + lengths[const]] = -3
    segs = np.zeros(len(lengths), dtype=mlib.TABLE_AUDIT_SEG_DTYPE)
    segs["first_frame"], segs["n_frames"] = first, lengths
    want = {K: np.array([M.record(is_[f0:f0 + cnt], 2, K, mlib.QMDCT_FEATURES_DTYPE) for f0, cnt in zip(first, lengths)]) for K in KS}
    for a, b in zip(range(len(lengths) - 1), range(1, len(lengths))):   # neighbours differ: a term that crosses a boundary changes a count
        if lengths[a] and lengths[b]:
            assert not np.array_equal(is_[first[a] + lengths[a] - 1], is_[first[b]])
    return {"is": is_, "segs": segs, "lengths": lengths, "first": first, "want": want, "zero": zero, "const": const}


def records_equal(got, want, where):
    for k in got.dtype.names:
        if k == "ch":
            for c in (0, 1):
                for q in got["ch"].dtype.names:
                    assert np.array_equal(got["ch"][q][:, c], want["ch"][q][:, c]), (where, c, q, np.nonzero(got["ch"][q][:, c] != want["ch"][q][:, c]))
        else:
            assert np.array_equal(got[k], want[k]), (where, k, got[k], want[k])
    assert got.tobytes() == want.tobytes(), where


@gpu
@pytest.mark.parametrize("K", KS)
def test_features_kernel_stereo(ctx, mlib, made, K):
    got = ctx.qmdct_features_dev(made["is"], made["segs"], 2, K)      # (the records are 0xFF bytes before the call)
    records_equal(got, made["want"][K], K)
    again = ctx.qmdct_features_dev(made["is"], made["segs"], 2, K)
    assert again.tobytes() == got.tobytes()
    G = 2 * np.array(made["lengths"])
    for c in (0, 1):
        assert np.array_equal(got["ch"]["hist"][:, c].sum(axis=1), G * K)
        assert np.array_equal(got["ch"]["intra"][:, c].sum(axis=(1, 2)), G * max(K - 2, 0))
        assert np.array_equal(got["ch"]["inter"][:, c].sum(axis=(1, 2)), np.maximum(G - 2, 0) * K)
    z = got[made["zero"]]["ch"]                                      # all zero: only the three dominant bins, and they are the identities
    gz = int(G[made["zero"]])
    for c in (0, 1):
        assert z["hist"][c][0] == gz * K and z["intra"][c][4][4] == gz * max(K - 2, 0) and z["inter"][c][4][4] == (gz - 2) * K
        assert z["hist"][c].sum() == z["hist"][c][0] and z["intra"][c].sum() == z["intra"][c][4][4] and z["inter"][c].sum() == z["inter"][c][4][4]
        assert z["max_abs"][c] == 0 and z["bandwidth"][c] == 0
    k3 = got[made["const"]]["ch"]
    assert k3["hist"][0][3] == int(G[made["const"]]) * K and k3["max_abs"][0] == 3 and k3["bandwidth"][1] == K
    assert not got[0]["ch"]["hist"].any() and got[0]["n_frames"] == 0 and got[0]["channels"] == 2 and got[0]["n_lines"] == K
    assert got[1]["ch"]["inter"].sum() == 0 and got[2]["ch"]["inter"].sum() == 2 * 2 * K      # G = 2: no pair; G = 4: two first rows


@gpu
@pytest.mark.parametrize("K", KS)
def test_features_kernel_mono(ctx, mlib, made, K):
    """the same arrays as a mono batch: channel 1 is garbage that is never read"""
    got = ctx.qmdct_features_dev(made["is"], made["segs"], 1, K)
    want = made["want"][K].copy()
    want["ch"][:, 1] = np.zeros((), dtype=mlib.QMDCT_CHANNEL_DTYPE)
    want["channels"] = 1
    records_equal(got, want, ("mono", K))
    assert not np.frombuffer(got["ch"][:, 1].tobytes(), dtype=np.uint8).any()


@gpu
def test_features_kernel_hand_made(ctx, mlib):
    is_, want = hand_made()
    got = ctx.qmdct_features_dev(is_, np.array([(0, 2)], dtype=mlib.TABLE_AUDIT_SEG_DTYPE), 1, 4)
    same(ctx._qmdct_features(got[0]), want, "hand-made on the device")


@gpu
@pytest.mark.parametrize("Gt", (10, 66, 70))
def test_batch_kernel(ctx, mlib, made, Gt):
    """stream 5 has G = S + 2 rows (66 for S = 64): Gt below, at and above it; every first_granule of the list on it and on others"""
    S = mlib.QMDCT_SLICE
    lengths, first = made["lengths"], made["first"]
    picks = [5] * 5 + [1, 2, 3, 6, 0, 9]
    rng = np.random.default_rng(Gt)
    slots = rng.permutation(len(picks))
    items = np.zeros(len(picks), dtype=mlib.QMDCT_BATCH_ITEM_DTYPE)
    for i, s in enumerate(picks):
        G = 2 * lengths[s]
        items[i] = (first[s], lengths[s], [0, 1, max(G - 1, 0), G, G + 5][i % 5], slots[i], 0)
    assert 2 * lengths[5] == S + 2
    for nch, C_ in ((2, 2), (1, 2), (1, 1)):
        got, guards = ctx.qmdct_batch_dev(made["is"], items, nch, C_, Gt)
        assert all((g.view(np.uint8) == 0x5A).all() for g in guards), (nch, C_)
        for i, s in enumerate(picks):
            want, valid = M.batch_slot(made["is"][first[s]:first[s] + lengths[s]], nch, C_, Gt, int(items["first_granule"][i]))
            assert np.array_equal(got[slots[i]], want), (nch, C_, i, s, valid)
            if nch < C_:
                assert not got[slots[i]][1].any()


# ------------------------------------------------------------------------------------------------ GPU, files
@pytest.fixture(scope="module")
def corpus(ctx, mlib, golden_dir):
    """the file list of tests/test_table_audit.py's corpus, built the same way, with test.mp3 and the streams of other encoders behind
    it (mono, mixed and short blocks, 32 and 48 kHz); with parse_stream's answer for each"""
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
    others = other_encoders(golden_dir)
    names = sorted(others)
    files += [others[n] for n in names]
    parsed = [mlib.parse_stream(f) for f in files]
    assert {p["channels"] for p in parsed} == {1, 2} and {p["sampling_rate"] for p in parsed} == {32000, 44100, 48000}
    return {"files": files, "parsed": parsed, "mono": 12 + names.index("mono_crc_32")}


def check_features(out, corpus, K, where):
    assert len(out) == len(corpus["files"])
    for i, (r, p) in enumerate(zip(out, corpus["parsed"])):
        same(r, M.features(p["is"], p["channels"], K), (where, i))
        assert (r["sampling_rate"], r["kbps"]) == (p["sampling_rate"], p["bit_rate"] // 1000), (where, i)


@gpu
@pytest.mark.parametrize("K", (576, 100))
def test_features_of_files(ctx, mlib, corpus, K):
    out = ctx.qmdct_features(corpus["files"], lines=K)
    check_features(out, corpus, K, K)
    assert [r["n_frames"] for r in out[:12]] == [60, 35, 1, 90, 260, 2, 17, 5, 48, 257, 513, 10]
    assert out[corpus["mono"]]["channels"] == 1 and out[corpus["mono"]]["hist"].shape == (1, 16)
    s = out[11]                                                      # digital silence
    assert s["max_abs"].tolist() == [0, 0] and s["hist"][:, 0].tolist() == [20 * K, 20 * K]
    if K == 576:                                                     # the order of the list does not matter
        back = ctx.qmdct_features(corpus["files"][::-1])
        for a, b in zip(out, back[::-1]):
            assert all(np.array_equal(a[k], b[k]) for k in a), (a, b)


def check_batch(batch, infos, corpus, firsts, C_, Gt, where):
    for i, (p, info) in enumerate(zip(corpus["parsed"], infos)):
        if p["channels"] > C_:
            continue
        want, valid = M.batch_slot(p["is"], p["channels"], C_, Gt, firsts[i])
        assert np.array_equal(batch[i], want), (where, i)
        assert (info["n_frames"], info["channels"], info["sampling_rate"], info["bit_rate"], info["n_granules"], info["first_granule"], info["valid_granules"]) == \
            (p["n_frames"], p["channels"], p["sampling_rate"], p["bit_rate"], 2 * p["n_frames"], firsts[i], valid), (where, i, info)


def run_batch(ctx, files, Gt, C_, firsts=None, per_file=False):
    """Context.qmdct_batch into device memory of the test's own, filled with 0x5A bytes before -> (int16 [n][C][Gt][576], infos)"""
    n = len(files)
    nbytes = n * C_ * Gt * 1152
    with ctx.device_scope() as dev:
        d = dev.alloc(nbytes)
        ctx.upload(d, np.full(nbytes, 0x5A, dtype=np.uint8))
        infos = ctx.qmdct_batch(files, d, nbytes, Gt, firsts, C_, per_file)
        return ctx.download(d, np.int16, (n, C_, Gt, 576)), infos


@gpu
def test_batch_of_files(ctx, mlib, corpus):
    files, n = corpus["files"], len(corpus["files"])
    sized = ctx.qmdct_batch(files, None, 0, 0)                       # the sizing call: the front end alone
    Gt = max(s["n_granules"] for s in sized)
    assert Gt == 2 * max(p["n_frames"] for p in corpus["parsed"]) and all(s["valid_granules"] == 0 for s in sized)
    batch, infos = run_batch(ctx, files, Gt, 2)
    check_batch(batch, infos, corpus, [0] * n, 2, Gt, "sized")
    assert sized == [dict(i, valid_granules=0) for i in infos]
    firsts = [(3 * i) % 40 for i in range(n)]                        # a window, odd first granules among them
    batch, infos = run_batch(ctx, files, 50, 2, firsts)
    check_batch(batch, infos, corpus, firsts, 2, 50, "window")
    with pytest.raises(mlib.Mp3sError) as e:                         # out_bytes a byte short: refused before anything is touched
        with ctx.device_scope() as dev:
            ctx.qmdct_batch(files, dev.alloc(n * 2 * 50 * 1152), n * 2 * 50 * 1152 - 1, 50)
    assert e.value.code == mlib.E_ARG


def test_tensors_qmdct_refuses_before_anything_is_touched():
    torch = pytest.importorskip("torch")
    from mp3stego import tensors

    class NoContext:
        device = 0

        def __getattr__(self, name):
            raise AssertionError(f"the context was asked for {name}")

    for t in (torch.zeros((2, 2, 4, 576), dtype=torch.float32), torch.zeros((2, 2, 4, 576), dtype=torch.int16), torch.zeros((2, 2, 2304), dtype=torch.int16),
              torch.zeros((2, 3, 4, 576), dtype=torch.int16), torch.zeros((2, 2, 4, 1152), dtype=torch.int16)[:, :, :, ::2]):
        with pytest.raises(ValueError):
            tensors.qmdct([b"", b""], out=t, ctx=NoContext())
    with pytest.raises(ValueError):
        tensors.qmdct([], ctx=NoContext())


@gpu
def test_tensor_of_files(ctx, mlib, corpus):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no torch.cuda")
    from mp3stego import tensors
    files, n = corpus["files"], len(corpus["files"])
    batch, infos = tensors.qmdct(files, ctx=ctx)
    Gt = 2 * max(p["n_frames"] for p in corpus["parsed"])
    assert batch.dtype == torch.int16 and tuple(batch.shape) == (n, 2, Gt, 576) and batch.device.index == ctx.device
    check_batch(batch.cpu().numpy(), infos, corpus, [0] * n, 2, Gt, "sized")
    # a window, into a tensor of the caller's that holds something else; the same through Context.qmdct_batch into the same memory
    firsts = [(3 * i) % 40 for i in range(n)]
    mine = torch.full((n, 2, 50, 576), 0x5A5A, dtype=torch.int16, device=batch.device)
    got, infos2 = tensors.qmdct(files, first_granules=firsts, ctx=ctx, out=mine)
    assert got is mine
    check_batch(mine.cpu().numpy(), infos2, corpus, firsts, 2, 50, "window")
    keep = mine.clone()
    mine.fill_(0x1111)
    torch.cuda.synchronize()
    infos3 = ctx.qmdct_batch(files, mine.data_ptr(), mine.numel() * 2, 50, firsts, 2)
    assert infos3 == infos2 and torch.equal(mine, keep)


@gpu
def test_per_file_status(ctx, mlib, corpus):
    rng = np.random.default_rng(5)
    junk = rng.integers(0, 256, size=300, dtype=np.uint8).tobytes()
    good = [corpus["files"][0], corpus["files"][corpus["mono"]], corpus["files"][6]]
    pg = [corpus["parsed"][0], corpus["parsed"][corpus["mono"]], corpus["parsed"][6]]
    files = [good[0], None, b"", junk, good[1], good[2]]
    audit = ctx.table_audits(files)                                  # the same front end: which of the odd files fail, and how
    out = ctx.qmdct_features(files)
    assert isinstance(out[1], mlib.Mp3sError) and out[1].code == mlib.E_ARG
    for i in (2, 3):
        assert isinstance(out[i], Exception) == isinstance(audit[i], Exception)
        if isinstance(out[i], Exception):
            assert out[i].code == audit[i].code
        else:
            assert out[i]["n_frames"] == 0 and out[i]["n_lines"] == 576 and not out[i]["hist"].any() and out[i]["channels"] == audit[i]["channels"]
    for i, p in zip((0, 4, 5), pg):
        same(out[i], M.features(p["is"], p["channels"]), i)
    # the batch: the same files, and a stereo file that one plane cannot hold fails alone
    batch, infos = run_batch(ctx, files, 40, 2, per_file=True)
    assert isinstance(infos[1], mlib.Mp3sError) and infos[1].code == mlib.E_ARG and not batch[1].any() and not batch[2].any() and not batch[3].any()
    for i in (2, 3):
        assert isinstance(infos[i], Exception) == isinstance(audit[i], Exception)
    for i, p in zip((0, 4, 5), pg):
        assert np.array_equal(batch[i], M.batch_slot(p["is"], p["channels"], 2, 40, 0)[0]), i
    with pytest.raises(mlib.Mp3sError):
        run_batch(ctx, files, 40, 2)
    one, infos1 = run_batch(ctx, [good[1], good[0], good[1]], 20, 1, per_file=True)
    assert isinstance(infos1[1], mlib.Mp3sError) and infos1[1].code == mlib.E_ARG and not one[1].any()
    want = M.batch_slot(pg[1]["is"], 1, 1, 20, 0)[0]
    assert np.array_equal(one[0], want) and np.array_equal(one[2], want) and infos1[0]["valid_granules"] == min(20, 2 * pg[1]["n_frames"])
    with pytest.raises(mlib.Mp3sError) as e:
        run_batch(ctx, [good[1], good[0]], 20, 1)
    assert e.value.code == mlib.E_ARG


@gpu
def test_host_parsed_front_end(ctx, mlib, corpus):
    """device_parse = 0: the front end parses on the host; both calls give the same answers"""
    old = ctx.set_option("device_parse", 0)
    try:
        check_features(ctx.qmdct_features(corpus["files"]), corpus, 576, "device_parse=0")
        n = len(corpus["files"])
        batch, infos = run_batch(ctx, corpus["files"], 30, 2)
        check_batch(batch, infos, corpus, [0] * n, 2, 30, "device_parse=0")
    finally:
        ctx.set_option("device_parse", old)
