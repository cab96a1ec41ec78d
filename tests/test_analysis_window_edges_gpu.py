"""The edges of the analysis window of k_enc_analysis / k_enc_fused (csrc/k_encode.hpp, enc_analysis_wave): the staging's clamped loads at the
ends of the batch and of a wave's tile, the masked window where a stream starts inside a wave, the first and the last sample a window sum
reads.  The file was written for window sums that take their samples and coefficients a half-group ahead of the products -- tried in two
forms, not kept (docs/LOG.md) --: the inputs are those on which a sum that takes a sample or a coefficient from the wrong group of columns
must differ.  Every case is compared bit for bit with the oracle's mdct_freq under both forms of the encode transform and both settings of
analysis_shared.

  sixteen_streams    sixteen one-frame streams in a row, loud random samples: the streams start at slots 0, 36, 8, 44, ... of a 64-slot wave --
                     every multiple of 4 --, so the masked window's boundary crosses the two rows of a half-group at every position there is.
                     (16 x 36 = 576 slots are nine whole waves of k_enc_analysis, and a stream's first slots hold zero window sums, so every wave
                     of this batch takes the matrixing that is exact for zeros.)
  sixteen_then_long  the same sixteen and a three-frame stream behind them: 684 slots, the batch ends in a partial wave (44 slots) that holds no
                     stream start -- the only wave of these cases that takes the matrixing with signed shares.
  impulses           one two-frame stream, silent except for one impulse per channel.  Channel 0's is the newest sample of slot 52's window
                     (row 0 back, column 31) and sits 15 rows back at column 31 for slot 67: the last read of the last half-group.  Channel 1's
                     sits at row 0 back, column 0 for slot 50 -- the first read of the prologue -- and is the oldest sample (m = 511) of slot 65's.
                     Slots 50 and 52 lie in the wave that holds the stream's start (masked window), 65 and 67 in the next one (unmasked).
  extremes           one frame of -32768 / 32767 / +-1 / 0.
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = 32                      # new samples per time slot; a frame is 36 slots, a wave of k_enc_analysis 64 slots of one channel
IMP = {0: (52, 31), 1: (50, 0)}   # channel: (row = slot whose 32 new samples hold the impulse, column)


def zero_cols():
    text = open(os.path.join(ROOT, "mp3-steganography-lib_amd", "csrc", "analysis_sign_plan.h")).read()
    return int(re.search(r"ANALYSIS_SIGN_ZERO_COLS = (0x[0-9a-f]+)", text).group(1), 16)


def window_sums(x, ew):
    """y[t][i] = sum_k ((x[32 t + 31 - (i + 64 k)] << 16) * enwindow[i + 64 k]) >> 32 of ONE stream's channel x (zeros in front of it)"""
    n = len(x) // SLOT
    xp = np.concatenate([np.zeros(512, dtype=np.int64), x.astype(np.int64)]) << 16
    idx = 512 + SLOT * np.arange(n)[:, None] + 31 - np.arange(512)[None, :]            # [slot][m]
    return ((xp[idx] * ew[None, :]) >> 32).reshape(n, 8, 64).sum(axis=1)               # m = i + 64 k


def wave_kinds(streams, ew, cols):
    """per channel and 64-slot wave of the batch: does a slot of the wave hold a zero y in a column that counts (-> the matrixing exact for zeros)"""
    y = np.concatenate([np.stack([window_sums(s[:, ch], ew) for ch in range(2)]) for s in streams], axis=1)   # [ch][slot][64]
    k = [i for i in range(64) if (cols >> i) & 1]
    z = (y[:, :, k] == 0).any(axis=2)
    n_waves = -(-z.shape[1] // 64)
    return np.array([[z[ch, 64 * w:64 * w + 64].any() for w in range(n_waves)] for ch in range(2)])


def where_in_window(sample, slot):
    """(rows back from the slot's own row, column) at which the window of `slot` reads `sample`, and its index m (0 = newest .. 511 = oldest)"""
    m = SLOT * slot + 31 - sample
    return m >> 5, 31 - (m & 31), m


def make_cases():
    rng = np.random.default_rng(41)

    def loud(frames):
        v = rng.integers(256, 32768, size=(frames * 1152, 2))
        return (v * rng.choice(np.array([1, -1]), size=v.shape)).astype(np.int16)

    sixteen = [loud(1) for _ in range(16)]
    impulses = np.zeros((2 * 1152, 2), dtype=np.int16)
    for ch, (row, col) in IMP.items():
        impulses[SLOT * row + col, ch] = (23000, -19000)[ch]
    hard = np.random.default_rng(5).choice(np.array([-32768, 32767, 0, 1, -1], dtype=np.int16), size=(1152, 2))
    return {"sixteen_streams": sixteen, "sixteen_then_long": sixteen + [loud(3)], "impulses": [impulses], "extremes": [hard]}


def check_properties(cs, ew, cols):
    """what the cases are for, shown on the arrays"""
    starts = np.cumsum([0] + [len(s) // SLOT for s in cs["sixteen_streams"]])[:-1]
    assert len(starts) == 16 and all(len(s) == 1152 for s in cs["sixteen_streams"])
    assert sorted(int(s) % 64 for s in starts) == list(range(0, 64, 4))             # every multiple of 4 inside a wave
    assert min(int(np.abs(s.astype(np.int64)).min()) for s in cs["sixteen_streams"]) >= 256
    n_slots = sum(len(s) // SLOT for s in cs["sixteen_then_long"])
    assert n_slots % 64 == 44 and n_slots // 64 == 10                                # ten whole waves and a partial one
    imp = cs["impulses"][0]
    assert len(imp) == 2 * 1152 and [int(np.count_nonzero(imp[:, ch])) for ch in range(2)] == [1, 1]
    p0, p1 = (int(np.flatnonzero(imp[:, ch])[0]) for ch in range(2))
    assert where_in_window(p0, 52) == (0, 31, 0)          # the newest sample of slot 52
    assert where_in_window(p0, 67)[:2] == (15, 31)        # row 15 back, column 31: the last read of the last half-group
    assert where_in_window(p1, 50)[:2] == (0, 0)          # row 0 back, column 0: the first read of the prologue
    assert where_in_window(p1, 65) == (15, 0, 511)        # the oldest sample of slot 65
    assert 52 // 64 == 50 // 64 == 0 and 65 // 64 == 67 // 64 == 1                   # the stream's first wave (masked) and the one behind it
    assert set(np.unique(cs["extremes"][0]).tolist()) == {-32768, 32767, 1, -1, 0} and len(cs["extremes"][0]) == 1152
    # both matrixing paths occur: a wave with a zero window sum takes the one that is exact for zeros, any other the signed shares
    kinds = {name: wave_kinds(streams, ew, cols) for name, streams in cs.items()}
    assert kinds["sixteen_streams"].shape == (2, 9) and kinds["sixteen_streams"].all()
    assert kinds["sixteen_then_long"].shape == (2, 11) and kinds["sixteen_then_long"][:, :10].all() and not kinds["sixteen_then_long"][:, 10].any()
    assert kinds["impulses"].all() and kinds["extremes"].all()


@pytest.fixture(scope="module")
def cases(mlib):
    ew = np.array(mlib.debug_tables()["enwindow"], dtype=np.int64).reshape(512)
    cs = make_cases()
    check_properties(cs, ew, zero_cols())
    return cs


@pytest.fixture(scope="module")
def wanted(orc, cases):
    return {name: np.concatenate([orc.encode(s, 44100, 320)["mdct_freq"] for s in streams]) for name, streams in cases.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sixteen_streams", "sixteen_then_long", "impulses", "extremes"])
def test_window_edges_are_bit_equal_to_the_oracle(ctx, mlib, cases, wanted, name):
    streams, want = cases[name], wanted[name]
    pcm = np.concatenate(streams)
    n = len(pcm) // 1152
    hdr = np.zeros(n, dtype=mlib.FRAME_HDR_DTYPE)
    hdr["nch"] = 2
    first = 0
    for s in streams:
        hdr["stream_first"][first:first + len(s) // 1152] = first
        first += len(s) // 1152
    old = ctx.get_option("analysis_shared"), ctx.get_option("fused_encode")
    try:
        for fused in (0, 1):
            for shared in (1, 0):
                ctx.set_option("fused_encode", fused)
                ctx.set_option("analysis_shared", shared)
                got = ctx.encode_transform(pcm, hdr)
                assert got.shape == want.shape and np.array_equal(got, want), (name, fused, shared)
    finally:
        ctx.set_option("analysis_shared", old[0])
        ctx.set_option("fused_encode", old[1])
