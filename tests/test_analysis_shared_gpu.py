"""k_enc_analysis / k_enc_fused with a product computed once for coefficients equal up to sign (MP3S_OPT_ANALYSIS_SHARED, csrc/analysis_sign_plan.h):
every wave chooses between that matrixing and the one that shares equal coefficients only, by whether a window sum y it would negate is zero.
Each case is compared with the oracle's mdct_freq under both settings of the option and both forms of the encode transform -- all four bit-equal --
and the cases are shown, on the CPU, to contain waves of both kinds."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = 32                      # new samples per time slot; a frame is 36 slots, a wave of k_enc_analysis 64 slots of one channel


def zero_cols():
    text = open(os.path.join(ROOT, "mp3-steganography-lib_amd", "csrc", "analysis_sign_plan.h")).read()
    return int(re.search(r"ANALYSIS_SIGN_ZERO_COLS = (0x[0-9a-f]+)", text).group(1), 16)


def window_sums(x, ew):
    """y[t][i] = sum_k ((x[32 t + 31 - (i + 64 k)] << 16) * enwindow[i + 64 k]) >> 32 of ONE stream's channel x (zeros in front of it:
    the encoder's ring starts empty, MP3_Encoder.py:336-354, 532-534)"""
    n = len(x) // SLOT
    xp = np.concatenate([np.zeros(512, dtype=np.int64), x.astype(np.int64)]) << 16
    m = np.arange(512)
    idx = 512 + SLOT * np.arange(n)[:, None] + 31 - m[None, :]            # [slot][m]
    prod = (xp[idx] * ew[None, :]) >> 32
    return prod.reshape(n, 8, 64).sum(axis=1)                            # m = i + 64 k


def wave_kinds(streams, ew, cols):
    """per channel and 64-slot wave of the batch (the streams one after the other): does a slot of the wave hold a zero y in a column that counts"""
    y = np.concatenate([np.stack([window_sums(s[:, ch], ew) for ch in range(2)]) for s in streams], axis=1)   # [ch][slot][64]
    k = [i for i in range(64) if (cols >> i) & 1]
    z = (y[:, :, k] == 0).any(axis=2)
    n_waves = -(-z.shape[1] // 64)
    return np.array([[z[ch, 64 * w:64 * w + 64].any() for w in range(n_waves)] for ch in range(2)])


def make_cases():
    rng = np.random.default_rng(23)

    def loud(frames):
        v = rng.integers(256, 32768, size=(frames * 1152, 2))
        return (v * rng.choice(np.array([1, -1]), size=v.shape)).astype(np.int16)

    impulses = np.zeros((4 * 1152, 2), dtype=np.int16)
    impulses[700, 0], impulses[2900, 0] = 20000, -15000
    hard = np.random.default_rng(7).choice(np.array([-32768, 32767, 0, 1, -1], dtype=np.int16), size=(8 * 1152, 2))
    return {"one_frame": [loud(1)], "loud": [loud(4)], "silence": [np.zeros((4 * 1152, 2), dtype=np.int16)], "impulses": [impulses],
            "extremes": [hard], "two_streams": [loud(3), loud(3)]}


@pytest.fixture(scope="module")
def cases(mlib):
    """the inputs, and -- before anything is compared -- that they send waves down both ways"""
    ew = np.array(mlib.debug_tables()["enwindow"], dtype=np.int64).reshape(512)
    cols = zero_cols()
    cs = make_cases()
    kinds = {name: wave_kinds(streams, ew, cols) for name, streams in cs.items()}
    assert kinds["one_frame"].shape == (2, 1) and kinds["loud"].shape == (2, 3) and kinds["two_streams"].shape == (2, 4)
    assert kinds["silence"].all()                                         # every wave holds zeros
    assert kinds["loud"][:, 0].all() and not kinds["loud"][:, 1:].any()   # only the stream's first 16 slots do, the partial third wave too is clean
    assert kinds["impulses"][1].all() and kinds["impulses"][0].any()      # the other channel is all zero
    # the second stream starts at slot 108, inside the second wave: zeros behind a masked window, clean waves on either side
    assert kinds["two_streams"][:, 1].all() and not kinds["two_streams"][:, 2:].any()
    every = np.concatenate([k.ravel() for k in kinds.values()])
    assert every.any() and not every.all(), "the cases hold waves with a zero y and waves without"
    return cs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_frame", "loud", "silence", "impulses", "extremes", "two_streams"])
def test_shared_analysis_is_bit_equal_to_the_oracle(ctx, mlib, orc, cases, name):
    streams = cases[name]
    want = np.concatenate([orc.encode(s, 44100, 320)["mdct_freq"] for s in streams])
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
        for shared in (1, 0):
            for fused in (0, 1):
                ctx.set_option("analysis_shared", shared)
                ctx.set_option("fused_encode", fused)
                got = ctx.encode_transform(pcm, hdr)
                assert got.shape == want.shape and np.array_equal(got, want), (name, shared, fused)
    finally:
        ctx.set_option("analysis_shared", old[0])
        ctx.set_option("fused_encode", old[1])
