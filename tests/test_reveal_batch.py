"""Reveal over a list of files as one device batch (mp3s_reveal_messages / Context.reveal_messages) and its device step alone
(mp3s_reveal_bits_dev / Context.reveal_bits, kernel k_reveal).  Reference: decoder/Frame.py:676-685, decoder/util.py:67-81 and
steganography.py:103-131.  The checker throughout is the host path -- mlib.scan_stream(...)["bits"], mlib.message_reveal and
mlib.reveal_message -- which tests/test_decode_corpus.py, tests/test_fuzz.py and tests/test_files_messages.py pin to the reference."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import frame_synth
from test_fuzz import header_mutants, mutants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = ["books_4_14_id3", "joint_ms_blocks_48", "long_reservoir_44", "mixed_blocks_44", "mono_crc_32", "no_reservoir_32k_lowrate"]
KEYS = ("data", "kbps", "sampling_rate", "channels", "n_frames")


@functools.lru_cache(maxsize=None)
def corpus_files(golden_dir):
    g = np.load(os.path.join(golden_dir, "g7_decode_corpus.npz"))
    files = [g[n + "__mp3"].tobytes() for n in CORPUS]
    files.append(open(os.path.join(golden_dir, "test.mp3"), "rb").read())
    files.append(open(os.path.join(golden_dir, "g3_hide_ddd.mp3"), "rb").read())
    files.append(np.load(os.path.join(golden_dir, "g6_synth128.npz"))["mp3"].tobytes())
    return tuple(files)


def same_as_single(mlib, got, data):
    """one entry of reveal_messages against reveal_message of that file alone"""
    want = mlib.reveal_message(data)
    assert not isinstance(got, Exception), got
    for k in KEYS:
        assert got[k] == want[k], k
    assert len(got["bits"]) == len(want["bits"]) and np.array_equal(got["bits"], want["bits"])


def against_scan(mlib, got, data):
    """... against the byte-level scan: the scan's error code, or the message of the scan's bits"""
    try:
        s = mlib.scan_stream(data)
    except mlib.Mp3sError as e:
        assert isinstance(got, mlib.Mp3sError) and got.code == e.code, (got, e)
        return False
    assert not isinstance(got, Exception), got
    assert got["data"] == mlib.message_reveal(s["bits"])
    assert len(got["bits"]) == len(s["bits"]) and np.array_equal(got["bits"], s["bits"])
    assert got["n_frames"] == s["n_frames"] and got["channels"] == s["channels"] and got["sampling_rate"] == s["sampling_rate"]
    assert got["kbps"] == s["bit_rate"] // 1000
    return True


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_argument_checks_do_not_need_a_gpu(mlib):
    L = mlib.lib()
    nothing = C.c_char()
    one = (C.c_void_p * 1)(C.addressof(nothing))
    lens = (C.c_size_t * 1)(0)
    out, status, owner = (mlib.File * 1)(), (C.c_int32 * 1)(), C.c_void_p()
    fake = C.c_void_p(16)                                            # a non-null context that must not be looked at
    assert L.mp3s_reveal_messages(None, one, lens, 1, C.byref(owner), out, status) == mlib.E_ARG
    assert L.mp3s_reveal_messages(fake, None, lens, 1, C.byref(owner), out, status) == mlib.E_ARG
    assert L.mp3s_reveal_messages(fake, one, None, 1, C.byref(owner), out, status) == mlib.E_ARG
    assert L.mp3s_reveal_messages(fake, one, lens, 1, None, out, status) == mlib.E_ARG
    assert L.mp3s_reveal_messages(fake, one, lens, 1, C.byref(owner), None, status) == mlib.E_ARG
    assert L.mp3s_reveal_messages(fake, one, lens, -1, C.byref(owner), out, status) == mlib.E_ARG
    args = [fake] * 2 + [0] + [fake] * 2 + [1] + [fake] * 4
    for k in (0, 1, 3, 4, 6, 7, 8, 9):
        a = list(args)
        a[k] = None
        assert L.mp3s_reveal_bits_dev(*a) == mlib.E_ARG, k
    a = list(args)
    a[5] = -1
    assert L.mp3s_reveal_bits_dev(*a) == mlib.E_ARG
    a[5] = 65536                                                     # a frame reference names its stream in 16 bits
    assert L.mp3s_reveal_bits_dev(*a) == mlib.E_ARG


def test_tile_constant_is_the_headers(mlib):
    txt = open(os.path.join(ROOT, "include", "mp3s.h")).read()
    assert int(re.search(r"#define MP3S_REVEAL_TILE (\d+)", txt).group(1)) == mlib.REVEAL_TILE
    assert mlib.REVEAL_TILE % 64 == 0


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_corpus_batch_equals_single_file_reveal(ctx, mlib, golden_dir):
    # what the fixture is worth: window-switching granules that inherit a non-zero third table index, odd bit counts
    g = np.load(os.path.join(golden_dir, "g7_decode_corpus.npz"))
    inherited = 0
    for n in CORPUS:
        nch = int(g[n + "__nch"])
        bt, ts = g[n + "__si_block_type"][:, :, :nch], g[n + "__table_select"][:, :, :nch]
        inherited += int(((bt != 0) & (ts[..., 2] != 0)).sum())
        assert len(g[n + "__bits"]) % 8 != 0, n
    assert inherited >= 20
    files = corpus_files(golden_dir)
    out = ctx.reveal_messages(files)
    assert len(out) == len(files) == 9
    for f, r in zip(files, out):
        same_as_single(mlib, r, f)
    for n, r in zip(CORPUS, out):
        assert np.array_equal(r["bits"], g[n + "__bits"]), n
    assert out[7]["data"] == b"ddd"
    assert len({(r["sampling_rate"], r["kbps"], r["channels"]) for r in out}) >= 5     # one batch of mixed streams


TILE_SEED = 3


@functools.lru_cache(maxsize=None)
def tile_streams(T):
    """stereo, mono, stereo, ... of 1, 63, 64, 65, T-1, T, T+1 and 2T+3 frames; every block type, little main data"""
    out = []
    for k, n in enumerate((1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3)):
        out.append(frame_synth.make_stream(TILE_SEED * 100 + k, n, mode=3 if k % 2 else 0, crc=(k == 3), id3=(k == 0),
                                           block_types=(0, 1, 2, 3), fill=0.05))
    return tuple(out)


def last_definer(unit, f, gr, ch):
    """the last frame in front of frame f whose granule (gr, ch) has no window switching (it leaves the third index behind), or -1"""
    for g in range(f - 1, -1, -1):
        if unit[g]["window_switching"][gr][ch] == 0:
            return g
    return -1


@pytest.mark.gpu
def test_tile_and_wave_boundaries(ctx, mlib):
    T = mlib.REVEAL_TILE
    files = tile_streams(T)
    scans = [mlib.scan_stream(f) for f in files]
    assert [s["n_frames"] for s in scans] == [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]
    assert [s["channels"] for s in scans] == [2, 1] * 4
    # the data exercise the carry across a tile: a window-switching granule in the first frame of a tile inherits a non-zero
    # index that a granule of the tile before left behind
    carries = 0
    for s in scans:
        u = s["side"]["unit"]
        for f in range(T, s["n_frames"], T):
            for gr in range(2):
                for ch in range(s["channels"]):
                    if u[f]["window_switching"][gr][ch] and u[f]["table_select"][gr][ch][2]:
                        d = last_definer(u, f, gr, ch)
                        assert f - T <= d < f and u[d]["table_select"][gr][ch][2] == u[f]["table_select"][gr][ch][2]
                        carries += 1
    assert carries >= 2
    # ... and the restart at a stream: a later stream of the batch opens with a window-switching granule, which reads 0 where
    # the stream in front of it left a non-zero index
    restarts = 0
    for k in range(1, len(scans)):
        u, p = scans[k]["side"]["unit"], scans[k - 1]["side"]["unit"]
        if u[0]["window_switching"][0][0]:
            assert u[0]["table_select"][0][0][2] == 0
            d = last_definer(p, scans[k - 1]["n_frames"], 0, 0)
            restarts += d >= 0 and p[d]["table_select"][0][0][2] != 0
    assert restarts >= 1
    for f, s in zip(files, scans):
        w = mlib.walk_stream(f)
        assert w["regular"]
        packed, n_bits = ctx.reveal_bits(f, w)
        assert n_bits == len(s["bits"])
        assert np.array_equal(packed, np.packbits(s["bits"]))
    out = ctx.reveal_messages(files)
    for f, r in zip(files, out):
        same_as_single(mlib, r, f)


@pytest.mark.gpu
def test_round_trip_of_a_message_longer_than_a_tile(ctx, mlib):
    from synth_pcm import synth_pcm
    T = mlib.REVEAL_TILE
    rng = np.random.default_rng(21)
    msg = "".join(chr(int(c)) for c in rng.integers(32, 127, size=12 * T // 8 + 16))
    assert len(msg) > 12 * T // 8                                     # more bits than one tile of frames can hold
    mp3 = ctx.encode_pcm(synth_pcm(360, seed=77), 44100, 128, None)["mp3"]
    hidden = ctx.hide_messages([mp3, mp3], [msg, None])
    assert not any(isinstance(h, Exception) for h in hidden)
    out = ctx.reveal_messages([hidden[0]["data"], hidden[1]["data"]])
    k = len(msg) if not hidden[0]["too_long"] else int(hidden[0]["hide_offset"]) // 8 - len(f"{len(msg)}#")
    assert k > 12 * T // 8 and bytes(out[0]["data"])[:k] == msg.encode()[:k]
    assert out[1]["data"] == b""
    same_as_single(mlib, out[0], hidden[0]["data"])
    same_as_single(mlib, out[1], hidden[1]["data"])


@pytest.mark.gpu
def test_per_file_status_and_host_fallback(ctx, mlib, golden_dir):
    files = corpus_files(golden_dir)
    good = files[6]                                                   # test.mp3
    res = files[CORPUS.index("long_reservoir_44")]
    s = mlib.scan_stream(res)
    first = len(res) - int(s["frame_size"].sum())
    cut_res = res[first + int(s["frame_size"][:3].sum()):]            # its first frames point in front of the file
    try:
        assert not mlib.walk_stream(cut_res)["regular"]
    except mlib.Mp3sError:
        pass
    batch = [good, b"", b"not an mp3 file at all" * 10] + [good[:-c] for c in (1, 5, 40, 1045)] + [good + b"\x00" * 700, cut_res]
    muts = list(header_mutants(mlib, good, 40, 31)) + list(mutants(good, 40, 32))
    batch += muts + [good]
    regular = 0
    for m in muts:
        try:
            w = mlib.walk_stream(m)
            regular += bool(w["regular"] and w["n_frames"])
        except mlib.Mp3sError:
            pass
    assert regular >= len(muts) / 4                                   # otherwise only the fallback would be exercised
    out = ctx.reveal_messages(batch)
    assert len(out) == len(batch)
    ok = sum(against_scan(mlib, r, f) for f, r in zip(batch, out))
    assert isinstance(out[1], mlib.Mp3sError) and ok >= len(batch) // 2
    same_as_single(mlib, out[0], good)
    same_as_single(mlib, out[-1], good)
    # status == NULL: the first failure fails the call, with that file's code
    n = len(batch)
    bufs = [np.frombuffer(b, dtype=np.uint8) for b in batch]
    nothing = C.c_char()
    ptr = (C.c_void_p * n)(*[b.ctypes.data if len(b) else C.addressof(nothing) for b in bufs])
    lens = (C.c_size_t * n)(*[len(b) for b in bufs])
    res_, owner = (mlib.File * n)(), C.c_void_p()
    assert mlib.lib().mp3s_reveal_messages(ctx.handle, ptr, lens, n, C.byref(owner), res_, None) == out[1].code


@pytest.mark.gpu
def test_a_list_in_several_launches(ctx, mlib, golden_dir):
    files = corpus_files(golden_dir) + tile_streams(mlib.REVEAL_TILE)[:4]
    one = ctx.reveal_messages(files)
    for cap in (1, 4):
        parts = ctx.reveal_messages(files, _max_streams=cap)
        assert len(parts) == len(one)
        for a, b in zip(one, parts):
            assert not isinstance(a, Exception) and not isinstance(b, Exception)
            assert all(a[k] == b[k] for k in KEYS) and np.array_equal(a["bits"], b["bits"])
