"""WAV files as device batches (mp3s_encode_files) and as jobs of the pipe (mp3s_pipe_submit_encode), and the kernel that
brings their samples into the encoder's PCM buffer (k_wav_gather).  Every GPU comparison is equality of bytes and fields
with Context.encode_file on the same file alone -- which tests/test_files_messages.py and tests/test_gpu_parity.py pin to the
reference (g3_facade.json, g3_encode_*320.npz, g9_wav_tail.npz) and to the oracle -- or with those golden files directly."""
import ctypes as C
import hashlib
import json
import os
import struct

import numpy as np
import pytest


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def wav_bytes(pcm, rate, k=None, channels=2, tail=b""):
    """a WAV file of int16 samples with a LIST chunk of k payload bytes in front of "data" (None: no such chunk).  The
    reference looks for the tags and does not ask for the pad byte of an odd chunk: the samples start at byte 44 without
    the chunk and at 52 + k with it -- odd for odd k"""
    data = np.ascontiguousarray(pcm, dtype="<i2").tobytes()
    fmt = struct.pack("<4sIHHIIHH", b"fmt ", 16, 1, channels, rate, rate * channels * 2, channels * 2, 16)
    extra = b"" if k is None else b"LIST" + struct.pack("<I", k) + bytes(range(1, k + 1))
    body = b"WAVE" + fmt + extra + b"data" + struct.pack("<I", len(data)) + data + tail
    return b"RIFF" + struct.pack("<I", len(body)) + body


def data_offset(k):
    return 44 if k is None else 52 + k


def _same(mlib, a, b, what):
    """a = an entry of encode_files / a pipe result, b = encode_file alone (a dict) or the Mp3sError it raised"""
    if isinstance(b, Exception):
        assert isinstance(a, mlib.Mp3sError) and a.code == b.code, (what, a, b)
        return
    assert not isinstance(a, Exception), (what, a)
    assert bytes(a["data"]) == bytes(b["data"]), what
    for f in ("kbps", "sampling_rate", "channels", "n_frames", "too_long", "hide_offset"):
        assert a[f] == b[f], (what, f, a[f], b[f])


def _alone(ctx, mlib, wav, kbps, bits):
    try:
        return ctx.encode_file(wav, kbps, bits)
    except mlib.Mp3sError as e:
        return e


def mixed_list(mlib):
    """-> [(wav, bitrate, hide bits or None)]: 1 to 3 000 frames, three sampling rates, four bitrates, data offsets that are
    odd and even in both 4-byte phases, silence, messages short / too long / longer than 1 024 bits / empty, and four files
    the encoder refuses"""
    from synth_pcm import synth_pcm
    bits = lambda m: np.array(mlib.message_frame(m), dtype=np.uint8)
    quiet = synth_pcm(120, seed=305, rate=44100)
    quiet[: 30 * 1152] = 0                                      # leading and inner silence: inherited addresses (E7)
    quiet[60 * 1152:80 * 1152] = 0
    ok = synth_pcm(40, seed=311, rate=44100)
    files = [
        (wav_bytes(synth_pcm(1, seed=300), 44100), 128, None),                                        # 0: offset 44
        (wav_bytes(synth_pcm(41, seed=301), 44100, k=1), 128, None),                                  # 1: offset 53
        (wav_bytes(synth_pcm(300, seed=302), 44100, k=3), 128, bits("hello")),                        # 2: offset 55
        (wav_bytes(synth_pcm(3000, seed=303, rate=48000), 48000, k=2), 192, bits("a long file")),     # 3: offset 54
        (wav_bytes(synth_pcm(60, seed=304, rate=32000), 32000, k=5), 64, None),                       # 4: offset 57
        (wav_bytes(quiet, 44100, k=7), 128, bits("three")),                                           # 5: offset 59
        (wav_bytes(synth_pcm(25, seed=306), 44100, k=4), 320, bits("x" * 200)),                       # 6: too long for 25 frames
        (wav_bytes(synth_pcm(500, seed=307), 44100, k=9), 128, bits("long " * 60)),                   # 7: > 1 024 bits: the variants
        (wav_bytes(synth_pcm(40, seed=308, rate=48000), 48000, k=6), 192, np.zeros(0, dtype=np.uint8)),   # 8: an empty bit string
        (wav_bytes(ok[:, 0], 44100, channels=1), 128, None),                                          # 9: mono
        (wav_bytes(ok, 22050, k=1), 128, bits("no")),                                                 # 10: a rate the reference refuses
        (wav_bytes(ok, 44100, k=3)[:-10], 128, None),                                                 # 11: ends inside its last frame
        (wav_bytes(synth_pcm(33, seed=312, rate=32000), 32000, k=11), 64, bits("thirty-two")),        # 12: offset 63
        (wav_bytes(ok, 44100), 100, None),                                                            # 13: a bitrate the reference refuses
    ]
    return files


# ------------------------------------------------------------------------------------------------ CPU
def test_encode_entry_points_check_their_arguments_without_a_gpu(mlib):
    L = mlib.lib()
    one = (C.c_void_p * 1)(None)
    lens = (C.c_size_t * 1)(0)
    kbps = (C.c_int32 * 1)(128)
    out, status, owner, ticket = mlib.File(), (C.c_int32 * 1)(), C.c_void_p(), C.c_int64()
    fake = C.c_void_p(8)                       # never dereferenced: the argument checks come first
    # a null context / pipe, null arrays, no files
    assert L.mp3s_encode_files(None, one, lens, 1, kbps, None, None, C.byref(owner), C.byref(out), status) == mlib.E_ARG
    assert L.mp3s_encode_files(fake, None, lens, 1, kbps, None, None, C.byref(owner), C.byref(out), status) == mlib.E_ARG
    assert L.mp3s_encode_files(fake, one, None, 1, kbps, None, None, C.byref(owner), C.byref(out), status) == mlib.E_ARG
    assert L.mp3s_encode_files(fake, one, lens, 1, None, None, None, C.byref(owner), C.byref(out), status) == mlib.E_ARG
    assert L.mp3s_encode_files(fake, one, lens, 1, kbps, None, None, None, C.byref(out), status) == mlib.E_ARG
    assert L.mp3s_encode_files(fake, one, lens, 1, kbps, None, None, C.byref(owner), None, status) == mlib.E_ARG
    assert L.mp3s_encode_files(fake, one, lens, 0, kbps, None, None, C.byref(owner), C.byref(out), status) == mlib.E_ARG
    assert L.mp3s_encode_files(fake, one, lens, -3, kbps, None, None, C.byref(owner), C.byref(out), status) == mlib.E_ARG
    assert L.mp3s_encode_files(fake, one, lens, 1, kbps, one, None, C.byref(owner), C.byref(out), status) == mlib.E_ARG   # bits without counts
    assert L.mp3s_pipe_submit_encode(None, one, lens, 1, kbps, None, None, C.byref(ticket)) == mlib.E_ARG
    assert L.mp3s_debug_wav_gather(None, one, lens, 1, None, 0, None) == mlib.E_ARG
    assert owner.value is None


def test_wav_gather_kernel_keeps_everything_in_registers():
    """the compiler's resource listing of the new kernel: no scratch, no spilled vector register -- and its name is no
    existing kernel's prefix, nor the other way round (tests/test_build_resources.py finds kernels by the start of their names)"""
    from test_build_resources import STEP_KERNELS, OTHER_KERNELS, _find, resource_usage
    usage = resource_usage()
    u = _find(usage, "mp3s::k_wav_gather")
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, u
    assert u["LDS Size [bytes/block]"] == 0 and u["Occupancy [waves/SIMD]"] >= 8, u
    for k in STEP_KERNELS + OTHER_KERNELS:
        assert not "mp3s::k_wav_gather".startswith(k) and not k.startswith("mp3s::k_wav_gather"), k


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_encode_files_gives_the_references_own_outputs(ctx, mlib, golden_dir):
    facade = json.load(open(os.path.join(golden_dir, "g3_facade.json")))
    with open(os.path.join(golden_dir, "test.mp3"), "rb") as f:
        d = ctx.decode_file(f.read())
    wav = bytes(d["data"])
    # what the reference's facade made of test.mp3 with "ddd" and with "ddd" * 100: two files of one group, one call
    short, long = ctx.encode_files([wav, wav], d["kbps"], hide_bits=[mlib.message_frame("ddd"), mlib.message_frame("ddd" * 100)])
    assert sha(short["data"]) == facade["hide_sha256"] and short["too_long"] is facade["too_long"]
    assert sha(long["data"]) == facade["hide_long_sha256"] and long["too_long"] is facade["too_long_300"]
    # ... the same through `messages`
    a, b = ctx.encode_files([wav, wav], d["kbps"], messages=["ddd", "ddd" * 100])
    assert bytes(a["data"]) == bytes(short["data"]) and bytes(b["data"]) == bytes(long["data"])
    # the reference's own encodes of its own WAV of test.mp3, plain and with a message, at 320
    w = np.load(os.path.join(golden_dir, "g3_testmp3_wav_pcm.npz"))
    pcm = w["pcm"]
    wav2 = mlib.wav_header(pcm.shape[0], 2, 44100) + np.ascontiguousarray(pcm, dtype="<i2").tobytes()
    gp = np.load(os.path.join(golden_dir, "g3_encode_plain320.npz"))
    gh = np.load(os.path.join(golden_dir, "g3_encode_hide_ddd320.npz"))
    plain, hid = ctx.encode_files([wav2, wav2], 320, hide_bits=[None, gh["hide_bits"]])
    for r, g in ((plain, gp), (hid, gh)):
        assert len(r["data"]) == int(g["mp3_len"]) and sha(r["data"]) == bytes(g["mp3_sha256"]).decode()
        assert r["too_long"] == bool(int(g["too_long"])) and r["hide_offset"] == int(g["hide_off"][-1])
    # the frame behind a partial one: taken from what follows the samples, refused where the file ends inside it
    g = np.load(os.path.join(golden_dir, "g9_wav_tail.npz"))
    tail, bad = ctx.encode_files([g["tail_wav"].tobytes(), g["short_wav"].tobytes()], 128)
    assert tail["n_frames"] == 3 and bytes(tail["data"]) == g["tail_mp3"].tobytes()
    assert isinstance(bad, mlib.Mp3sError) and bad.code == mlib.E_UNSUPPORTED


@pytest.mark.gpu
def test_a_mixed_list_in_one_call_equals_the_files_alone(ctx, mlib):
    files = mixed_list(mlib)
    assert len(files) >= 12
    want = [_alone(ctx, mlib, *f) for f in files]
    assert [w.code for w in want if isinstance(w, Exception)] == [mlib.E_UNSUPPORTED, mlib.E_EXIT, mlib.E_UNSUPPORTED, mlib.E_EXIT]
    assert want[6]["too_long"] and not want[2]["too_long"] and not want[7]["too_long"] and len(files[7][2]) > 1024 and len(files[8][2]) == 0
    got = ctx.encode_files([f[0] for f in files], [f[1] for f in files], hide_bits=[f[2] for f in files])
    assert len(got) == len(files)
    for i, (a, b) in enumerate(zip(got, want)):
        _same(mlib, a, b, i)
    # status == NULL: the first file that fails, fails the call with its own code
    L = mlib.lib()
    n = 3
    bufs = [np.frombuffer(files[i][0], dtype=np.uint8) for i in (0, 9, 10)]
    ptr = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)(*[len(b) for b in bufs])
    kbps = (C.c_int32 * n)(128, 128, 128)
    out, owner = (mlib.File * n)(), C.c_void_p()
    assert L.mp3s_encode_files(ctx.handle, ptr, lens, n, kbps, None, None, C.byref(owner), out, None) == mlib.E_UNSUPPORTED
    assert owner.value is None


@pytest.mark.gpu
def test_the_gather_alone(ctx, mlib, golden_dir):
    """k_wav_gather against numpy.frombuffer of the same bytes: data offsets on every residue mod 16 (the files start on
    16-byte boundaries of the image, so these are the shifts the kernel sees), full-range samples, files short enough to be
    laid end to end and long enough to go up on their own, bytes behind the samples that belong to nobody's frames"""
    rng = np.random.default_rng(1607)
    wavs, want = [], []
    frames = [1, 2, 3, 70, 1, 5, 2, 64, 3, 1, 2, 7, 1, 130, 2, 3, 4]
    for i, k in enumerate([None] + list(range(16))):
        pcm = rng.integers(-32768, 32768, size=(frames[i] * 1152, 2), dtype=np.int64).astype(np.int16)
        tail = bytes(rng.integers(1, 256, size=int(rng.integers(0, 40)), dtype=np.int64).astype(np.uint8))
        wavs.append(wav_bytes(pcm, (32000, 44100, 48000)[i % 3], k=k, tail=tail))
        assert mlib.wav_parse(wavs[-1], 128)["data_offset"] == data_offset(k)
        want.append(np.frombuffer(wavs[-1], dtype="<i2", count=frames[i] * 2304, offset=data_offset(k)))
    assert sorted({data_offset(k) % 16 for k in [None] + list(range(16))}) == list(range(16))
    # the over-read frame of E3: taken from the LIST chunk behind the samples, as np.fromfile takes it
    g = np.load(os.path.join(golden_dir, "g9_wav_tail.npz"))
    tw = g["tail_wav"].tobytes()
    info = mlib.wav_parse(tw, 128)
    wavs.insert(5, tw)
    want.insert(5, np.frombuffer(tw, dtype="<i2", count=3 * 2304, offset=info["data_offset"]))
    got = ctx.debug_wav_gather(wavs)
    assert got.shape == (sum(len(w) for w in want) // 2304, 1152, 2)
    at = 0
    for i, w in enumerate(want):
        n = len(w) // 2304
        assert np.array_equal(got[at:at + n].reshape(-1), w), (i, "stream", at)
        at += n
    # ... and every file alone, and in the opposite order (other neighbours, other places in the image)
    for i in (0, 4, 13):
        assert np.array_equal(ctx.debug_wav_gather([wavs[i]]).reshape(-1), want[i]), i
    back = ctx.debug_wav_gather(wavs[::-1])
    assert np.array_equal(back.reshape(-1), np.concatenate(want[::-1]))


def _drain(pipe, jobs):
    """keep the pipe full, collect in order; jobs = [(kind, args)] -> results per job"""
    submit = {"enc": lambda a: pipe.submit_encode(a[0], a[1], hide_bits=a[2]), "hide": lambda a: pipe.submit(*a),
              "dec": lambda a: pipe.submit_decode(a)}
    out, nxt = [], 0
    while len(out) < len(jobs):
        while nxt < len(jobs):
            t = submit[jobs[nxt][0]](jobs[nxt][1])
            if t is None:
                break
            assert t == nxt
            nxt += 1
        t, res = pipe.collect()
        assert t == len(out)
        out.append(res)
    assert pipe.collect() is None
    return out


@pytest.mark.gpu
def test_encode_jobs_of_the_pipe_equal_encode_files(mlib):
    files = mixed_list(mlib)
    job = lambda idx: ("enc", ([files[i][0] for i in idx], [files[i][1] for i in idx], [files[i][2] for i in idx]))
    clean = [job([0]), job([3]), job([7]), job([0, 1, 2, 5]), job([4, 12]), job([6]), job([8, 3])]   # one group each, no failing file
    other = [job([1, 3]),                                   # two groups: the synchronous path
             job([9]), job([10, 0]), job([11]), job([2, 13, 5])]   # failing files
    ctx = mlib.Context(0)
    try:
        mp3 = bytes(ctx.encode_file(files[2][0], 128)["data"])
        mp3b = bytes(ctx.encode_file(files[5][0], 128)["data"])
        hide = ("hide", ([mp3, mp3b], ["between", None]))
        dec = ("dec", [mp3b, mp3])
        jobs = [clean[0], hide, clean[1], other[0], dec, clean[2], clean[3], other[1], hide, other[2], clean[4], dec, other[3], clean[5], other[4], clean[6]]
        want = []
        for kind, a in jobs:
            if kind == "enc":
                want.append(ctx.encode_files(a[0], a[1], hide_bits=a[2]))
            elif kind == "hide":
                want.append(ctx.hide_messages(*a))
            else:
                want.append([ctx.decode_file(m) for m in a])
        for depth, threads in ((3, 2), (1, 1), (5, 4)):
            pipe = mlib.Pipe(ctx, depth=depth, max_job_bytes=1 << 20, scan_threads=threads)
            try:
                got = _drain(pipe, jobs * 2)
                st = pipe.stats()
            finally:
                pipe.close()
            for k, res in enumerate(got):
                w = want[k % len(jobs)]
                assert len(res) == len(w), k
                for a, b in zip(res, w):
                    _same(mlib, a, b, (depth, k))
            assert st["collected"] == 2 * len(jobs) and st["fast"] + st["resolved"] + st["slow"] == st["collected"], st
            assert st["slow"] >= 2 * len(other), st
        # the jobs the stages can take -- one group, inside the slot, no failing file -- never go the other way.  (A slot is made
        # for max_job_bytes of MP3: the 3 000 frames of file 3 are 1.7 MB at 192 kbit/s and do not fit the 1 MB slots above --
        # there the job is one of those "larger than the slot" -- so this pipe has slots of 4 MB.)
        pipe = mlib.Pipe(ctx, depth=3, max_job_bytes=4 << 20, scan_threads=2)
        try:
            got = _drain(pipe, clean * 2)
            st = pipe.stats()
        finally:
            pipe.close()
        assert st["slow"] == 0 and st["fast"] + st["resolved"] == st["collected"] == 2 * len(clean), st
        for k, res in enumerate(got):
            a = clean[k % len(clean)][1]
            for r, w, kb, hb in zip(res, a[0], a[1], a[2]):
                _same(mlib, r, ctx.encode_file(w, kb, hb), k)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_an_encode_job_larger_than_the_slot_and_a_pipe_destroyed_in_flight(mlib):
    from synth_pcm import synth_pcm
    ctx = mlib.Context(0)
    try:
        wav = wav_bytes(synth_pcm(200, seed=3), 44100, k=5)
        bits = np.array(mlib.message_frame("fits nowhere"), dtype=np.uint8)
        want = ctx.encode_file(wav, 128, bits)
        pipe = mlib.Pipe(ctx, depth=2, max_job_bytes=8192, scan_threads=1)     # slots of 101 frames
        try:
            assert pipe.submit_encode([wav], 128, hide_bits=[bits]) == 0
            assert pipe.submit_encode([wav], 128, hide_bits=[bits]) == 1
            assert pipe.submit_encode([wav], 128, hide_bits=[bits]) is None    # both slots taken
            for t in range(2):
                tk, res = pipe.collect()
                assert tk == t
                _same(mlib, res[0], want, t)
            assert pipe.stats()["slow"] == 2
        finally:
            pipe.close()
        # a pipe that goes with encode jobs in flight, fast ones and one for the other path
        pipe = mlib.Pipe(ctx, depth=3, max_job_bytes=1 << 20, scan_threads=2)
        try:
            assert pipe.submit_encode([wav, wav], 128, hide_bits=[bits, None]) == 0
            assert pipe.submit_encode([wav], [320]) == 1
            assert pipe.submit_encode([wav, wav], [128, 192]) == 2
        finally:
            pipe.close()
        # the context is usable again after the pipes are gone
        _same(mlib, ctx.encode_file(wav, 128, bits), want, "after")
        _same(mlib, ctx.encode_files([wav], 128, hide_bits=[bits])[0], want, "after, batch")
    finally:
        ctx.close()


@pytest.mark.gpu
def test_submit_encode_checks_its_arguments_on_a_real_pipe(mlib):
    """null arrays, no files, bits without counts: MP3S_E_ARG, nothing is queued, and the pipe takes the next job"""
    from synth_pcm import synth_pcm
    ctx = mlib.Context(0)
    try:
        wav = wav_bytes(synth_pcm(3, seed=9), 44100, k=1)
        want = ctx.encode_file(wav, 128)
        L = mlib.lib()
        buf = np.frombuffer(wav, dtype=np.uint8)
        ptr, lens, kbps, ticket = (C.c_void_p * 1)(buf.ctypes.data), (C.c_size_t * 1)(len(wav)), (C.c_int32 * 1)(128), C.c_int64(-1)
        pipe = mlib.Pipe(ctx, depth=2, max_job_bytes=1 << 20, scan_threads=1)
        try:
            h = pipe.handle
            assert L.mp3s_pipe_submit_encode(h, None, lens, 1, kbps, None, None, C.byref(ticket)) == mlib.E_ARG
            assert L.mp3s_pipe_submit_encode(h, ptr, None, 1, kbps, None, None, C.byref(ticket)) == mlib.E_ARG
            assert L.mp3s_pipe_submit_encode(h, ptr, lens, 1, None, None, None, C.byref(ticket)) == mlib.E_ARG
            assert L.mp3s_pipe_submit_encode(h, ptr, lens, 0, kbps, None, None, C.byref(ticket)) == mlib.E_ARG
            assert L.mp3s_pipe_submit_encode(h, ptr, lens, -1, kbps, None, None, C.byref(ticket)) == mlib.E_ARG
            assert L.mp3s_pipe_submit_encode(h, ptr, lens, 1, kbps, ptr, None, C.byref(ticket)) == mlib.E_ARG
            assert ticket.value == -1 and pipe.stats()["submitted"] == 0 and pipe.collect() is None
            assert pipe.submit_encode([wav], 128) == 0
            t, res = pipe.collect()
            assert t == 0
            _same(mlib, res[0], want, "after the refused calls")
        finally:
            pipe.close()
    finally:
        ctx.close()
