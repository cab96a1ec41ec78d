"""The frame the list-of-files calls share (csrc/mp3s_internal.h: FileStatus, FileGroups, run_groups, finish_files, file_from_seg,
walk_whole; _lib.py: _file_list, _per_file), pinned on the four synchronous calls and on the pipe's collect: one code per file, the
FIRST failing file's text in mp3s_last_error(), that file's code as the call's when there is no status array, groups in arrival
order with every result at its own file, and the whole-file walk against what the library answered before its loops became one."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from synth_pcm import synth_pcm

CALLS = ("decode", "hide", "encode", "reveal")
GARBAGE = b"\xff\xfb\xf0\x00" * 50             # a frame header with the forbidden bitrate index: no call takes it
CUT_HEADER = b"\xff\xfb\x90"                   # ... and a file that ends inside its first header


def _arrays(items):
    """a list of byte strings (None: a null pointer; an empty one points at a byte of its own) -> (keepalive, pointers, lengths)"""
    n = len(items)
    keep = [None if f is None else np.frombuffer(f if len(f) else b"\0", dtype=np.uint8) for f in items]
    ptrs = (C.c_void_p * n)(*[None if k is None else k.ctypes.data for k in keep])
    lens = (C.c_size_t * n)(*[0 if f is None else len(f) for f in items])
    return keep, ptrs, lens


def call(mlib, which, handle, files, with_status=True, msgs=None, kbps=128):
    """one of the four calls at the C level -> (rc, status as a list, out array, owner, mp3s_last_error())"""
    L, n = mlib.lib(), len(files)
    keep, ptrs, lens = _arrays(files)
    owner, status = C.c_void_p(), (C.c_int32 * n)(*([77] * n))
    st = status if with_status else None
    out = (mlib.Decoded * n)() if which == "decode" else (mlib.File * n)()
    if which == "decode":
        rc = L.mp3s_decode_streams(handle, ptrs, lens, n, mlib.MP3S_PCM_I16, C.byref(owner), out, st)
    elif which == "hide":
        enc = [None if m is None else m.encode("utf-8") for m in (msgs or [None] * n)]
        mkeep, mptr, _ = _arrays(enc)
        mlen = (C.c_size_t * n)(*[0 if e is None else len(e) for e in enc])
        rc = L.mp3s_hide_messages(handle, ptrs, lens, n, mptr, mlen, C.byref(owner), out, st)
    elif which == "encode":
        kb = (C.c_int32 * n)(*([kbps] * n if np.isscalar(kbps) else kbps))
        rc = L.mp3s_encode_files(handle, ptrs, lens, n, kb, None, None, C.byref(owner), out, st)
    else:
        rc = L.mp3s_reveal_messages(handle, ptrs, lens, n, C.byref(owner), out, st)
    return rc, list(status), out, owner, L.mp3s_last_error().decode("utf-8", "replace")


def release(mlib, owner):
    if owner.value:
        mlib.lib().mp3s_buf_free(owner)


def check_null_lists(mlib, which, handle):
    rc, status, _, owner, _ = call(mlib, which, handle, [None] * 3, with_status=True)
    assert rc == 0 and status == [mlib.E_ARG] * 3 and owner.value, (which, rc, status)
    release(mlib, owner)
    rc, status, _, owner, _ = call(mlib, which, handle, [None] * 3, with_status=False)
    assert rc == mlib.E_ARG and not owner.value and status == [77] * 3, (which, rc, status)


def wav_of(mlib, pcm, rate):
    return mlib.wav_header(pcm.shape[0], 2, rate) + np.ascontiguousarray(pcm, dtype="<i2").tobytes()


def file_fields(f):
    return {k: getattr(f, k) for k in ("kbps", "sampling_rate", "channels", "n_frames", "hide_offset")} | {"too_long": bool(f.too_long)}


def same_file(mlib, f, single):
    """an mp3s_file of a list call against the dict the single-file call returns: bytes and fields"""
    assert C.string_at(f.data, f.len) == bytes(single["data"])
    assert file_fields(f) == {k: single[k] for k in ("kbps", "sampling_rate", "channels", "n_frames", "hide_offset", "too_long")}


# ------------------------------------------------------------------------------------------------ no device
@pytest.mark.parametrize("which", ["decode", "hide"])
def test_a_list_of_null_pointers_needs_no_device(mlib, which):
    # (a list of more than one file: the one-file calls borrow the context's spare scan)
    check_null_lists(mlib, which, C.c_void_p(16))                    # a non-null context that must not be looked at


def test_whole_file_walk_answers_what_it_answered_before_the_loops_were_one(mlib, golden_dir):
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_walk_whole_golden", os.path.join(golden_dir, "gen_walk_whole_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    g = np.load(os.path.join(golden_dir, "g11_walk_whole.npz"))
    cases = gen.cases()
    assert {k.split("__")[0] for k in g.files} == set(cases)
    for name, data in cases.items():
        got = gen.walk(mlib, data)
        want = {k.split("__")[1]: g[k] for k in g.files if k.startswith(name + "__")}
        assert set(got) == set(want), name
        for k in want:
            assert np.array_equal(got[k], want[k]), (name, k)
    assert int(g["whole__n_frames"]) == 36 and int(g["cut__n_frames"]) == 25 and int(g["irregular__regular"]) == 0
    # the walk's rate probe goes through the same loop: the frames of a pass are the stream's, a stream it does not take is refused
    assert mlib.walk_rate(cases["whole"], 0.001)[1] == 36 and mlib.walk_rate(cases["garbage"], 0.001)[1] == 0
    with pytest.raises(mlib.Mp3sError) as e:
        mlib.walk_rate(cases["irregular"], 0.001)
    assert e.value.code == mlib.E_UNSUPPORTED
    with pytest.raises(mlib.Mp3sError) as e:
        mlib.walk_rate(cases["one_byte"], 0.001)
    assert e.value.code == mlib.E_MALFORMED


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def mp3s(ctx):
    """short streams of two (sampling rate, bitrate) pairs: a (44100, 128), b (48000, 192)"""
    def make(n, rate, kbps, seed):
        return bytes(ctx.encode_pcm(synth_pcm(n, seed=seed, rate=rate), rate, kbps, None)["mp3"])
    return {"a": [make(5, 44100, 128, 71), make(12, 44100, 128, 72), make(2, 44100, 128, 73)],
            "b": [make(3, 48000, 192, 74), make(7, 48000, 192, 75)]}


@pytest.fixture(scope="module")
def wavs(mlib):
    def make(n, rate, seed):
        return wav_of(mlib, synth_pcm(n, seed=seed, rate=rate), rate)
    return {"a": [make(2, 44100, 81), make(4, 44100, 82), make(3, 44100, 83)], "b": [make(3, 48000, 84), make(2, 48000, 85)]}


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["encode", "reveal"])
def test_a_list_of_null_pointers_with_a_context(ctx, mlib, which):
    # (these two read options of the context before they look at the files: they need a real one)
    check_null_lists(mlib, which, ctx.handle)


def single_code(ctx, mlib, which, f, kbps=128):
    try:
        {"decode": ctx.decode_stream, "hide": lambda x: ctx.hide_message(x, "m"), "encode": lambda x: ctx.encode_file(x, kbps),
         "reveal": mlib.reveal_message}[which](f)
    except mlib.Mp3sError as e:
        return e.code, e.text
    return 0, ""


@pytest.mark.gpu
@pytest.mark.parametrize("which", CALLS)
def test_the_first_failing_file_names_the_call(ctx, mlib, mp3s, wavs, which):
    if which == "encode":
        w = bytearray(wavs["a"][0])
        w[24:28] = struct.pack("<I", 22050)      # tests/test_files_messages.py: 'Unsupported sampling frequency.', then 'Bad WAVE file.'
        files = [wavs["a"][0], bytes(w), b"", wavs["a"][1]]
    else:
        files = [mp3s["a"][0], GARBAGE, CUT_HEADER, mp3s["a"][1]]
    want = [single_code(ctx, mlib, which, f) for f in files]
    assert [c for c, _ in want][0::3] == [0, 0] and want[1][0] != 0 and want[2][0] != 0, want
    rc, status, out, owner, text = call(mlib, which, ctx.handle, files, msgs=["m"] * 4)
    assert rc == 0 and owner.value and status == [c for c, _ in want], (rc, status, want)
    if which == "encode":
        assert text == want[1][1] == "Unsupported sampling frequency." and want[2][1] == "Bad WAVE file."
    else:
        assert "file 1" in text and "file 2" not in text, text
    assert bytes(out[1]) == bytes(C.sizeof(out[1])) and bytes(out[2]) == bytes(C.sizeof(out[2])) and out[0].n_frames > 0 and out[3].n_frames > 0
    release(mlib, owner)
    rc, _, _, owner, text2 = call(mlib, which, ctx.handle, files, with_status=False, msgs=["m"] * 4)
    assert rc == want[1][0] and not owner.value and text2 == text, (rc, text2)


@pytest.mark.gpu
def test_groups_keep_arrival_order_and_results_stay_per_file(ctx, mlib, mp3s, wavs):
    a, b = mp3s["a"], mp3s["b"]
    files = [a[0], b[0], a[1], GARBAGE, b[1], a[2]]
    msgs = ["one", None, "a message that does not fit into twelve frames " * 4, "bad", "five", ""]
    rc, status, out, owner, _ = call(mlib, "hide", ctx.handle, files, msgs=msgs)
    assert rc == 0 and [s != 0 for s in status] == [False, False, False, True, False, False], status
    for i, (f, m) in enumerate(zip(files, msgs)):
        if i == 3:
            assert bytes(out[i]) == bytes(C.sizeof(out[i]))
            continue
        same_file(mlib, out[i], ctx.clear_file(f) if m is None else ctx.hide_message(f, m))
    assert out[2].too_long and (out[0].sampling_rate, out[0].kbps, out[1].sampling_rate, out[1].kbps) == (44100, 128, 48000, 192)
    release(mlib, owner)
    wa, wb = wavs["a"], wavs["b"]
    files, kbps = [wa[0], wb[0], wa[1], b"", wb[1], wa[2]], [128, 192, 128, 128, 192, 128]
    rc, status, out, owner, _ = call(mlib, "encode", ctx.handle, files, kbps=kbps)
    assert rc == 0 and [s != 0 for s in status] == [False, False, False, True, False, False], status
    for i, (f, k) in enumerate(zip(files, kbps)):
        if i == 3:
            assert bytes(out[i]) == bytes(C.sizeof(out[i]))
            continue
        same_file(mlib, out[i], ctx.encode_file(f, k))
    assert (out[4].sampling_rate, out[4].kbps, out[5].sampling_rate, out[5].kbps) == (48000, 192, 44100, 128)
    release(mlib, owner)


@pytest.mark.gpu
def test_collect_fills_results_like_the_direct_calls(mlib, mp3s, wavs):
    keys = ("data", "kbps", "sampling_rate", "channels", "n_frames", "too_long", "hide_offset")
    msgs = ["one", None, "three"]
    c = mlib.Context(0)
    try:
        direct_hide = c.hide_messages(mp3s["a"], msgs)
        direct_enc = c.encode_files(wavs["a"], 128, messages=msgs)
        pipe = mlib.Pipe(c, depth=2, max_job_bytes=1 << 20, scan_threads=1)
        try:
            t0 = pipe.submit(mp3s["a"], msgs)
            t1 = pipe.submit_encode(wavs["a"], 128, messages=msgs)
            assert t0 is not None and t1 is not None
            for t, direct in ((t0, direct_hide), (t1, direct_enc)):
                got_t, got = pipe.collect()
                assert got_t == t and len(got) == 3
                for r, d in zip(got, direct):
                    assert not isinstance(r, Exception) and not isinstance(d, Exception)
                    assert {k: bytes(r[k]) if k == "data" else r[k] for k in keys} == {k: bytes(d[k]) if k == "data" else d[k] for k in keys}
        finally:
            pipe.close()
    finally:
        c.close()


@pytest.mark.gpu
def test_an_empty_file_in_a_python_list_is_that_files_error(ctx, mlib, mp3s):
    good = mp3s["a"][0]
    out = ctx.hide_messages([good, b""], ["a", "b"])
    assert isinstance(out[1], mlib.Mp3sError) and out[1].code == single_code(ctx, mlib, "hide", b"")[0] != 0
    assert bytes(out[0]["data"]) == bytes(ctx.hide_message(good, "a")["data"])
    out = ctx.decode_streams([good, b""], per_file=True)
    assert isinstance(out[1], mlib.Mp3sError) and out[1].code == single_code(ctx, mlib, "decode", b"")[0] != 0
    assert out[0]["n_frames"] == 5 and np.array_equal(out[0]["pcm"], ctx.decode_stream(good)["pcm"])
