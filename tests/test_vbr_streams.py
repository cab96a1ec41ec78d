"""Streams whose headers change from frame to frame (tests/vbr_streams.py: per-frame VBR, rate switches at every wave
offset and across the 16 384-frame decode chunk, bit rates that ramp by 10x, a last frame of its own, reserved rate bits,
a late channel change) through every decode and hide route, against the oracle (pinned to the reference on such
streams by tests/test_vbr_golden.py).  The reference parses each frame under its own header (decoder/MP3_Parser.py:66-79)
and takes the WAV's rate and the re-encode bit rate from the last frame (:91, :93-98, steganography.py:137-162)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import vbr_streams as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = {"a": V.family_a, "b": V.family_b, "c": V.family_c, "d": V.family_d, "e": V.family_e}
SHORT = ("a", "c", "d", "e")                                      # (b and c_chunk_halo run through the plain routes only)
_ref = {}


class options:
    def __init__(self, ctx, **kw):
        self.ctx, self.kw = ctx, kw

    def __enter__(self):
        self.old = {}
        try:
            for k, v in self.kw.items():
                self.old[k] = self.ctx.set_option(k, v)
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *a):
        for k, v in self.old.items():
            self.ctx.set_option(k, v)


def streams(*fams, long=True):
    out = {}
    for f in fams:
        out.update(FAMILIES[f]())
    if not long:
        out = {k: v for k, v in out.items() if len(v) < 1 << 20}
    return out


def ref(orc, name, data):
    if name not in _ref:
        d = orc.decode(data)
        assert d["rc"] == 0, name
        _ref[name] = d
    return _ref[name]


def check_pcm(mlib, o, got, fmt, what):
    """float64 bit-identical to the oracle; int16 = pcm_to_i16; float32 = float64 rounded once; bits, frames, last frame's rates"""
    if fmt == mlib.MP3S_PCM_F64:
        assert got["pcm"].tobytes() == o["pcm"].tobytes(), what
    elif fmt == mlib.MP3S_PCM_F32:
        assert got["pcm"].tobytes() == o["pcm"].astype(np.float32).tobytes(), what
    else:
        assert np.array_equal(got["pcm"], oracle_i16(o)), what
    assert np.array_equal(got["bits"], o["bits"]), what
    assert (got["n_frames"], got["channels"], got["sampling_rate"], got["bit_rate"]) == \
        (o["n_frames"], o["channels"], o["sampling_rate"], o["bit_rate"]), what


def oracle_i16(o):
    import oracle_lib
    if "i16" not in o:
        o["i16"] = oracle_lib.pcm_to_i16(o["pcm"])
    return o["i16"]


def expect_hide(orc, mlib, o, message):
    """orc.decode -> pcm_to_i16 -> orc.encode at the LAST frame's rate and bit rate (test_pipe.py _expect)"""
    key = ("enc", message)
    if key not in o:
        bits = None if message is None else np.array(mlib.message_frame(message))
        e = orc.encode(oracle_i16(o), int(o["sampling_rate"]), int(o["bit_rate"]) // 1000, bits)
        assert e["rc"] == 0
        o[key] = {k: e[k] for k in ("mp3", "hide_offset", "too_long")}
        # what the reference's reveal reads back from those bytes: at 32 kHz and some bit rates (56, 96, 192 kbit/s) its
        # encoder sets the padding bit without writing the byte, so its decoder loses sync behind the first frame
        o[key]["reveal"] = mlib.message_reveal(orc.decode(e["mp3"])["bits"])
    return o[key]


def check_hide(orc, mlib, o, got, message, what):
    e = expect_hide(orc, mlib, o, message)
    assert bytes(got["data"]) == e["mp3"], what
    assert (got["kbps"], got["sampling_rate"]) == (o["bit_rate"] // 1000, o["sampling_rate"]), what
    if message is not None:
        assert got["hide_offset"] == e["hide_offset"] and got["too_long"] == e["too_long"], what
        assert mlib.reveal_message(bytes(got["data"]))["data"] == e["reveal"], what
        if o["sampling_rate"] != 32000:
            assert e["reveal"] == message.encode(), what


@pytest.mark.parametrize("fam", list(FAMILIES))
def test_decode_stream_every_format(ctx, mlib, orc, fam):
    for name, data in streams(fam).items():
        o = ref(orc, name, data)
        fmts = (mlib.MP3S_PCM_F64, mlib.MP3S_PCM_F32, mlib.MP3S_PCM_I16) if len(data) < 1 << 21 else (mlib.MP3S_PCM_F64, mlib.MP3S_PCM_I16)
        for fmt in fmts:
            check_pcm(mlib, o, ctx.decode_stream(data, fmt), fmt, (fam, name, "decode_stream", fmt))


DECODE_OPTIONS = [dict(file_pipeline=0), dict(device_parse=0), dict(fused_decode=0), dict(fast_imdct=0), dict(chunk_frames=16),
                  dict(chunk_frames=64), dict(file_up=0), dict(file_up=0, chunk_frames=16)]


@pytest.mark.parametrize("opts", DECODE_OPTIONS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_decode_routes_under_options(ctx, mlib, orc, opts):
    """decode_stream (F64, I16) and decode_file (the WAV: int16 PCM at the last frame's rate)"""
    for name, data in streams(*SHORT, "b", long=False).items():
        o = ref(orc, name, data)
        with options(ctx, **opts):
            for fmt in (mlib.MP3S_PCM_F64, mlib.MP3S_PCM_I16):
                check_pcm(mlib, o, ctx.decode_stream(data, fmt), fmt, (name, "decode_stream", opts, fmt))
            w = ctx.decode_file(data)
        assert bytes(w["data"]) == orc.wav_bytes(oracle_i16(o), o["sampling_rate"]), (name, "decode_file", opts)
        assert np.array_equal(w["bits"], o["bits"]) and w["kbps"] == o["bit_rate"] // 1000, (name, "decode_file", opts)
        assert (w["n_frames"], w["sampling_rate"], w["channels"]) == (o["n_frames"], o["sampling_rate"], o["channels"]), name


def test_float_fast_within_contract(ctx, mlib, orc):
    with options(ctx, float_fast=1):
        for name, data in streams(*SHORT, long=False).items():
            o = ref(orc, name, data)
            got = ctx.decode_stream(data, mlib.MP3S_PCM_F32)
            assert got["pcm"].shape == o["pcm"].shape, name
            assert np.abs(got["pcm"].astype(np.float64) - o["pcm"]).max() <= 1e-5 * max(1.0, np.abs(o["pcm"]).max()), (name, "float_fast")
            assert np.array_equal(got["bits"], o["bits"]) and got["sampling_rate"] == o["sampling_rate"], name


@pytest.mark.parametrize("per_file", [False, True])
def test_decode_streams_mixed_with_cbr(ctx, mlib, orc, golden_dir, per_file):
    cbr = open(os.path.join(golden_dir, "test.mp3"), "rb").read()
    vbr = streams(*SHORT, long=False)
    names, files = [], []
    for i, (n, d) in enumerate(vbr.items()):
        names += [n, "cbr"] if i % 3 == 0 else [n]
        files += [d, cbr] if i % 3 == 0 else [d]
    ref(orc, "cbr", cbr)
    stereo = [i for i, d in enumerate(files) if ref(orc, names[i], d)["channels"] == 2]
    mono = [i for i in range(len(files)) if i not in stereo]
    for fmt in (mlib.MP3S_PCM_F64, mlib.MP3S_PCM_I16):
        for sel in (stereo, mono):
            got = ctx.decode_streams([files[i] for i in sel], fmt, per_file=per_file)
            for i, g in zip(sel, got):
                check_pcm(mlib, _ref[names[i]], g, fmt, (names[i], "decode_streams", per_file, fmt))
    if per_file:                                           # a mixed batch: each file gets what it alone would
        got = ctx.decode_streams(files, mlib.MP3S_PCM_I16, per_file=True)
        for i, g in enumerate(got):
            if isinstance(g, mlib.Mp3sError):
                assert g.code == single_error(ctx, lambda: ctx.decode_stream(files[i], mlib.MP3S_PCM_I16)), names[i]
            else:
                check_pcm(mlib, _ref[names[i]], g, mlib.MP3S_PCM_I16, (names[i], "decode_streams mixed"))


HIDE_NAMES = ["a_44_joint", "a_48_stereo", "a_32_joint", "a_44_crc_some", "a_48_deep_reservoir", "c_per_frame", "c_offsets",
              "d_last_rate", "d_last_bitrate", "e_reserved_48", "e_reserved_32"]
HIDE_OPTIONS = [dict(file_pipeline=0), dict(chunk_frames=16), dict(chunk_frames=64), dict(chunk_frames=0),
                dict(file_up=0, chunk_frames=16), dict(file_up=1, chunk_frames=64), dict(fused_encode=0)]


@pytest.mark.parametrize("opts", HIDE_OPTIONS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_hide_and_clear_under_options(ctx, mlib, orc, opts):
    every = streams(*SHORT)
    for name in HIDE_NAMES:
        data = every[name]
        o = ref(orc, name, data)
        with options(ctx, **opts):
            h = ctx.hide_message(data, "vbr " + name)
            c = ctx.clear_file(data)
        check_hide(orc, mlib, o, h, "vbr " + name, (name, "hide_message", opts))
        check_hide(orc, mlib, o, c, None, (name, "clear_file", opts))


def test_ramps_and_long_streams_hide(ctx, mlib, orc):
    """32 -> 320 kbit/s and back, 3 000 frames; a last frame at another rate behind 4 000 frames: the default chunk plan"""
    every = streams("b", "d")
    for name in ("b_32_then_320", "b_320_then_32", "d_last_rate_long"):
        o = ref(orc, name, every[name])
        for opts in (dict(), dict(chunk_frames=64), dict(file_pipeline=0)):
            with options(ctx, **opts):
                h = ctx.hide_message(every[name], "ramp")
            check_hide(orc, mlib, o, h, "ramp", (name, "hide_message", opts))


def test_first_frame_sizing_fallbacks_are_reached(ctx, mlib, orc):
    """the one-file path sizes its frame table, result block and staging from the FIRST frame: a stream of small frames behind
    a large one, and a hide whose last header names another rate, go to the synchronous path -- counted in run_stats, and the
    reason is the one named (MP3S_TRACE in a child process)"""
    b, d = V.family_b(), V.family_d()
    s0 = ctx.run_stats()
    for name, data in (("b_320_then_32", b["b_320_then_32"]), ("b_320_then_32_long", b["b_320_then_32_long"])):
        w = ctx.decode_file(data)
        o = ref(orc, name, data)
        assert bytes(w["data"]) == orc.wav_bytes(oracle_i16(o), o["sampling_rate"]), name
    s1 = ctx.run_stats()
    assert s1["fallbacks"] - s0["fallbacks"] == 2, (s0, s1)
    # (the first chunk reaches as far as the message: the last frame must lie in a later chunk)
    with options(ctx, chunk_frames=16):
        c = ctx.clear_file(d["d_last_rate"])
    with options(ctx, chunk_frames=64):
        h = ctx.hide_message(d["d_last_rate_long"], "late")
    s2 = ctx.run_stats()
    check_hide(orc, mlib, ref(orc, "d_last_rate", d["d_last_rate"]), c, None, "d_last_rate clear chunk_frames=16")
    check_hide(orc, mlib, ref(orc, "d_last_rate_long", d["d_last_rate_long"]), h, "late", "d_last_rate_long chunk_frames=64")
    assert s2["fallbacks"] - s1["fallbacks"] == 2, (s1, s2)
    # the ramp the other way round: the first frame's size promises ten times the frames there are
    with options(ctx, chunk_frames=64):
        w = ctx.decode_file(b["b_32_then_320"])
    o = ref(orc, "b_32_then_320", b["b_32_then_320"])
    assert bytes(w["data"]) == orc.wav_bytes(oracle_i16(o), o["sampling_rate"]), "b_32_then_320 chunk_frames=64"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vbr_trace_child.py")], env=dict(os.environ, MP3S_TRACE="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for why in ("more frames than the file's first frame size promised", "more frames than the result block holds",
                "the last header names another rate"):
        assert "run_file: " + why in r.stderr, why


def test_decode_block_across_switches(ctx, mlib, orc):
    every = streams("c", "e", long=False)
    for name in ("c_per_frame", "c_offsets", "e_reserved_32"):
        data = every[name]
        o = ref(orc, name, data)
        n = o["n_frames"]
        for first, cnt in ((0, 7), (5, 11), (31, 3), (32, 33), (n - 4, 10), (17, 1)):
            if first >= n:
                continue
            for fmt in (mlib.MP3S_PCM_F64, mlib.MP3S_PCM_I16):
                b = ctx.decode_block(data, first, cnt, fmt)
                k = min(cnt, n - first)
                want = o["pcm"][first * 1152:(first + k) * 1152]
                want = want if fmt == mlib.MP3S_PCM_F64 else orc.pcm_to_i16(want)
                assert b["n_frames"] == k and b["pcm"].tobytes() == np.ascontiguousarray(want).tobytes(), (name, "decode_block", first, cnt, fmt)
                assert (b["sampling_rate"], b["bit_rate"]) == (o["sampling_rate"], o["bit_rate"]), (name, first)


def test_pipe_interleaves_decode_and_hide_jobs(ctx, mlib, orc):
    every = streams(*SHORT, long=False)
    names = [n for n in HIDE_NAMES if n in every]
    pipe = mlib.Pipe(ctx, depth=3, max_job_bytes=4 << 20, scan_threads=2)
    try:
        jobs = []
        for i in range(0, len(names), 2):
            grp = names[i:i + 2]
            jobs.append(("decode", grp, None))
            jobs.append(("hide", grp, ["p" + n for n in grp]))
            jobs.append(("hide", grp, None))
        results, nxt = [], 0
        while len(results) < len(jobs):
            while nxt < len(jobs):
                kind, grp, msgs = jobs[nxt]
                files = [every[n] for n in grp]
                t = pipe.submit_decode(files) if kind == "decode" else pipe.submit(files, msgs)
                if t is None:
                    break
                nxt += 1
            results.append(pipe.collect())
        assert pipe.collect() is None
    finally:
        pipe.close()
    for (kind, grp, msgs), (_, res) in zip(jobs, results):
        for k, n in enumerate(grp):
            o, r = ref(orc, n, every[n]), res[k]
            assert not isinstance(r, Exception), (n, kind, r)
            if kind == "decode":
                assert bytes(r["data"]) == orc.wav_bytes(oracle_i16(o), o["sampling_rate"]), (n, "pipe decode")
                assert np.array_equal(r["bits"], o["bits"]), (n, "pipe decode")
            else:
                check_hide(orc, mlib, o, r, None if msgs is None else msgs[k], (n, "pipe hide"))


def test_hide_messages_batch(ctx, mlib, orc):
    every = streams(*SHORT, long=False)
    names = HIDE_NAMES + ["a_44_mono"]
    msgs = [None if i % 4 == 3 else "batch " + n for i, n in enumerate(names)]
    got = ctx.hide_messages([every[n] for n in names], msgs)
    for n, m, g in zip(names, msgs, got):
        single = single_error(ctx, lambda: ctx.hide_message(every[n], m or "") if m is not None else ctx.clear_file(every[n]))
        if isinstance(g, mlib.Mp3sError):
            assert g.code == single, (n, "hide_messages")
            continue
        assert single == 0, (n, "hide_messages succeeded where the single call fails")
        check_hide(orc, mlib, ref(orc, n, every[n]), g, m, (n, "hide_messages"))


def single_error(ctx, f):
    from mp3stego import _lib
    try:
        f()
        return 0
    except _lib.Mp3sError as e:
        return e.code


@pytest.mark.parametrize("name", list(V.family_f()))
def test_late_channel_change_is_refused_on_every_route(ctx, mlib, orc, name):
    data = V.family_f()[name]
    assert orc.decode(data)["rc"] != 0
    code = single_error(ctx, lambda: ctx.decode_stream(data, mlib.MP3S_PCM_I16))
    assert code in (mlib.E_MALFORMED, mlib.E_UNSUPPORTED), code
    routes = {"decode_stream_f64": lambda: ctx.decode_stream(data, mlib.MP3S_PCM_F64),
              "decode_file": lambda: ctx.decode_file(data), "hide_message": lambda: ctx.hide_message(data, "x"),
              "clear_file": lambda: ctx.clear_file(data)}
    for opts in (dict(), dict(chunk_frames=16), dict(chunk_frames=64), dict(file_pipeline=0), dict(device_parse=0), dict(file_up=0)):
        with options(ctx, **opts):
            for r, f in routes.items():
                assert single_error(ctx, f) == code, (name, r, opts)
    cbr = V.family_d()["d_last_bitrate"]
    got = ctx.decode_streams([cbr, data], mlib.MP3S_PCM_I16, per_file=True)
    assert isinstance(got[1], mlib.Mp3sError) and got[1].code == code, (name, "decode_streams")
    check_pcm(mlib, ref(orc, "d_last_bitrate", cbr), got[0], mlib.MP3S_PCM_I16, "decode_streams neighbour")
    assert single_error(ctx, lambda: ctx.decode_streams([cbr, data], mlib.MP3S_PCM_I16)) == code, (name, "decode_streams whole")
    got = ctx.hide_messages([cbr, data], ["n", "x"])
    assert isinstance(got[1], mlib.Mp3sError) and got[1].code == code, (name, "hide_messages")
    check_hide(orc, mlib, ref(orc, "d_last_bitrate", cbr), got[0], "n", "hide_messages neighbour")
    # the fd routes leave no partial output behind
    import tempfile
    with tempfile.TemporaryFile() as fh:
        assert single_error(ctx, lambda: ctx.recode_to_fd(data, "x", fh.fileno())) == code, (name, "recode_to_fd")
        assert os.fstat(fh.fileno()).st_size == 0, (name, "recode_to_fd left output")
        assert single_error(ctx, lambda: ctx.decode_file_to_fd(data, fh.fileno())) == code, (name, "decode_file_to_fd")
        assert os.fstat(fh.fileno()).st_size == 0, (name, "decode_file_to_fd left output")
