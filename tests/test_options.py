"""The options of a context (MP3S_OPT_*, include/mp3s.h): the defaults the environment gives at creation and what mp3s_ctx_set_option takes,
normalises and refuses.  The expectations below are written out from the header and from the rules the library has had; nothing is read back
from the table in csrc/mp3s_api.cpp that implements them."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

# name -> number (include/mp3s.h)
NUMBERS = {"analysis_shared": 0, "select": 1, "redo": 2, "fast_imdct": 3, "pipe_tail": 4, "chunk_frames": 5, "device_parse": 6, "file_pipeline": 7,
           "scan_threads": 8, "first_chunk_frames": 9, "file_up": 10, "huf_lanes": 11, "numa": 12, "float_fast": 13, "fail_chunk": 14,
           "fused_decode": 15, "fused_encode": 16, "pipe_dec": 17, "rate_signals": 18, "pipe_signals": 19, "wav_import": 20, "wav_resample": 21}
ON_BY_DEFAULT = {"select", "redo", "fast_imdct", "pipe_tail", "device_parse", "file_pipeline", "file_up", "numa", "fused_decode", "analysis_shared"}
FLAGS = {"analysis_shared", "select", "redo", "fast_imdct", "device_parse", "file_pipeline", "file_up", "numa", "float_fast", "fused_decode",
         "fused_encode", "pipe_dec", "rate_signals", "wav_import"}

# every environment name at once, and what the context makes of it
ENVIRONMENT = {
    "MP3S_NO_SELECT": ("", "select", 0),                 # presence disables, the empty string included
    "MP3S_NO_REDO": ("0", "redo", 0),                    # ... and whatever the value says
    "MP3S_NO_FILE_UP": ("1", "file_up", 0),
    "MP3S_NO_NUMA": ("", "numa", 0),
    "MP3S_FAST_IMDCT": ("", "fast_imdct", 1),            # a value: empty = the default
    "MP3S_DEVICE_PARSE": ("0", "device_parse", 0),
    "MP3S_FILE_PIPELINE": ("7", "file_pipeline", 1),     # a flag: non-zero = 1
    "MP3S_FLOAT_FAST": ("7", "float_fast", 1),
    "MP3S_FUSED_DECODE": ("0", "fused_decode", 0),
    "MP3S_FUSED_ENCODE": ("1", "fused_encode", 1),
    "MP3S_ANALYSIS_SHARED": ("0", "analysis_shared", 0),
    "MP3S_PIPE_DEC": ("7", "pipe_dec", 1),
    "MP3S_RATE_SIGNALS": ("1", "rate_signals", 1),
    "MP3S_WAV_IMPORT": ("7", "wav_import", 1),
    "MP3S_PIPE_TAIL": ("9", "pipe_tail", 2),             # clamped to 0..2
    "MP3S_PIPE_SIGNALS": ("7", "pipe_signals", 3),       # masked with 3
    "MP3S_WAV_RESAMPLE": ("12345", "wav_resample", 0),   # not one of the set: 0
    "MP3S_CHUNK_FRAMES": ("2", "chunk_frames", 2),       # (set_option refuses 1..3; the environment takes them)
    "MP3S_FIRST_CHUNK_FRAMES": ("-5", "first_chunk_frames", 0),   # a negative number: 0
    "MP3S_SCAN_THREADS": ("100", "scan_threads", 100),   # (set_option refuses more than 64; the environment takes them)
    "MP3S_HUF_LANES": ("62", "huf_lanes", 62),
    "MP3S_FAIL_CHUNK": ("3", "fail_chunk", 0),           # no such name: the option has none
}

# a context, every option printed; then a second value of MP3S_WAV_RESAMPLE and its option of another context
CHILD = """
import json, os, sys
sys.path.insert(0, sys.argv[1])
from mp3stego import _lib
def options():
    c = _lib.Context(0)
    try:
        return {n: c.get_option(n) for n in _lib.Context.OPTIONS}
    finally:
        c.close()
out = {"first": options()}
if "MP3S_WAV_RESAMPLE" in os.environ:
    os.environ["MP3S_WAV_RESAMPLE"] = "32000"
    out["resample_32000"] = options()["wav_resample"]
print("OPTIONS " + json.dumps(out))
"""


def _child(env_add):
    import mp3stego
    pkg = os.path.dirname(os.path.dirname(os.path.abspath(mp3stego.__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("MP3S_")}
    env.update(env_add)
    r = subprocess.run([sys.executable, "-c", CHILD, pkg], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("OPTIONS ")][-1]
    return json.loads(line[len("OPTIONS "):])


def test_defaults_without_the_environment(mlib):
    got = _child({})["first"]
    assert set(mlib.Context.OPTIONS) == set(NUMBERS) and all(mlib.Context.OPTIONS[n] == k for n, k in NUMBERS.items())
    assert got == {n: (1 if n in ON_BY_DEFAULT else 0) for n in NUMBERS}


def test_defaults_from_the_environment(mlib):
    assert {name for _, name, _ in ENVIRONMENT.values()} == set(NUMBERS)
    got = _child({var: value for var, (value, _, _) in ENVIRONMENT.items()})
    assert got["first"] == {name: want for _, name, want in ENVIRONMENT.values()}
    assert got["resample_32000"] == 32000


def _refused(mlib, ctx, name, value):
    before = ctx.get_option(name)
    with pytest.raises(mlib.Mp3sError) as e:
        ctx.set_option(name, value)
    assert e.value.code == mlib.E_ARG and ("option %d" % NUMBERS[name]) in e.value.text, (name, value, e.value.text)
    assert ctx.get_option(name) == before, (name, value)


def test_set_option_takes_normalises_and_refuses(mlib):
    import ctypes as C
    ctx = mlib.Context(0)
    try:
        for name in NUMBERS:
            _refused(mlib, ctx, name, -1)                            # negatives: every option
        for name in sorted(FLAGS):                                   # flags: 0 / 1, non-zero = 1
            for value, want in ((0, 0), (1, 1), (7, 1), (0, 0)):
                ctx.set_option(name, value)
                assert ctx.get_option(name) == want, (name, value)
        assert ctx.get_option("fused_decode") == 0 and ctx.set_option("fused_decode", 7) == 0 and ctx.get_option("fused_decode") == 1
        for name in ("chunk_frames", "first_chunk_frames"):          # 0 = chosen by the library, or at least 4
            for value in (4, 1000, 0):
                ctx.set_option(name, value)
                assert ctx.get_option(name) == value, (name, value)
            for value in (1, 2, 3):
                _refused(mlib, ctx, name, value)
        for value in (1, 64, 0):
            ctx.set_option("scan_threads", value)
            assert ctx.get_option("scan_threads") == value
        _refused(mlib, ctx, "scan_threads", 65)
        for name, value, want in (("pipe_tail", 0, 0), ("pipe_tail", 2, 2), ("pipe_tail", 5, 2), ("pipe_tail", 1, 1),   # clamped at 2
                                  ("pipe_signals", 7, 7), ("pipe_signals", 2, 2), ("pipe_signals", 0, 0),             # stored as they are
                                  ("huf_lanes", 62, 62), ("huf_lanes", 0, 0), ("fail_chunk", 3, 3), ("fail_chunk", 0, 0)):
            ctx.set_option(name, value)
            assert ctx.get_option(name) == want, (name, value)
        for value in (1, 32000, 44100, 48000, 0):                    # one of the set
            ctx.set_option("wav_resample", value)
            assert ctx.get_option("wav_resample") == value
        for value in (2, 12345, 22050, 48001):
            _refused(mlib, ctx, "wav_resample", value)
        # no such option
        L, v = mlib.lib(), C.c_int64(0)
        for number in (-1, 22):
            assert L.mp3s_ctx_set_option(ctx.handle, number, 1) == mlib.E_ARG and ("option %d" % number) in L.mp3s_last_error().decode()
            assert L.mp3s_ctx_get_option(ctx.handle, number, C.byref(v)) == mlib.E_ARG and ("option %d" % number) in L.mp3s_last_error().decode()
    finally:
        ctx.close()
