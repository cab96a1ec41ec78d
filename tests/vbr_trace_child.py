"""Child process of test_vbr_streams.py::test_first_frame_sizing_fallbacks_are_reached, run with MP3S_TRACE set: the
one-file path names on stderr why it hands a stream to the synchronous path.  A fresh context, so that the frame table
is sized by these calls alone."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "mp3-steganography-lib_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from mp3stego import _lib  # noqa: E402
import vbr_streams as V  # noqa: E402

ctx = _lib.Context(0)
try:
    b, d = V.family_b(), V.family_d()
    ctx.decode_file(b["b_320_then_32"])       # the frame table holds what the first (320 kbit/s) frame's size promises
    ctx.decode_file(b["b_32_then_320"])       # ... grown by a file of 32 kbit/s first frame
    ctx.decode_file(b["b_320_then_32"])       # ... so that now the result block is the bound
    ctx.set_option("chunk_frames", 16)
    ctx.clear_file(d["d_last_rate"])          # the first chunk's rate is not the last frame's
finally:
    ctx.close()
