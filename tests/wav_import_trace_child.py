"""Child process of test_wav_import.py::test_canonical_files_keep_the_gather, run with MP3S_TRACE and MP3S_WAV_IMPORT set:
encode_files names on stderr how many streams of a batch went through k_wav_gather and how many through k_wav_import."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "mp3-steganography-lib_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

from mp3stego import _lib  # noqa: E402
from synth_pcm import synth_pcm  # noqa: E402
from test_encode_batch import wav_bytes  # noqa: E402
import wav_import_files as W  # noqa: E402

ctx = _lib.Context(0)
try:
    assert ctx.get_option("wav_import") == 1
    pcm = synth_pcm(3, seed=41)
    canonical = [wav_bytes(pcm, 44100), wav_bytes(pcm[:2304], 44100, k=3)]
    other = [W.wav_file(pcm[:, 0], W.S16), W.wav_file(pcm[:1700], W.S16), W.wav_file(pcm.astype(np.int64) << 8, W.S24)]
    print("batch canonical", file=sys.stderr, flush=True)
    ctx.encode_files(canonical, 128)
    print("batch mixed", file=sys.stderr, flush=True)
    ctx.encode_files(canonical + other, 128)
    print("batch other", file=sys.stderr, flush=True)
    ctx.encode_files(other, 128)
finally:
    ctx.close()
