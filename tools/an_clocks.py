"""Phase clocks of k_enc_analysis (library built with -DMP3S_AN_CLOCKS=1: every wave writes the shader clocks it spent in staging, window sums,
matrixing and write-out into a device array, read back through mp3s_debug_an_clocks).  usage (GPU box): python tools/an_clocks.py [frames]"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mp3-steganography-lib_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from mp3stego import _lib
from synth_pcm import synth_pcm
n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
ctx = _lib.Context(0)
pcm = synth_pcm(n, seed=7)
hdr = np.zeros(n, dtype=_lib.FRAME_HDR_DTYPE)
hdr["nch"] = 2
ctx.set_option("fused_encode", 0)
for _ in range(3):
    ctx.encode_transform(pcm, hdr)
buf = np.zeros(4096 * 8, dtype=np.uint32)
assert _lib.lib().mp3s_debug_an_clocks(buf.ctypes.data_as(ctypes.c_void_p)) == 0
d = buf.reshape(-1, 8).astype(np.int64)
d = d[d[:, 4] > 0]
names = ["staging", "window sums", "matrixing", "write-out", "whole wave"]
for k in range(5):
    print("%-12s median %7d  mean %9.1f  max %7d clocks  (%4.1f %% of the wave)" % (names[k], np.median(d[:, k]), d[:, k].mean(), d[:, k].max(),
                                                                                  100.0 * d[:, k].sum() / d[:, 4].sum()))
print("waves", len(d), "masked window", int((d[:, 5] & 1).sum()), "signed shares", int((d[:, 5] >> 1).sum()))
ctx.close()
