"""What hiding changed, for a list of file pairs: what docs/LOG.md records about Context.pcm_distortions.  Prints one JSON line.

  python tools/distortion_bench.py [--repeats N] [--once]

Context.pcm_distortions(hidden, clear) against the way to the same numbers without it -- Context.decode_streams of both lists and the
reduction in numpy (int64) --, in one process, alternating, median of N calls after warm-up: 250 pairs of 40 frames, and one pair of
10 000 frames, 44.1 kHz / 128 kbit/s, the hide re-encode of a message against the clear re-encode of the same input.  With the bytes each
way brings down from the device, counted from the layouts (mp3s_distortion_files.cpp: 40 bytes a pair, 32 a compared frame with the
profile; decode_streams: the int16 PCM of both lists).  The two ways are compared field by field before anything is timed.
--once stops behind that comparison (one pcm_distortions call per workload): the run to put under `rocprofv3 --kernel-trace --stats` for
the two kernels' own times.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mp3-steganography-lib_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def alternate_ms(fs, repeats):
    """median / min / max of each of the calls fs, taken in turn"""
    for f in fs:
        f()
        f()
    t = [[] for _ in fs]
    for _ in range(repeats):
        for k, f in enumerate(fs):
            t0 = time.perf_counter()
            f()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return [{"median": round(statistics.median(x), 3), "min": round(min(x), 3), "max": round(max(x), 3)} for x in t]


def numpy_way(ctx, a, b):
    """decode both lists, every sample to the host, the sums in int64"""
    out = []
    for x, y in zip(ctx.decode_streams(a), ctx.decode_streams(b)):
        rows = min(len(x["pcm"]), len(y["pcm"]))
        p, q = x["pcm"][:rows].astype(np.int64).reshape(-1), y["pcm"][:rows].astype(np.int64).reshape(-1)
        d = p - q
        ne = np.nonzero(d)[0]
        out.append({"err2": int((d * d).sum()), "sig2": int((p * p).sum()), "max_abs": int(np.abs(d).max()) if len(d) else 0, "n_diff": len(ne),
                    "first_diff": int(ne[0]) if len(ne) else -1, "n_frames": rows // 1152})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    from mp3stego import _lib
    from synth_pcm import synth_pcm
    ctx = _lib.Context(0)
    rng = np.random.default_rng(3)
    loads = {}
    wavs = [_lib.wav_header(40 * 1152, 2, 44100) + synth_pcm(40, seed=2000 + i).astype("<i2").tobytes() for i in range(250)]
    loads["250 pairs of 40 frames"] = [bytes(e["data"]) for e in ctx.encode_files(wavs, 128)]
    loads["one pair of 10 000 frames"] = [bytes(ctx.encode_pcm(synth_pcm(10000, seed=7), 44100, 128, None)["mp3"])]
    out = {"device": ctx.device_name(), "repeats": args.repeats, "time": {}}
    for name, files in loads.items():
        msgs = ["".join(chr(int(c)) for c in rng.integers(32, 127, size=24)) for _ in files]
        clear = [h["data"] for h in ctx.hide_messages(files, [None] * len(files))]
        hidden = [h["data"] for h in ctx.hide_messages(files, msgs)]
        got, want = ctx.pcm_distortions(hidden, clear), numpy_way(ctx, hidden, clear)
        for g, w in zip(got, want):
            assert all(int(g[k]) == w[k] for k in w), (g, w)
        if args.once:
            continue
        frames, n = sum(w["n_frames"] for w in want), len(files)
        t = alternate_ms([lambda: ctx.pcm_distortions(hidden, clear), lambda: numpy_way(ctx, hidden, clear),
                          lambda: ctx.pcm_distortions(hidden, clear, profile=True), lambda: ctx.decode_streams(hidden + clear)], args.repeats)
        out["time"][name] = {"frames_compared": frames, "pairs_changed": sum(1 for w in want if w["err2"]),
                             "pcm_distortions_ms": t[0], "decode_streams_and_numpy_ms": t[1], "pcm_distortions_with_profile_ms": t[2],
                             "decode_streams_of_both_lists_alone_ms": t[3],
                             "pcm_distortions_over_numpy_way": round(t[0]["median"] / t[1]["median"], 3),
                             "down_bytes": {"pcm_distortions": 40 * n, "pcm_distortions_with_profile": (40 * n + 15) // 16 * 16 + 32 * frames,
                                            "decode_streams_and_numpy": 2 * frames * 4608}}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
