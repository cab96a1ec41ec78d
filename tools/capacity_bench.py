"""Message capacity of a list of files: what docs/LOG.md records about Context.capacities.  Prints one JSON line.

  python tools/capacity_bench.py [--repeats N] [--only time|estimate]

time      Context.capacities(files) against Context.hide_messages(files, None) -- the call one had to make to learn the same number --
          in one process, alternating, median of N calls after warm-up: 250 files of 40 frames, and one file of 10 000 frames, 44.1 kHz /
          128 kbit/s.  With the bytes each call brings down from the device, counted from the layouts (mp3s_internal.h: small_bytes, the
          MP3 bytes of the batch; capacity_batch's block).
estimate  how far the clear capacity is from the capacity under a message: for the files of tests/test_capacity.py's first GPU test, a
          random ASCII message too long for every file is hidden (capacities with messages: hide_offset is then the exact capacity under
          that message, checked against hide_messages) and set against the clear bits, per file.
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


def up16(x):
    return (x + 15) & ~15


def time_part(ctx, _lib, synth_pcm, repeats):
    loads = {}
    wavs = [_lib.wav_header(40 * 1152, 2, 44100) + synth_pcm(40, seed=2000 + i).astype("<i2").tobytes() for i in range(250)]
    loads["250 files of 40 frames"] = [bytes(e["data"]) for e in ctx.encode_files(wavs, 128)]
    loads["one file of 10 000 frames"] = [bytes(ctx.encode_pcm(synth_pcm(10000, seed=7), 44100, 128, None)["mp3"])]
    out = {}
    for name, files in loads.items():
        cap, hid = ctx.capacities(files), ctx.hide_messages(files, [None] * len(files))
        assert all(c["n_frames"] == h["n_frames"] and c["fallback"] == 0 for c, h in zip(cap, hid))
        frames, n = sum(c["n_frames"] for c in cap), len(files)
        small = 32 + 80 * n
        t = alternate_ms([lambda: ctx.capacities(files), lambda: ctx.hide_messages(files, [None] * len(files)),
                          lambda: ctx.capacities(files, profile=True)], repeats)
        out[name] = {"frames": frames, "bits": sum(c["bits"] for c in cap),
                     "capacities_ms": t[0], "hide_messages_ms": t[1], "capacities_with_profile_ms": t[2],
                     "capacities_over_hide_messages": round(t[0]["median"] / t[1]["median"], 3),
                     "down_bytes": {"capacities": up16(small) + 16 * n, "capacities_with_profile": up16(small) + 16 * n + 4 * frames,
                                    "hide_messages": small + sum(len(h["data"]) for h in hid)}}
    return out


def estimate_part(ctx, _lib, synth_pcm):
    rng = np.random.default_rng(5)
    files = []
    for i, (rate, kbps, n) in enumerate([(44100, 128, 60), (48000, 192, 35), (44100, 128, 1), (32000, 64, 90),
                                         (44100, 128, 260), (48000, 192, 2), (44100, 128, 17), (32000, 64, 5)]):
        pcm = synth_pcm(n, rate=rate, seed=1000 + i)
        if n > 100:
            pcm[50 * 1152:70 * 1152] = 0
        files.append(bytes(ctx.encode_pcm(pcm, rate, kbps, None)["mp3"]))
    files.append(np.load(os.path.join(ROOT, "tests", "golden", "g6_synth128.npz"))["mp3"].tobytes())
    files.append(bytes(ctx.encode_pcm(synth_pcm(257, seed=1100), 44100, 128, None)["mp3"]))
    files.append(bytes(ctx.encode_pcm(synth_pcm(513, rate=48000, seed=1101), 48000, 192, None)["mp3"]))
    clear = ctx.capacities(files)
    # 12 bits a frame at the most: a message of 2 bytes per frame and some does not fit
    msgs = ["".join(chr(int(c)) for c in rng.integers(32, 127, size=2 * c["n_frames"] + 16)) for c in clear]
    under = ctx.capacities(files, msgs)
    hidden = ctx.hide_messages(files, msgs)
    rows = []
    for c, u, h in zip(clear, under, hidden):
        assert u["too_long"] and h["too_long"] and u["hide_offset"] == h["hide_offset"] == u["bits"]
        d = c["bits"] - u["hide_offset"]
        rows.append({"n_frames": c["n_frames"], "kbps": c["kbps"], "sampling_rate": c["sampling_rate"], "clear_bits": c["bits"],
                     "hide_offset": u["hide_offset"], "difference": d, "relative": round(d / max(u["hide_offset"], 1), 5), "fallback": u["fallback"]})
    return {"files": rows, "max_abs_difference": max(abs(r["difference"]) for r in rows),
            "max_abs_relative": max(abs(r["relative"]) for r in rows)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--only", choices=("time", "estimate"))
    args = ap.parse_args()
    from mp3stego import _lib
    from synth_pcm import synth_pcm
    ctx = _lib.Context(0)
    out = {"device": ctx.device_name(), "repeats": args.repeats}
    if args.only != "estimate":
        out["time"] = time_part(ctx, _lib, synth_pcm, args.repeats)
    if args.only != "time":
        out["estimate"] = estimate_part(ctx, _lib, synth_pcm)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
