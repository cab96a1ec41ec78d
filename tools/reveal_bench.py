"""Reveal over a list of files: Context.reveal_messages (one device batch, k_reveal) against a loop of the host's
mlib.reveal_message over the same files.  Two workloads: 250 files of 40 frames (the files README.md quotes for hide_messages)
and one 10 000-frame file, 44.1 kHz / 128 kbit/s, each with a message hidden.  Every result of the batch is compared with the
loop's before anything is timed.  Prints one JSON line.

  python tools/reveal_bench.py [--repeats N] [--only short|long] [--once]

--once runs each batch call a few times and nothing else: the run to put under `rocprofv3 --kernel-trace --stats` for the
time of k_reveal alone.
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


def median_ms(f, repeats):
    f()
    f()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--only", choices=("short", "long"))
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    from mp3stego import _lib
    from synth_pcm import synth_pcm
    ctx = _lib.Context(0)
    loads = {}
    if args.only != "long":
        wavs = [_lib.wav_header(40 * 1152, 2, 44100) + synth_pcm(40, seed=2000 + i).astype("<i2").tobytes() for i in range(250)]
        enc = ctx.encode_files(wavs, 128, messages=["message %d" % i for i in range(250)])
        loads["250 files of 40 frames"] = [bytes(e["data"]) for e in enc]
    if args.only != "short":
        loads["one file of 10 000 frames"] = [bytes(ctx.encode_pcm(synth_pcm(10000, seed=7), 44100, 128, _lib.message_frame("a long file's message"))["mp3"])]
    out = {"device": ctx.device_name(), "repeats": args.repeats, "workloads": {}}
    for name, files in loads.items():
        got, want = ctx.reveal_messages(files), [_lib.reveal_message(f) for f in files]
        for g, w in zip(got, want):
            assert g["data"] == w["data"] and np.array_equal(g["bits"], w["bits"]) and all(g[k] == w[k] for k in ("kbps", "sampling_rate", "channels", "n_frames"))
        if args.once:
            for _ in range(5):
                ctx.reveal_messages(files)
            continue
        batch = median_ms(lambda: ctx.reveal_messages(files), args.repeats)
        loop = median_ms(lambda: [_lib.reveal_message(f) for f in files], args.repeats)
        out["workloads"][name] = {"frames": sum(w["n_frames"] for w in want), "bytes": sum(len(f) for f in files),
                                  "reveal_messages_ms": {"median": round(batch[0], 3), "min": round(batch[1], 3), "max": round(batch[2], 3)},
                                  "host_loop_ms": {"median": round(loop[0], 3), "min": round(loop[1], 3), "max": round(loop[2], 3)},
                                  "loop_over_batch": round(loop[0] / batch[0], 2), "first_message": got[0]["data"].decode("latin-1")}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
