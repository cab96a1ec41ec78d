"""Table audit of a list of files: what docs/LOG.md records about Context.table_audits.  Prints one JSON line.

  python tools/table_audit_bench.py [--repeats N]

Context.table_audits(files), Context.decode_streams(files) (int16) and Context.reveal_messages(files) in one process, taken in turn,
median of N calls after a warm-up: 250 files of 40 frames, and one file of 10 000 frames, 44.1 kHz / 128 kbit/s.  Per call the wall
time and the time between mp3s_timer_start and mp3s_timer_stop on the context's stream (the events bracket the call: the host's scan
lies between them, as it does for every list call).  The audit's two kernels alone (Context.table_audit_dev on arrays already in
device memory) are timed the same way on the long file's samples."""
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


def summary(x):
    return {"median": round(statistics.median(x), 3), "min": round(min(x), 3), "max": round(max(x), 3)}


def alternate_ms(ctx, fs, repeats):
    """wall and stream-event times of each of the calls fs, taken in turn"""
    for f in fs:
        f()
        f()
    wall, dev = [[] for _ in fs], [[] for _ in fs]
    for _ in range(repeats):
        for k, f in enumerate(fs):
            ctx.timer_start()
            t0 = time.perf_counter()
            f()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            dev[k].append(ctx.timer_stop())
    return [{"wall_ms": summary(w), "timer_ms": summary(d)} for w, d in zip(wall, dev)]


def kernels_alone(ctx, _lib, mp3, repeats):
    import ctypes as C
    p, s = _lib.parse_stream(mp3), _lib.scan_stream(mp3)
    n = p["n_frames"]
    segs = np.array([(0, n)], dtype=_lib.TABLE_AUDIT_SEG_DTYPE)
    d_is, d_side, d_segs = ctx.to_device(np.ascontiguousarray(p["is"])), ctx.to_device(s["side"]), ctx.to_device(segs)
    d_out, d_units, d_prof = ctx.alloc(_lib.TABLE_AUDIT_DTYPE.itemsize), ctx.alloc(n * 64), ctx.alloc(n * 4)
    t = []
    for k in range(repeats + 3):
        ctx.timer_start()
        _lib.check(_lib.lib().mp3s_table_audit_dev(ctx.handle, d_is, d_side, n, 2, d_segs, 1, d_units, d_out, d_prof))
        ms = ctx.timer_stop()
        if k >= 3:
            t.append(ms)
    rec = ctx.download(d_out, _lib.TABLE_AUDIT_DTYPE, (1,))
    for d in (d_is, d_side, d_segs, d_out, d_units, d_prof):
        ctx.free(d)
    return {"frames": n, "regions": int(rec["regions"][0]), "timer_ms": summary(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    from mp3stego import _lib
    from synth_pcm import synth_pcm
    ctx = _lib.Context(0)
    out = {"device": ctx.device_name(), "repeats": args.repeats}
    loads = {}
    wavs = [_lib.wav_header(40 * 1152, 2, 44100) + synth_pcm(40, seed=2000 + i).astype("<i2").tobytes() for i in range(250)]
    loads["250 files of 40 frames"] = [bytes(e["data"]) for e in ctx.encode_files(wavs, 128)]
    loads["one file of 10 000 frames"] = [bytes(ctx.encode_pcm(synth_pcm(10000, seed=7), 44100, 128, None)["mp3"])]
    for name, files in loads.items():
        aud = ctx.table_audits(files)
        assert all(a["verdict"] == "clean" for a in aud)
        t = alternate_ms(ctx, [lambda: ctx.table_audits(files), lambda: ctx.decode_streams(files, _lib.MP3S_PCM_I16),
                               lambda: ctx.reveal_messages(files), lambda: ctx.table_audits(files, profile=True)], args.repeats)
        frames = sum(a["n_frames"] for a in aud)
        out[name] = {"frames": frames, "regions": sum(a["regions"] for a in aud), "table_audits": t[0], "decode_streams_i16": t[1],
                     "reveal_messages": t[2], "table_audits_with_profile": t[3],
                     "audit_over_decode_wall": round(t[0]["wall_ms"]["median"] / t[1]["wall_ms"]["median"], 3),
                     "down_bytes": {"table_audits": 104 * len(files), "table_audits_with_profile": 104 * len(files) + 4 * frames,
                                    "decode_streams_i16": frames * 1152 * 2 * 2}}
    out["kernels alone, 10 000 frames"] = kernels_alone(ctx, _lib, loads["one file of 10 000 frames"][0], args.repeats)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
