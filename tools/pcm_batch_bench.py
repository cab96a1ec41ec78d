"""PCM batches in device memory: what docs/LOG.md records about Context.decode_batch and the two kernels.  Prints one JSON line.

  python tools/pcm_batch_bench.py [--repeats N]

Two ways to one planar float32 batch [files][2][rows] in device memory, in one process, taken in turn, median of N calls after a
warm-up: Context.decode_batch, and the route there was before it -- Context.decode_streams (int16), numpy's transpose and scale
into the batch layout, one upload.  250 files of 40 frames, and one file of 10 000 frames, 44.1 kHz / 128 kbit/s; the results are
compared bit for bit first.  Then k_pcm_batch and k_pcm_unbatch alone on 10 000 stereo frames already in device memory, between
mp3s_timer_start and mp3s_timer_stop, beside the bytes they move divided by what mp3s_bench_copy reports.
Then the calls that take a sampling rate, each beside the same call at the native rate, taken in turn: Context.decode_batch of the two
lists at 44 100 -> 16 000 Hz, k_pcm_batch_resample alone at that ratio beside k_pcm_batch, and Context.encode_batch of a batch at
16 000 Hz (resample=1: -> 32 000 Hz) beside the same audio at 32 000 Hz (every row twice: the same number of frames to encode)."""
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
    return {"median": round(statistics.median(x), 4), "min": round(min(x), 4), "max": round(max(x), 4)}


def alternate_ms(fs, repeats):
    for f in fs:
        f()
        f()
    wall = [[] for _ in fs]
    for _ in range(repeats):
        for k, f in enumerate(fs):
            t0 = time.perf_counter()
            f()
            wall[k].append((time.perf_counter() - t0) * 1e3)
    return [summary(w) for w in wall]


def two_routes(ctx, _lib, files, repeats):
    rows = max(i["n_rows"] for i in ctx.batch_rows(files))
    nbytes = len(files) * 2 * rows * 4
    d_new, d_old = ctx.alloc(nbytes), ctx.alloc(nbytes)
    parts = {"decode_streams": [], "numpy": [], "upload": []}

    def new():
        return ctx.decode_batch(files, d_new, nbytes, rows, channels=2, fmt="f32")

    def old():
        t0 = time.perf_counter()
        dec = ctx.decode_streams(files, _lib.MP3S_PCM_I16)
        t1 = time.perf_counter()
        batch = np.zeros((len(files), 2, rows), dtype=np.float32)
        for b, d in enumerate(dec):
            batch[b, :, :len(d["pcm"])] = d["pcm"].T.astype(np.float32) / np.float32(32768)
        t2 = time.perf_counter()
        ctx.upload(d_old, batch)
        t3 = time.perf_counter()
        for k, v in zip(parts, (t1 - t0, t2 - t1, t3 - t2)):
            parts[k].append(v * 1e3)

    new()
    old()
    assert ctx.download(d_new, np.uint8, (nbytes,)).tobytes() == ctx.download(d_old, np.uint8, (nbytes,)).tobytes()
    t = alternate_ms([new, old], repeats)
    for d in (d_new, d_old):
        ctx.free(d)
    return {"files": len(files), "rows": rows, "batch_bytes": nbytes, "decode_batch_wall_ms": t[0], "decode_streams_numpy_upload_wall_ms": t[1],
            "of_which_ms": {k: summary(v[-repeats:]) for k, v in parts.items()}, "old_over_new": round(t[1]["median"] / t[0]["median"], 2)}


def kernels_alone(ctx, _lib, frames, repeats, gb_per_s):
    rows = frames * 1152
    rng = np.random.default_rng(5)
    d_pcm = ctx.to_device(rng.integers(-32768, 32768, size=(rows, 2), dtype=np.int64).astype(np.int16))
    items = np.array([(0, rows, 0, 0, 0)], dtype=_lib.PCM_BATCH_ITEM_DTYPE)
    uitems = np.array([(0, rows, 0, 0)], dtype=_lib.PCM_UNBATCH_ITEM_DTYPE)
    d_items, d_uitems = ctx.to_device(items), ctx.to_device(uitems)
    d_batch, d_back = ctx.alloc(2 * rows * 4), ctx.alloc(rows * 4)
    out = {"frames": frames, "copy_gb_per_s": round(gb_per_s, 1)}
    for fmt, esz in (("i16", 2), ("f32", 4)):
        for name, moved, call in (("k_pcm_batch", rows * 4 + 2 * rows * esz, lambda: ctx.pcm_batch_dev(d_pcm, 2, d_items, items, 2, fmt, rows, d_batch)),
                                  ("k_pcm_unbatch", 2 * rows * esz + rows * 4, lambda: ctx.pcm_unbatch_dev(d_batch, 2, fmt, rows, d_uitems, uitems, d_back))):
            t = []
            for k in range(repeats + 5):
                ctx.timer_start()
                call()
                ms = ctx.timer_stop()
                if k >= 5:
                    t.append(ms)
            out[f"{name} {fmt}"] = {"timer_ms": summary(t), "bytes_moved": moved, "at_copy_bandwidth_ms": round(moved / (gb_per_s * 1e9) * 1e3, 4)}
    for d in (d_pcm, d_items, d_uitems, d_batch, d_back):
        ctx.free(d)
    return out


def decode_at(ctx, files, rate, repeats):
    """decode_batch at the files' own rate and at `rate`, float32 stereo, in turn"""
    rows = max(i["n_rows"] for i in ctx.batch_rows(files))
    rows_at = max(i["n_rows"] for i in ctx.batch_rows(files, samplerate=rate))
    d_out = ctx.alloc(len(files) * 2 * rows * 4)
    t = alternate_ms([lambda: ctx.decode_batch(files, d_out, len(files) * 2 * rows * 4, rows, channels=2, fmt="f32"),
                      lambda: ctx.decode_batch(files, d_out, len(files) * 2 * rows_at * 4, rows_at, channels=2, fmt="f32", samplerate=rate)], repeats)
    ctx.free(d_out)
    return {"files": len(files), "rows": rows, "rows_at_rate": rows_at, "out_rate": rate, "native_wall_ms": t[0], "at_rate_wall_ms": t[1],
            "at_rate_over_native": round(t[1]["median"] / t[0]["median"], 3)}


def resample_kernel_alone(ctx, _lib, frames, L, M, repeats):
    """k_pcm_batch and k_pcm_batch_resample on the same stereo frames in device memory, float32 stereo out, between the context's timers"""
    rows = frames * 1152
    rows_at = -(-rows * L // M)
    rng = np.random.default_rng(5)
    d_pcm = ctx.to_device(rng.integers(-32768, 32768, size=(rows, 2), dtype=np.int64).astype(np.int16))
    items = np.array([(0, rows, 0, 0, 0)], dtype=_lib.PCM_BATCH_ITEM_DTYPE)
    ritems = np.array([(0, rows, 0, 0, L, M, 0)], dtype=_lib.PCM_RESAMPLE_ITEM_DTYPE)
    d_items, d_batch = ctx.to_device(items), ctx.alloc(2 * rows * 4)
    out = {"frames": frames, "L": L, "M": M}
    for name, call in (("k_pcm_batch f32", lambda: ctx.pcm_batch_dev(d_pcm, 2, d_items, items, 2, "f32", rows, d_batch)),
                       ("k_pcm_batch_resample f32", lambda: ctx.pcm_batch_resample_dev(d_pcm, 2, ritems, 2, "f32", rows_at, d_batch))):
        t = []
        for k in range(repeats + 5):
            ctx.timer_start()
            call()
            ms = ctx.timer_stop()
            if k >= 5:
                t.append(ms)
        out[name] = {"timer_ms": summary(t)}
    for d in (d_pcm, d_items, d_batch):
        ctx.free(d)
    return out


def encode_at(ctx, n_items, frames, repeats):
    """encode_batch of int16 stereo items at 16 000 Hz (resample=1: 32 000 Hz) and of the same audio at 32 000 Hz (every row twice), in turn"""
    from synth_pcm import synth_pcm
    rows = frames * 1152
    x = np.stack([np.ascontiguousarray(synth_pcm(frames, seed=3000 + i).T) for i in range(n_items)])      # [items][2][rows]
    d_16, d_32 = ctx.to_device(x), ctx.to_device(np.repeat(x, 2, axis=2))
    t = alternate_ms([lambda: ctx.encode_batch(d_32, n_items, 2, "i16", 2 * rows, [2 * rows] * n_items, 32000, 128),
                      lambda: ctx.encode_batch(d_16, n_items, 2, "i16", rows, [rows] * n_items, 16000, 128, resample=1)], repeats)
    for d in (d_16, d_32):
        ctx.free(d)
    return {"items": n_items, "frames_in": frames, "frames_out": 2 * frames, "native_32000_wall_ms": t[0], "from_16000_wall_ms": t[1],
            "resampled_over_native": round(t[1]["median"] / t[0]["median"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    from mp3stego import _lib
    from synth_pcm import synth_pcm
    ctx = _lib.Context(0)
    out = {"device": ctx.device_name(), "repeats": args.repeats}
    wavs = [_lib.wav_header(40 * 1152, 2, 44100) + synth_pcm(40, seed=2000 + i).astype("<i2").tobytes() for i in range(250)]
    loads = {"250 files of 40 frames": [bytes(e["data"]) for e in ctx.encode_files(wavs, 128)],
             "one file of 10 000 frames": [bytes(ctx.encode_pcm(synth_pcm(10000, seed=7), 44100, 128, None)["mp3"])]}
    for name, files in loads.items():
        out[name] = two_routes(ctx, _lib, files, args.repeats)
    out["kernels alone"] = kernels_alone(ctx, _lib, 10000, args.repeats, ctx.bench_copy())
    for name, files in loads.items():
        out[name + " at 16 000 Hz"] = decode_at(ctx, files, 16000, args.repeats)
    out["resample kernel alone"] = resample_kernel_alone(ctx, _lib, 10000, 160, 441, args.repeats)
    out["encode 250 items of 40 frames from 16 000 Hz"] = encode_at(ctx, 250, 40, max(3, args.repeats // 3))
    out["encode one item of 10 000 frames from 16 000 Hz"] = encode_at(ctx, 1, 10000, max(3, args.repeats // 3))
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
