"""QMDCT features and batches of a list of files: what docs/LOG.md records about Context.qmdct_features and tensors.qmdct.  Prints one
JSON line.

  python tools/qmdct_bench.py [--repeats N] [--host-repeats N]

Context.qmdct_features(files), Context.table_audits(files) (the same front half of the decode: the difference is the kernels), the
spectra as a batch (tensors.qmdct into a tensor made once; Context.qmdct_batch into device memory of the library where torch sees no
device) in one process, taken in turn, median of N calls after a warm-up: 250 files of 40 frames, and one file of 10 000 frames,
44.1 kHz / 128 kbit/s.  Per call the wall time and the time between mp3s_timer_start and mp3s_timer_stop on the context's stream.  The
host alternative -- a loop of parse_stream and the numpy model of tests/qmdct_model.py -- is taken a few times only.  The two kernels
alone (mp3s_qmdct_features_dev, mp3s_qmdct_batch_dev on arrays already in device memory) are timed the same way on the long file's
samples and set beside the time to stream the same bytes at mp3s_bench_copy's bandwidth."""
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


def batch_call(ctx, files, granules):
    """-> (what writes the batch, its name): through a torch tensor made once where torch sees the device, else into memory of the library's"""
    try:
        import torch
        if torch.cuda.is_available():
            from mp3stego import tensors
            out = torch.empty((len(files), 2, granules, 576), dtype=torch.int16, device=torch.device("cuda", ctx.device))
            return (lambda: tensors.qmdct(files, ctx=ctx, out=out)), "tensors.qmdct"
    except ImportError:
        pass
    nbytes = len(files) * 2 * granules * 1152
    d = ctx.alloc(nbytes)
    return (lambda: ctx.qmdct_batch(files, d, nbytes, granules)), "Context.qmdct_batch"


def host_alternative(_lib, files, repeats):
    import qmdct_model as M
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for f in files:
            p = _lib.parse_stream(f)
            M.features(p["is"], p["channels"])
        t.append((time.perf_counter() - t0) * 1e3)
    return {"wall_ms": summary(t), "repeats": repeats}


def kernels_alone(ctx, _lib, mp3, repeats, copy_gbs):
    p = _lib.parse_stream(mp3)
    n = p["n_frames"]
    segs = np.array([(0, n)], dtype=_lib.TABLE_AUDIT_SEG_DTYPE)
    items = np.array([(0, n, 0, 0, 0)], dtype=_lib.QMDCT_BATCH_ITEM_DTYPE)
    d_is, d_segs, d_items = ctx.to_device(np.ascontiguousarray(p["is"])), ctx.to_device(segs), ctx.to_device(items)
    d_out, d_batch = ctx.alloc(_lib.QMDCT_FEATURES_DTYPE.itemsize), ctx.alloc(n * 4608)
    calls = {"k_qmdct_features": lambda: _lib.lib().mp3s_qmdct_features_dev(ctx.handle, d_is, n, 2, d_segs, segs.ctypes.data, 1, 576, d_out),
             "k_qmdct_batch": lambda: _lib.lib().mp3s_qmdct_batch_dev(ctx.handle, d_is, 2, d_items, items.ctypes.data, 1, 2, 2 * n, d_batch)}
    out = {"frames": n, "bytes_read": n * 4608, "copy_gb_per_s": round(copy_gbs, 1),
           "workgroups_k_qmdct_features": 2 * ((2 * n + _lib.QMDCT_SLICE - 1) // _lib.QMDCT_SLICE), "slice": _lib.QMDCT_SLICE}
    for name, call in calls.items():
        t = []
        for k in range(repeats + 3):
            ctx.timer_start()
            _lib.check(call())
            ms = ctx.timer_stop()
            if k >= 3:
                t.append(ms)
        moved = n * 4608 * (2 if name == "k_qmdct_batch" else 1)
        floor_ms = moved / (copy_gbs * 1e9) * 1e3
        out[name] = {"timer_ms": summary(t), "floor_ms": round(floor_ms, 4), "over_floor": round(statistics.median(t) / floor_ms, 2)}
    for d in (d_is, d_segs, d_items, d_out, d_batch):
        ctx.free(d)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--host-repeats", type=int, default=2)
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
        feats = ctx.qmdct_features(files)
        frames = sum(f["n_frames"] for f in feats)
        granules = 2 * max(f["n_frames"] for f in feats)
        batch, batch_name = batch_call(ctx, files, granules)
        t = alternate_ms(ctx, [lambda: ctx.qmdct_features(files), lambda: ctx.table_audits(files), batch], args.repeats)
        out[name] = {"frames": frames, "zero_share": round(sum(int(f["hist"][:, 0].sum()) for f in feats) / (frames * 2304), 3),
                     "qmdct_features": t[0], "table_audits": t[1], batch_name: t[2], "host_parse_stream_and_model": host_alternative(_lib, files, args.host_repeats),
                     "features_over_audit_wall": round(t[0]["wall_ms"]["median"] / t[1]["wall_ms"]["median"], 3),
                     "down_bytes": {"qmdct_features": 2904 * len(files), "table_audits": 104 * len(files), batch_name: 0}}
    out["kernels alone, 10 000 frames"] = kernels_alone(ctx, _lib, loads["one file of 10 000 frames"][0], args.repeats, ctx.bench_copy())
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
