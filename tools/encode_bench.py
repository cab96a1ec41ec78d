#!/usr/bin/env python3
"""WAV -> MP3 three ways, measured in ONE process, alternating: (a) a loop of Context.encode_file (the one-file call), (b)
Context.encode_files (one device batch per group), (c) a Pipe of depth 3 fed with the same job for >= 2 s (ms per job in steady
state).  Two workloads: one 10 000-frame file at 44.1 kHz / 128 kbit/s, and 250 files of 40 frames.  Beside them the floor of (c)
: the larger of a plain Context.upload of the job's WAV bytes from ordinary memory and the encode side alone on resident PCM.
(a), (b) and the upload are taken from the same buffers in every repeat, from four sets in rotation and from fresh buffers per
repeat; (c) from the same set and from the four in rotation.  Host clock around work that ends in a synchronise (every call
returns finished results), device events for the resident half; every shape is warmed up first; profiler off.

    python tools/encode_bench.py [--out profiles/r07_encode_batch.json] [--repeats 5] [--pipe-seconds 2] [--only long|short]

--format u8|s16|s24|s32|f32 and --channels 1|2 write the same audio as WAV files of that sample format and channel count and turn the
context's "wav_import" option on (k_wav_import converts them on the device); --wav-import 1 turns it on for the canonical 16-bit stereo
files too (they keep k_wav_gather: the figure to hold against the option's off state).

--resample runs ONE other case instead: Context.encode_files on 250 files x 40 output frames of 16-bit stereo at 22 050 Hz with the
"wav_resample" option on (k_wav_import + k_wav_resample on the device), against the same call on the same audio resampled on the host
beforehand (tests/wav_resample_model.py with the library's tap table: the same rows, so the same MP3 bytes) to 44 100 Hz, option off;
medians of --repeats alternating runs, and k_wav_resample's own time from the profile counters in a run of its own.  --resample-rate R
takes files of R Hz instead (96000, 192000, 384000: the down-sampling ratios with their longer filters).
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


def wav_of(pcm, rate, fmt="s16", channels=2):
    """-> (the WAV file, the int16 stereo rows the encoder gets from it)"""
    from mp3stego import _lib
    if fmt == "s16" and channels == 2:
        return _lib.wav_header(pcm.shape[0], 2, rate) + np.ascontiguousarray(pcm, dtype="<i2").tobytes(), pcm
    import wav_import_files as W
    f = {"u8": W.U8, "s16": W.S16, "s24": W.S24, "s32": W.S32, "f32": W.F32}[fmt]
    p = (pcm if channels == 2 else pcm[:, 0]).astype(np.int64)
    s = {"u8": (p >> 8) + 128, "s16": p, "s24": p << 8, "s32": p << 16, "f32": (p / 32768.0).astype(np.float32)}[fmt]
    return W.wav_file(s, f, rate=rate), W.stereo_frames(s, f)


def pipe_ms_per_job(_lib, ctx, sets, kbps, seconds, want, frames):
    wavs, turn = sets[0], [0]

    def submit():
        turn[0] += 1
        return pipe.submit_encode(sets[turn[0] % len(sets)], kbps)

    # (slots for the job's MP3 bytes -- 418 per frame at 44.1 kHz / 128 kbit/s -- with a fifth to spare; their frame capacity, 1/96 of
    #  that, is what the slot's WAV image is made from)
    pipe = _lib.Pipe(ctx, depth=3, max_job_bytes=max(1 << 20, frames * 500), scan_threads=2, max_files=max(1024, len(wavs)))
    try:
        for _ in range(4):                                     # warm-up: every slot has seen the shape
            while submit() is not None:
                pass
            while pipe.collect() is not None:
                pass
        done, t0 = 0, time.perf_counter()
        inflight = 0
        while True:
            while submit() is not None:
                inflight += 1
            _, res = pipe.collect()
            inflight -= 1
            done += 1
            if time.perf_counter() - t0 >= seconds:
                break
        t1 = time.perf_counter()                               # (steady state: the jobs still in flight are not counted)
        assert all(bytes(r["data"]) == w for r, w in zip(res, want)), "the pipe's bytes differ from encode_file's"
        while pipe.collect() is not None:
            pass
        st = pipe.stats()
    finally:
        pipe.close()
    return (t1 - t0) * 1e3 / done, done, {k: st[k] for k in ("fast", "resolved", "slow", "collected")}


def encode_half_resident_ms(_lib, ctx, pcms, want, repeats):
    """floor (ii): the encode side of the job alone, on PCM that is already in HBM and with every host-made input resident --
    mp3s_encode_transform_dev, the rate loop, the chain check with the device's re-runs, mp3s_pack_frames_dev; what enc_issue
    queues for this job (the workloads hide nothing, so the job has no variant entries: the rate loop is mp3s_rate_loop_dev, the
    launch mp3s_rate_select_dev makes when there is no message).  Device events around the four calls; the bytes are compared."""
    L = _lib.lib()
    counts = [p.shape[0] // 1152 for p in pcms]
    n, units, ns = sum(counts), sum(counts) * 4, len(counts)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    hdr = np.zeros(n, dtype=_lib.FRAME_HDR_DTYPE)
    hdr["nch"] = 2
    rf = np.zeros(n, dtype=_lib.RATE_FRAME_DTYPE)
    pad = np.zeros(n, dtype=np.int32)
    seg = np.zeros(ns, dtype=_lib.CHAIN_SEG_DTYPE)
    for i, c in enumerate(counts):                                  # padding and slot lag restart with every stream
        a, b = int(first[i]), int(first[i + 1])
        rf[a:b], pad[a:b] = _lib.rate_frames(44100, 128, 2, c)
        rf["stream"][a:b] = i
        hdr["stream_first"][a:b] = a
        seg["first_frame"][i], seg["n_frames"][i] = a, c
    rf["hide_end"] = 32
    seg["hide_base"] = seg["hide_begin"] = seg["hide_end"] = 32     # behind the eight patterns: no message
    cur = np.minimum(32 + 3 * np.concatenate([np.arange(c * 4) for c in counts]), _lib.NO_CURSOR).astype(np.int32)
    slots = (128 * 1000 * 1152 // 8) // 44100
    off = np.concatenate([[0], np.cumsum(slots + pad)]).astype(np.uint32)
    d_pcm = ctx.to_device(np.concatenate(pcms).astype(np.int16))
    d_hdr, d_rf, d_seg, d_cur, d_hide = (ctx.to_device(a) for a in (hdr, rf, seg, cur, _lib.select_patterns()))
    d_off, d_pad = ctx.to_device(off), ctx.to_device(pad.astype(np.uint8))
    d_mdct, d_ix, d_out, d_en = ctx.alloc(n * 2304 * 4), ctx.alloc(n * 2304 * 2), ctx.alloc(units * 72), ctx.alloc(units * 88)
    d_mp3, d_sc, d_pst, d_ver, d_so = ctx.alloc(int(off[-1]) + 16), ctx.alloc(n * 8 * 4), ctx.alloc(16), ctx.alloc(16), ctx.alloc(ns * 80)

    def half():
        _lib.check(L.mp3s_encode_transform_dev(ctx.handle, d_pcm, d_hdr, n, d_mdct))
        _lib.check(L.mp3s_rate_loop_dev(ctx.handle, d_mdct, d_rf, n, d_hide, 32, d_cur, None, None, 0, d_ix, d_out, d_en))
        _lib.check(L.mp3s_chain_redo_dev(ctx.handle, d_mdct, d_rf, n, d_hide, 32, d_cur, d_seg, ns, d_ix, d_out, d_en, d_ver, d_so))
        _lib.check(L.mp3s_pack_frames_dev(ctx.handle, d_ix, d_out, d_en, n, 44100, 128, d_off, d_pad, d_mp3, d_sc, d_pst))

    half(); half(); ctx.sync()
    ms = []
    for _ in range(repeats):
        ctx.timer_start(); half(); ms.append(ctx.timer_stop())
    mp3 = ctx.download(d_mp3, np.uint8, (int(off[-1]),)).tobytes()
    ver = ctx.download(d_ver, np.int32, (2,))
    assert int(ver[0]) == 0 and int(ver[1]) == 0, ver
    for i, w in enumerate(want):
        assert mp3[int(off[first[i]]):int(off[first[i]]) + len(w)] == w, ("the resident encode half's bytes differ", i)
    for p in (d_pcm, d_hdr, d_rf, d_seg, d_cur, d_hide, d_off, d_pad, d_mdct, d_ix, d_out, d_en, d_mp3, d_sc, d_pst, d_ver, d_so):
        ctx.free(p)
    return ms


def resample_case(_lib, ctx, repeats, rate=22050):
    from synth_pcm import synth_pcm
    import wav_resample_model as R
    plan = R.plan(rate, 1)
    L, M, out_rate = plan["L"], plan["M"], plan["out_rate"]
    assert 40 * M % L == 0, "a rate whose 40 output frames are whole input frames"
    taps = _lib.wav_resample_taps(L, M)
    low = [synth_pcm(40 * M // L, seed=3000 + i) for i in range(250)]         # e.g. 20 frames at 22 050 Hz = 40 frames at 44 100 Hz
    wavs_low = [_lib.wav_header(p.shape[0], 2, rate) + np.ascontiguousarray(p, dtype="<i2").tobytes() for p in low]
    wavs_pre = [wav_of(R.frames_of(R.resample(p, L, M, taps)), out_rate)[0] for p in low]
    on = lambda: (ctx.set_option("wav_resample", 1), ctx.encode_files(wavs_low, 128))[1]
    off = lambda: (ctx.set_option("wav_resample", 0), ctx.encode_files(wavs_pre, 128))[1]
    assert [bytes(r["data"]) for r in on()] == [bytes(r["data"]) for r in off()], "the resampled batch's bytes differ from the pre-resampled one's"
    on(); off()
    on_ms, off_ms = [], []
    for _ in range(repeats):
        t0 = time.perf_counter(); on(); t1 = time.perf_counter(); off(); t2 = time.perf_counter()
        on_ms.append((t1 - t0) * 1e3); off_ms.append((t2 - t1) * 1e3)
    ctx.profile_select(["k_wav_resample"]); ctx.profile_enable(True)
    for _ in range(repeats):
        on()
    ms, launches = ctx.profile_collect()["k_wav_resample"]
    ctx.profile_enable(False); ctx.profile_select(None); ctx.set_option("wav_resample", 0)
    rows_in, rows_out = sum(p.shape[0] for p in low), 250 * 40 * 1152
    k_ms = ms / max(1, launches)
    return {"what": "250 files x 40 output frames, %d -> %d Hz (L / M = %d / %d, %d taps), 128 kbit/s, 16-bit stereo" % (rate, out_rate, L, M, plan["taps"]), "resample_on_ms": on_ms, "pre_resampled_off_ms": off_ms,
            "resample_on_median_ms": statistics.median(on_ms), "pre_resampled_off_median_ms": statistics.median(off_ms),
            "ratio": statistics.median(on_ms) / statistics.median(off_ms), "k_wav_resample_ms_per_launch": k_ms, "k_wav_resample_launches": launches,
            "k_wav_resample_bytes_read_written": 4 * (rows_in + rows_out), "k_wav_resample_gb_per_s": 4 * (rows_in + rows_out) / (k_ms * 1e-3) / 1e9 if k_ms else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pipe-seconds", type=float, default=2.0)
    ap.add_argument("--only", choices=["long", "short"], default=None)
    ap.add_argument("--no-pipe", action="store_true", help="(a) and (b) only: the kernel-trace run")
    ap.add_argument("--format", choices=["u8", "s16", "s24", "s32", "f32"], default="s16")
    ap.add_argument("--channels", type=int, choices=[1, 2], default=2)
    ap.add_argument("--wav-import", type=int, choices=[0, 1], default=None, help="the context's wav_import option (default: on for what only it reads)")
    ap.add_argument("--resample-rate", type=int, default=22050, help="the files' sampling rate in the --resample case (22050, 96000, 192000, 384000 ...)")
    ap.add_argument("--resample", action="store_true", help="only the wav_resample case: 250 files at 22 050 Hz against the same audio pre-resampled")
    args = ap.parse_args()
    from mp3stego import _lib
    from synth_pcm import synth_pcm
    ctx = _lib.Context(0)
    if args.resample:
        r = {"device": ctx.device_name(), "repeats": args.repeats, "clock": "host perf_counter around calls that return finished results", "resample": resample_case(_lib, ctx, args.repeats, args.resample_rate)}
        ctx.close()
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r["resample"].items() if not isinstance(v, list)}), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(r, indent=1, sort_keys=True) + "\n")
        return
    canonical = args.format == "s16" and args.channels == 2
    ctx.set_option("wav_import", (0 if canonical else 1) if args.wav_import is None else args.wav_import)
    result = {"device": ctx.device_name(), "repeats": args.repeats, "format": args.format, "channels": args.channels, "wav_import": ctx.get_option("wav_import"), "clock": "host perf_counter around calls that return finished results", "workloads": {}}
    loads = {"long": ("one 10 000-frame file, 44.1 kHz, 128 kbit/s", [synth_pcm(10000, seed=1234)]),
             "short": ("250 files of 40 frames, 44.1 kHz, 128 kbit/s", [synth_pcm(40, seed=2000 + i) for i in range(250)])}
    for name, (what, pcms) in loads.items():
        if args.only and name != args.only:
            continue
        made = [wav_of(p, 44100, args.format, args.channels) for p in pcms]
        wavs, pcms = [m[0] for m in made], [m[1] for m in made]         # (pcms: what the encoder sees, for the resident floor)
        n_bytes = sum(len(w) for w in wavs)
        frames = sum(p.shape[0] // 1152 for p in pcms)
        one_by_one = lambda: [ctx.encode_file(w, 128) for w in wavs]
        batch = lambda: ctx.encode_files(wavs, 128)
        want = [bytes(r["data"]) for r in one_by_one()]                      # warm-up of (a) ...
        assert [bytes(r["data"]) for r in batch()] == want                   # ... and of (b), and the bytes agree
        one_by_one(); batch()
        # Where the bytes come from matters to the runtime (a copy from ordinary memory pins the pages it reads), so every figure is
        # taken three times: from the SAME buffers in every repeat, from four distinct sets of buffers in ROTATION, and from FRESH
        # buffers per repeat (copied outside the clock, never uploaded from before, dropped afterwards) -- what a caller who encodes a
        # series of different files hands over.  `other_upload`: the same buffers, with a plain upload of ANOTHER 46 MB buffer between
        # the repeats (the order in which this tool first ran: docs/LOG.md).
        copy = lambda: [bytes(bytearray(w)) for w in wavs]
        rot = [copy() for _ in range(4)]
        d = ctx.alloc(n_bytes)
        other = np.frombuffer(b"".join(wavs), dtype=np.uint8)
        r = {"what": what, "frames": frames, "wav_bytes": n_bytes, "inputs": {}}
        for mode in ("same", "rotating", "fresh", "other_upload"):
            a_ms, b_ms, up_ms = [], [], []
            for k in range(args.repeats):
                ws = wavs if mode in ("same", "other_upload") else rot[k % 4] if mode == "rotating" else copy()
                t0 = time.perf_counter(); [ctx.encode_file(w, 128) for w in ws]; t1 = time.perf_counter(); ctx.encode_files(ws, 128); t2 = time.perf_counter()
                a_ms.append((t1 - t0) * 1e3); b_ms.append((t2 - t1) * 1e3)
                if mode == "other_upload":
                    ctx.upload(d, other)
                # the floor's first part: the job's WAV bytes going up from ordinary memory, as the images travel (a set of buffers of its own:
                # the encodes above have not touched it, except in `same`)
                us = wavs if mode in ("same", "other_upload") else rot[(k + 2) % 4] if mode == "rotating" else copy()
                blob = np.frombuffer(us[0] if len(us) == 1 else b"".join(us), dtype=np.uint8)   # (short files end to end, outside the clock)
                t2 = time.perf_counter()
                ctx.upload(d, blob)
                up_ms.append((time.perf_counter() - t2) * 1e3)
                del ws, us, blob
            r["inputs"][mode] = {"a_encode_file_loop_ms": a_ms, "b_encode_files_ms": b_ms, "floor_upload_ms": up_ms,
                                 "a_median_ms": statistics.median(a_ms), "a_spread_ms": max(a_ms) - min(a_ms), "b_median_ms": statistics.median(b_ms),
                                 "floor_upload_median_ms": statistics.median(up_ms)}
        ctx.free(d)
        half = encode_half_resident_ms(_lib, ctx, pcms, want, args.repeats)
        r["floor_encode_half_resident_ms"] = half
        r["floor_encode_half_resident_median_ms"] = statistics.median(half)
        if not args.no_pipe:
            for mode, sets in (("same", [wavs]), ("rotating", rot)):
                ms, jobs, st = pipe_ms_per_job(_lib, ctx, sets, 128, args.pipe_seconds, want, frames)
                r["inputs"][mode].update({"c_pipe_ms_per_job": ms, "c_pipe_jobs_timed": jobs, "c_pipe_stats_with_warm_up": st})
            r["floor_ms"] = max(r["inputs"]["rotating"]["floor_upload_median_ms"], r["floor_encode_half_resident_median_ms"])
        result["workloads"][name] = r
        print(json.dumps({name: {"half_ms": round(r["floor_encode_half_resident_median_ms"], 3),
                                 **{m: {k: round(v, 3) for k, v in x.items() if "median" in k or k == "c_pipe_ms_per_job" or k == "a_spread_ms"} for m, x in r["inputs"].items()}}}), flush=True)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
