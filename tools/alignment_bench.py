"""A cover file against its stego file, for a list of pairs: what docs/LOG.md records about Context.pcm_alignments.  Prints one JSON line.

  python tools/alignment_bench.py [--repeats N] [--once] [--rates]

Context.pcm_alignments(stego, cover) against the way to the same numbers without it -- Context.decode_streams of both lists and a numpy
loop over the lags (int64) --, in one process, alternating, median of N calls after warm-up: 250 pairs of 40 frames, and one pair of
10 000 frames, 44.1 kHz / 128 kbit/s, the hide re-encode of a message against the file it was hidden in, at the default max_lag and
search_rows.  The two ways are compared field by field, every score included, before anything is timed.
--once stops behind that comparison (one pcm_alignments call per workload): the run to put under `rocprofv3 --kernel-trace --stats` for
the three kernels' own times.
--rates adds the lag found for tests/golden/test.mp3 and for one file of every sampling rate (the re-encode's delay in rows).
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
MAX_LAG, SEARCH_ROWS = 2304, 4608
FIELDS = ("lag", "n_best", "err2_best", "err2_at_0", "search_first", "search_rows", "err2", "sig2", "max_abs", "n_diff", "first_diff", "n_samples")


def alternate_ms(fs, repeats):
    """median / min / max of each of the calls fs, taken in turn after one warm-up call each (the numpy way takes a minute for 250 pairs)"""
    for f in fs:
        f()
    t = [[] for _ in fs]
    for _ in range(repeats):
        for k, f in enumerate(fs):
            t0 = time.perf_counter()
            f()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return [{"median": round(statistics.median(x), 3), "min": round(min(x), 3), "max": round(max(x), 3)} for x in t]


def numpy_way(ctx, a, b, scores_out=None):
    """decode both lists, every sample to the host, the lag loop and the sums at the lag in int64"""
    out = []
    M = MAX_LAG
    for x, y in zip(ctx.decode_streams(a), ctx.decode_streams(b)):
        p, q = x["pcm"].astype(np.int64), y["pcm"].astype(np.int64)
        p, q = p.reshape(len(p), -1), q.reshape(len(q), -1)
        W = min(len(p), len(q)) - 2 * M
        S = min(W, SEARCH_ROWS)
        s0 = M + (W - S) // 2
        qw = q[s0:s0 + S]
        sc = np.empty(2 * M + 1, dtype=np.int64)
        for L in range(-M, M + 1):
            d = p[s0 + L:s0 + L + S] - qw
            sc[L + M] = (d * d).sum()
        best = int(sc.min())
        lag = min((int(i) - M for i in np.nonzero(sc == best)[0]), key=lambda v: (abs(v), v < 0))
        i0, i1 = max(0, -lag), min(len(q), len(p) - lag)
        u, v = p[i0 + lag:i1 + lag].reshape(-1), q[i0:i1].reshape(-1)
        d = u - v
        ne = np.nonzero(d)[0]
        out.append({"lag": lag, "n_best": int((sc == best).sum()), "err2_best": best, "err2_at_0": int(sc[M]), "search_first": s0, "search_rows": S,
                    "err2": int((d * d).sum()), "sig2": int((u * u).sum()), "max_abs": int(np.abs(d).max()) if len(d) else 0, "n_diff": len(ne),
                    "first_diff": int(ne[0]) if len(ne) else -1, "n_samples": len(d)})
        if scores_out is not None:
            scores_out.append(sc)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--rates", action="store_true")
    args = ap.parse_args()
    from mp3stego import _lib
    from synth_pcm import synth_pcm
    ctx = _lib.Context(0)
    rng = np.random.default_rng(3)
    out = {"device": ctx.device_name(), "repeats": args.repeats, "max_lag": MAX_LAG, "search_rows": SEARCH_ROWS, "time": {}}
    if args.rates:
        files = {"tests/golden/test.mp3 (44100 Hz, 320 kbit/s)": open(os.path.join(ROOT, "tests", "golden", "test.mp3"), "rb").read()}
        for rate, kbps in ((32000, 64), (44100, 128), (48000, 192)):
            files[f"synth {rate} Hz, {kbps} kbit/s, 40 frames"] = bytes(ctx.encode_pcm(synth_pcm(40, rate=rate, seed=4000 + rate), rate, kbps, None)["mp3"])
        names, covers = list(files), list(files.values())
        res = ctx.stego_distortions(covers, ["a short message"] * len(covers))
        want = numpy_way(ctx, [bytes(h["data"]) for h in ctx.hide_messages(covers, ["a short message"] * len(covers))], covers)
        out["lags"] = {n: {"lag": r["lag"], "n_best": r["n_best"], "err2_best": r["err2_best"], "err2_at_0": r["err2_at_0"], "snr_db": round(r["snr_db"], 2),
                           "numpy_lag": w["lag"]} for n, r, w in zip(names, res, want)}
    loads = {}
    wavs = [_lib.wav_header(40 * 1152, 2, 44100) + synth_pcm(40, seed=2000 + i).astype("<i2").tobytes() for i in range(250)]
    loads["250 pairs of 40 frames"] = [bytes(e["data"]) for e in ctx.encode_files(wavs, 128)]
    loads["one pair of 10 000 frames"] = [bytes(ctx.encode_pcm(synth_pcm(10000, seed=7), 44100, 128, None)["mp3"])]
    for name, files in loads.items():
        msgs = ["".join(chr(int(c)) for c in rng.integers(32, 127, size=24)) for _ in files]
        stego = [bytes(h["data"]) for h in ctx.hide_messages(files, msgs)]
        scores = []
        got, want = ctx.pcm_alignments(stego, files, profile=True), numpy_way(ctx, stego, files, scores)
        for g, w, sc in zip(got, want, scores):
            assert all(int(g[k]) == w[k] for k in FIELDS), ({k: g[k] for k in FIELDS}, w)
            assert np.array_equal(g["scores"].astype(np.int64), sc)
        if args.once:
            continue
        del got
        t = alternate_ms([lambda: ctx.pcm_alignments(stego, files), lambda: numpy_way(ctx, stego, files),
                          lambda: ctx.pcm_alignments(stego, files, profile=True), lambda: ctx.decode_streams(stego + files),
                          lambda: ctx.pcm_alignments(stego, files, lags=[w["lag"] for w in want])], args.repeats)
        lags = sorted(set(w["lag"] for w in want))
        out["time"][name] = {"pairs": len(files), "lags_found": lags[:8], "ambiguous_pairs": sum(1 for w in want if w["n_best"] != 1),
                             "pcm_alignments_ms": t[0], "decode_streams_and_numpy_ms": t[1], "pcm_alignments_with_profile_ms": t[2],
                             "decode_streams_of_both_lists_alone_ms": t[3], "pcm_alignments_given_lags_ms": t[4],
                             "pcm_alignments_over_numpy_way": round(t[0]["median"] / t[1]["median"], 5)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
