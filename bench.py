#!/usr/bin/env python3
"""Benchmark of the hot path: MP3 frames/s for decode + re-encode at 44.1 kHz stereo 128 kbps.

    python bench.py --gpus N --steps K --warmup W
    (N > 1: either under python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ..., or on its own:
     with WORLD_SIZE unset bench.py starts its N ranks itself as child processes, tools/launch_ranks.py)

Three timed regions, all on the same 10 000-frame stream and the same 67-byte message:

  (i)   `value`: one step = one batch through the whole DEVICE pipeline, inputs resident in HBM (MP3 main data + parsed
        side info, what the host scan uploads): Huffman decode -> decode transforms -> int16 PCM -> encode transforms ->
        rate loop with the message's variants in the same launch -> cursor chain decided on the device (mp3s_rate_select_dev)
        -> chain check on the device, with the re-runs it asks for and the check behind them (mp3s_chain_redo_dev, as the
        library's own encoder issues it: nothing about the serial chains is precomputed outside the timed region, nothing is
        guessed) -> bit packing.  K steps, wall clock between barriers.
  (ii)  `regions.h2d_kernels_d2h`: the same batch from page-locked host staging: upload + kernels + download, one batch at
        a time (pipe of depth 1; HIP events from the first uploaded byte to the last downloaded one), averaged.
  (iii) `e2e_steady`: MP3 bytes -> MP3 bytes through the asynchronous host-fed pipeline (mp3s_pipe_*: host scan on worker
        threads || upload || kernels || download, several batches in flight), >= 200 batches, steady state.  This is
        what a caller of the library gets.  `regions.bytes_to_bytes_one_at_a_time` is the synchronous call in a loop.

`single_file_10k` / `single_file_100k` are ONE file per call -- the reference's call shape (steganography.py:137-162) --
through `Context.hide_message` (one native call: the file as chunks through the overlapped stages) and through the drop-in
`Steganography.hide_message(quiet=True)`.  `config5` is BASELINE configs[4]: streams with short / switching / mixed blocks, MS,
mono, bit reservoir at 32 / 44.1 / 48 kHz (decode, frames/s) and re-encodes at 32 ... 320 kbps.

`decode_only` is BASELINE config 2 (Huffman + decode transforms to float32 PCM, resident).  Multi-GPU: every rank owns
its own batches (weak scaling, no collective on the data path) and runs regions (i) and (iii); torch is used only for the
rendezvous / barrier / max-over-ranks (gloo).

A plain run measures the headline alone: it builds the resident batch, warms up on untimed steps (--warmup steps, 3-10 more
as --full's per-kernel pass, then max(--warmup, PLAIN_SETTLE_STEPS); no event pairs), times EXACTLY --steps steps of region (i)
as one region and prints a short line (`value`, `ms_per_step` = wall clock of the region / --steps, max over ranks).  Everything else above -- the per-kernel table, the roofline and its rocprofv3 passes, the three
regions behind `value_min` / `value_max`, the parity checks against the library and the oracle, the four-stream step,
`decode_only`, the host-fed regions, config5 and the CPU baseline -- runs with --full, as it did before that option existed.
--dump-outputs DIR (either mode) writes what the last timed step computed: its MP3 bytes, its message offset and a fixed
sample of its int16 PCM (dump_outputs below).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(ROOT, "mp3-steganography-lib_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _baseline_metric():
    """the metric string exactly as BASELINE.json has it (the file travels with the repo)"""
    try:
        with open(os.path.join(ROOT, "BASELINE.json")) as f:
            return json.load(f)["metric"]
    except Exception:
        return "MP3 frames/sec (decode+re-encode) @44.1kHz stereo 128kbps, 1→8 GPU"


METRIC = _baseline_metric()
B_PIPE = 14208        # algorithmic bytes per stereo frame of the full pipeline (SURVEY.md section 8d / BASELINE.md 4)
B_DEC = 14128         # decode-only
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak (MI355X_MICROARCH.md)
N_SIMD, CLOCK_GHZ, CLK_PER_VALU = 1024, 2.4, 4.0   # 256 CUs x 4 SIMDs; fp64 / 32-bit multiply class: >= 4 clk per wave instruction (tools/ubench/valu_rates.hip: 4.5)
MESSAGE = "64#" + "The quick brown fox jumps over the lazy dog, again & again, 0123"


def same_bytes(view, ref):
    """compare a result (a view of the library's page-locked block) with reference bytes without copying it"""
    a, b = np.frombuffer(view, dtype=np.uint8), np.frombuffer(ref, dtype=np.uint8)
    return a.size == b.size and bool(np.array_equal(a, b))


def bits_of(s):
    return np.frombuffer("".join(format(b, "08b") for b in s.encode()).encode(), dtype=np.uint8) - ord("0")


PLAIN_SETTLE_STEPS = 40         # a plain run: untimed steps directly in front of its one region, at least (main: the second warm-up)
DUMP_MAX_MP3_BYTES = 8 << 20     # --dump-outputs: MP3 bytes kept whole up to this many (32 MiB as float32), a sample beyond
DUMP_PCM_SAMPLES = 1 << 20       # ... and this many int16 PCM samples of the step's decode half, at fixed positions
DUMP_SEED = 0x5EED


def dump_outputs(out_dir, mp3, hide_offset, pcm):
    """--dump-outputs: the last timed step's results as DIR/<name>.npy (float32 / float64, at most 36 MiB in all): `mp3_bytes` = the MP3
    stream out (the `data` a caller of Context.hide_message receives), `hide_offset` = where the message ended up (its `hide_offset`),
    `pcm_int16_sample` = int16 PCM of the step's decode half (interleaved) at DUMP_PCM_SAMPLES positions drawn with DUMP_SEED, in
    ascending order: the same positions in every run of the same arguments.  A stream longer than DUMP_MAX_MP3_BYTES is sampled the same way."""
    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.default_rng(DUMP_SEED)

    def sample(a, k):
        return a if a.size <= k else a[np.sort(rng.choice(a.size, size=k, replace=False))]
    arrays = {"mp3_bytes": sample(mp3.reshape(-1), DUMP_MAX_MP3_BYTES).astype(np.float32),
              "hide_offset": np.array([hide_offset], dtype=np.float64),
              "pcm_int16_sample": sample(pcm.reshape(-1), DUMP_PCM_SAMPLES).astype(np.float32)}
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def rank_host_record(rank, scan_threads, e2e_steady, host_share):
    """what one rank reports of the host it shares (the line's `ranks_on_this_host`): its CPUs, its walk / issue time per batch, its share of
    the page-locked pool (mp3s_ctx_host_share).  `host_share`: a callable returning that dict (the context's, or the library's without a context)"""
    host = {"rank": rank, "cpus_allowed": len(os.sched_getaffinity(0)), "scan_threads": scan_threads,
            "host_walk_ms_per_batch": e2e_steady["host_scan_ms_per_batch"] if e2e_steady else None,
            "host_issue_ms_per_batch": e2e_steady["host_issue_ms_per_batch"] if e2e_steady else None,
            "pcie_gb_s": round((e2e_steady["bytes_in_per_batch"] + e2e_steady["bytes_out_per_batch"]) / (e2e_steady["ms_per_batch"] * 1e-3) / 1e9, 2) if e2e_steady else None}
    try:
        host.update(host_share())            # page-locked bytes pooled / cap, the ranks it believes share the host, CPUs on the GPU's NUMA node
    except Exception:                         # noqa: BLE001
        pass
    return host


def gather_rank_hosts(dist, world, host):
    """every rank's record on every rank, in rank order (rank 0 prints them); one process: just its own"""
    if dist is None:
        return [host]
    hosts = [None] * world
    dist.all_gather_object(hosts, host)
    return hosts


def run_config5(ctx, _lib, O, synth_pcm, n):
    """BASELINE configs[4]: mixed bitrate / sampling-rate corpus with long / short block switching, mono and joint stereo.
    Decode side: streams from tests/frame_synth.py (250 synthesised frames, laid end to end up to `n`: every copy starts with
    main_data_begin = 0 and the reservoir only looks back) -> frames/s of Context.decode_stream to int16 (fast kernels behind
    the guard) and to float32 (exact kernels), a prefix compared with the oracle.  Encode side: this encoder's own streams
    at (sampling rate, bitrate) pairs -> frames/s of Context.hide_message, compared with the stages one after the other and,
    on a prefix, with the oracle.  Reference: decoder/Frame.py:120-125, 186-208, 574-602."""
    import frame_synth
    ok = True
    reps = max(1, n // 250)
    nf = 250 * reps
    mixes = [("long_blocks_44k_128", dict(seed=101, block_types=(0,), use_reservoir=True)),
             ("all_short_44k_128", dict(seed=102, block_types=(2,), use_reservoir=True)),
             ("long_blocks_no_reservoir_44k_128", dict(seed=109, block_types=(0,), use_reservoir=False)),   # (granules cut short by the frame's end: the reference decodes on into the next granule's bits)
             ("switching_reservoir_44k_128", dict(seed=103, block_types=(0, 1, 2, 3), use_reservoir=True)),
             ("mixed_blocks_44k_128", dict(seed=104, block_types=(0, 2), allow_mixed=True, use_reservoir=True)),
             ("joint_ms_short_48k_192", dict(seed=105, sr_idx=1, bitrate_idx=11, mode=1, mode_ext=2, block_types=(0, 2), use_reservoir=True)),
             ("mono_crc_32k_64", dict(seed=106, sr_idx=2, bitrate_idx=5, mode=3, crc=True, block_types=(0, 1, 2, 3), use_reservoir=True)),
             ("long_reservoir_44k_320", dict(seed=107, bitrate_idx=14, block_types=(0,), use_reservoir=True)),
             ("low_rate_32k_32", dict(seed=108, sr_idx=2, bitrate_idx=1, block_types=(0, 2), use_reservoir=True))]
    dec = {}
    for name, kw in mixes:
        seed = kw.pop("seed")
        one = frame_synth.make_stream(seed, 250, **kw)
        data = one * reps
        row = {"frames": nf, "bytes": len(data)}
        od = O.decode(one)                                                   # the oracle on the 250 synthesised frames
        rs0 = ctx.run_stats()
        exact_i16 = 0
        for fmt, key in ((_lib.MP3S_PCM_I16, "int16_fast"), (_lib.MP3S_PCM_F32, "float32_exact")):
            ctx.synth_mode(1.0)                                                # (reads and clears the counter of guarded samples)
            if os.environ.get("MP3S_TRACE"):
                sys.stderr.write("==== config5 %s %s\n" % (name, key)); sys.stderr.flush()
            r = ctx.decode_stream(data, fmt)
            ok = ok and r["n_frames"] == nf
            head = r["pcm"][:250 * 1152]
            want = O.pcm_to_i16(od["pcm"]) if fmt == _lib.MP3S_PCM_I16 else od["pcm"].astype(np.float32)
            ok = ok and bool(np.array_equal(head, want)) and bool(np.array_equal(r["bits"][:len(od["bits"])], od["bits"]))
            del r
            ts = []
            for _ in range(7):
                t0 = time.perf_counter()
                r = ctx.decode_stream(data, fmt); del r
                ts.append(time.perf_counter() - t0)
            dt = sorted(ts)[len(ts) // 2]                                      # median of 7 calls (the first calls of a size find no page-locked block in the pool)
            row[key] = {"ms": round(dt * 1e3, 3), "frames_per_s": round(nf / dt), "calls_ms": [round(t * 1e3, 3) for t in ts]}
            if fmt == _lib.MP3S_PCM_I16:
                exact_i16 = ctx.synth_mode(1.0)
        rs1 = ctx.run_stats()
        row["calls_through_the_overlapped_stages"] = rs1["files"] - rs0["files"]     # of 16; the others needed the host parser (scalefactors inherited
        row["calls_through_the_stages_one_after_the_other"] = rs1["fallbacks"] - rs0["fallbacks"]   # across frames, Huffman data that runs into the next granule)
        row["int16_samples_recomputed_in_exact_order_per_call"] = exact_i16 // 8
        row["lanes"], row["queue_shared"] = rs1["lanes"], rs1["queue_shared"]
        try:
            row["pinned_pooled_mb"] = round(ctx.host_share()["pinned_pooled_bytes"] / 2 ** 20, 1)
        except Exception:                                                      # noqa: BLE001
            pass
        if name == "all_short_44k_128":
            # per kernel, the stages one after the other (event pairs around every launch)
            ctx.set_option("file_pipeline", 0)
            ctx.profile_select(None); ctx.profile_enable(True)
            for _ in range(3):
                r = ctx.decode_stream(data, _lib.MP3S_PCM_I16); del r
            pr = ctx.profile_collect()
            ctx.profile_enable(False)
            row["kernels_ms_int16"] = {kn: round(ms / 3, 4) for kn, (ms, cnt) in pr.items() if cnt}
            ctx.profile_enable(True)
            for _ in range(3):
                r = ctx.decode_stream(data, _lib.MP3S_PCM_F32); del r
            pr = ctx.profile_collect()
            ctx.profile_enable(False)
            row["kernels_ms_float32"] = {kn: round(ms / 3, 4) for kn, (ms, cnt) in pr.items() if cnt}
            ctx.set_option("file_pipeline", 1)
        dec[name] = row
    enc = {}
    msg = "The quick brown fox jumps over the lazy dog, again & again, 0123"
    pcm = synth_pcm(min(n, 2500), seed=0x5EED)
    for rate, kbps in ((44100, 64), (44100, 320), (48000, 192), (32000, 128), (32000, 32), (48000, 320)):
        src = bytes(ctx.encode_pcm(pcm, rate, kbps, None)["mp3"])
        fsz = _lib.parse_stream(src)["frame_size"].astype(np.int64)
        m = len(fsz) - 1
        if m < 64:          # (32 kHz at 48 / 96 kbit/s: the reference's encoder sets a padding bit its own decoder does not expect, the stream ends after a frame)
            enc["%d_Hz_%d_kbps" % (rate, kbps)] = {"frames": int(m + 1), "skipped": "the reference's decoder stops after the first frame of this encoder's stream"}
            continue
        whole = src[:int(fsz[:m].sum())]
        r4 = max(1, n // m)
        data = whole * r4
        nfr = m * r4
        got = ctx.hide_message(data, msg)
        ctx.set_option("file_pipeline", 0)
        want = ctx.hide_message(data, msg)
        ctx.set_option("file_pipeline", 1)
        ok = ok and same_bytes(got["data"], bytes(want["data"])) and got["hide_offset"] == want["hide_offset"]
        # the oracle on a prefix of 64 frames
        k = 64
        o_dec = O.decode(data[:int(fsz[:k + 1].sum())])
        o_enc = O.encode(O.pcm_to_i16(o_dec["pcm"])[:k * 1152], rate, kbps, bits_of("%d#%s" % (len(msg), msg)))
        ok = ok and bytes(got["data"])[:len(o_enc["mp3"]) - 8] == o_enc["mp3"][:len(o_enc["mp3"]) - 8]
        del got, want
        kk = 8
        t0 = time.perf_counter()
        for _ in range(kk):
            r = ctx.hide_message(data, msg); del r
        dt = (time.perf_counter() - t0) / kk
        enc["%d_Hz_%d_kbps" % (rate, kbps)] = {"frames": nfr, "bytes": len(data), "ms": round(dt * 1e3, 3), "frames_per_s": round(nfr / dt)}
    # ---- band-limited real music: the PCM of the reference's own fixture (tests/test.mp3: 36 frames, 44.1 kHz stereo, the upper
    #      third of its spectrum empty), laid end to end and encoded here at 320 kbit/s -> decode and re-encode of that stream
    music = None
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "test.mp3")
    if os.path.exists(gold):
        og = O.decode(open(gold, "rb").read())
        pcm36 = O.pcm_to_i16(og["pcm"])
        r36 = max(1, n // 36)
        src = bytes(ctx.encode_pcm(np.ascontiguousarray(np.tile(pcm36, (r36, 1))), 44100, 320, None)["mp3"])
        nfm = 36 * r36
        p = _lib.parse_stream(src[:int(_lib.parse_stream(src)["frame_size"][:72].sum())])
        nz = p["is"] != 0
        last = np.where(nz.any(axis=-1), 576 - np.argmax(nz[..., ::-1], axis=-1), 0)
        music = {"frames": nfm, "bytes": len(src), "mean_lines_in_use_of_576": round(float(last.mean()), 1)}
        od = O.decode(src[:int(_lib.parse_stream(src)["frame_size"][:65].sum())])
        for fmt, key in ((_lib.MP3S_PCM_I16, "decode_int16_fast"), (_lib.MP3S_PCM_F32, "decode_float32_exact")):
            r = ctx.decode_stream(src, fmt)
            want = O.pcm_to_i16(od["pcm"]) if fmt == _lib.MP3S_PCM_I16 else od["pcm"].astype(np.float32)
            ok = ok and bool(np.array_equal(r["pcm"][:64 * 1152], want[:64 * 1152]))
            del r
            ts = []
            for _ in range(7):
                t0 = time.perf_counter()
                r = ctx.decode_stream(src, fmt); del r
                ts.append(time.perf_counter() - t0)
            dt = sorted(ts)[len(ts) // 2]
            music[key] = {"ms": round(dt * 1e3, 3), "frames_per_s": round(nfm / dt)}
        got = ctx.hide_message(src, msg)
        o_enc = O.encode(O.pcm_to_i16(od["pcm"])[:64 * 1152], 44100, 320, bits_of("%d#%s" % (len(msg), msg)))
        ok = ok and bytes(got["data"])[:len(o_enc["mp3"]) - 8] == o_enc["mp3"][:len(o_enc["mp3"]) - 8]
        del got
        ts = []
        for _ in range(7):
            t0 = time.perf_counter()
            r = ctx.hide_message(src, msg); del r
            ts.append(time.perf_counter() - t0)
        dt = sorted(ts)[len(ts) // 2]
        music["hide_message"] = {"ms": round(dt * 1e3, 3), "frames_per_s": round(nfm / dt)}
    slow = min(dec, key=lambda kname: dec[kname]["int16_fast"]["frames_per_s"])
    return {"what": "BASELINE configs[4]: decode of synthesised streams (250 frames laid end to end) and re-encode (hide_message) of this encoder's streams, "
                    "one file per call through the overlapped stages; every result compared with the oracle on a prefix",
            "decode": dec, "reencode": enc, "band_limited_music_44k_320": music, "slowest_decode_mix": slow}, ok


def live_pmc(frames, timeout_s=200):
    """HBM bytes and VALU wave instructions per launch of every kernel of the resident step, measured NOW: separate rocprofv3 --pmc
    passes (FETCH_SIZE / WRITE_SIZE / SQ_INSTS_VALU + SQ_INSTS_SALU + SQ_WAVES; never combined with --stats or other traces) over a
    short --resident-only run of this script as a CHILD process -- this process has not touched the GPU yet when it is called and
    never execs.  Bytes as MI355X_MICROARCH.md (HBM section) prescribes for gfx950: 2 x FETCH_SIZE + WRITE_SIZE, both converted
    from the counters' KB.  -> {kernel: {"hbm_bytes": ..., "SQ_INSTS_VALU": ...}} or None (no rocprofv3, a pass failed or timed out)."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None, "rocprofv3 not found"
    td = tempfile.mkdtemp(prefix="mp3s_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    res, t_begin = {}, time.time()
    try:
        for name, counters in (("fetch", ["FETCH_SIZE"]), ("write", ["WRITE_SIZE"]), ("sq", ["SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_WAVES"]),
                               # the vector instructions EXECUTED, by the hardware's own classes (data type, not encoding): roofline_alu.valu_by_type
                               ("sqt", ["SQ_INSTS_VALU_INT32", "SQ_INSTS_VALU_INT64", "SQ_INSTS_VALU_CVT", "SQ_INSTS_VALU_ADD_F64", "SQ_INSTS_VALU_MUL_F64",
                                        "SQ_INSTS_VALU_FMA_F64", "SQ_INSTS_VALU_TRANS_F64"])):
            left = timeout_s - (time.time() - t_begin)
            if left < 10:
                return None, "time budget spent"
            out = os.path.join(td, name)
            cmd = [prof, "--kernel-trace", "--pmc"] + counters + ["--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__),
                   "--full", "--resident-only", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-live-pmc", "--frames", str(frames)]
            r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=left)
            if r.returncode != 0:
                if name == "sqt":                  # (an extra: the by-type counters are not what the roofline needs)
                    break
                return None, f"pass {name}: exit {r.returncode}: {(r.stderr or r.stdout)[-200:]}"
            vals = {}
            for f in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(f)):
                    k = row["Kernel_Name"].split("(")[0].replace("void ", "").replace("mp3s::", "").split("<")[0]
                    vals.setdefault((k, row["Counter_Name"]), []).append(float(row["Counter_Value"]))
            if not vals:
                return None, f"pass {name}: no counters in the output"
            for (k, c), v in vals.items():
                res.setdefault(k, {})[c] = sum(v) / len(v)
    except Exception as e:                                   # noqa: BLE001
        return None, f"{type(e).__name__}: {e}"[:200]
    finally:
        shutil.rmtree(td, ignore_errors=True)
    for k, c in res.items():
        if "FETCH_SIZE" in c and "WRITE_SIZE" in c:
            c["hbm_bytes"] = c["FETCH_SIZE"] * 2048 + c["WRITE_SIZE"] * 1024
    return res, f"live: rocprofv3 --pmc passes (FETCH_SIZE | WRITE_SIZE | SQ instruction counts | SQ vector instructions by type) of bench.py --resident-only --steps 3 ({time.time() - t_begin:.0f} s)"


class GpuMonitor:
    """clocks / power / busy of one device read from sysfs by a side thread that makes no GPU call (the `sustained` region):
    /sys/bus/pci/devices/<address>/pp_dpm_sclk, pp_dpm_mclk (the line with the star), gpu_busy_percent, hwmon/*/power1_average"""

    def __init__(self, pci, period=0.2):
        import threading
        self.base = "/sys/bus/pci/devices/" + pci
        self.period, self.rows, self._stop = period, [], threading.Event()
        self._th = threading.Thread(target=self._run, daemon=True)

    @staticmethod
    def _star(path):
        try:
            for line in open(path):
                if "*" in line:
                    return int("".join(ch for ch in line.split(":")[1] if ch.isdigit()))
        except Exception:
            return None
        return None

    @staticmethod
    def _num(path):
        try:
            return int(open(path).read().split()[0])
        except Exception:
            return None

    def _power(self):
        import glob
        for f in glob.glob(self.base + "/hwmon/hwmon*/power1_average") + glob.glob(self.base + "/hwmon/hwmon*/power1_input"):
            v = self._num(f)
            if v is not None:
                return round(v / 1e6, 1)
        return None

    def _run(self):
        while not self._stop.is_set():
            self.rows.append((time.perf_counter(), self._star(self.base + "/pp_dpm_sclk"), self._star(self.base + "/pp_dpm_mclk"),
                              self._num(self.base + "/gpu_busy_percent"), self._power()))
            self._stop.wait(self.period)

    def start(self):
        self._th.start()
        return self

    def stop(self):
        self._stop.set()
        self._th.join(2)

    def summary(self, t0, t1):
        rows = [r for r in self.rows if t0 <= r[0] <= t1]

        def col(i, rows):
            v = [r[i] for r in rows if r[i] is not None]
            return None if not v else {"min": min(v), "max": max(v), "mean": round(sum(v) / len(v), 1)}
        first = [r for r in rows if r[0] <= t0 + 1.0]
        last = [r for r in rows if r[0] >= t1 - 1.0]
        return {"samples": len(rows), "readable": os.path.isdir(self.base),
                "sclk_mhz": col(1, rows), "mclk_mhz": col(2, rows), "gpu_busy_percent": col(3, rows), "power_w": col(4, rows),
                "sclk_mhz_first_second": col(1, first), "sclk_mhz_last_second": col(1, last)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=10000, help="frames per GPU per step / per batch")
    ap.add_argument("--full", action="store_true", help="besides the headline, everything else this script measures and checks (see the top of the file); "
                    "the options below from --e2e-batches to --no-live-pmc, except those that change the step itself (--no-overlap, --huffman-under, "
                    "--lean-sync, --no-tail-stream, --decode-stream), only act with it")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed to DIR/<name>.npy (dump_outputs; rank 0's batch)")
    ap.add_argument("--regions", type=int, default=None, help="timed regions of --steps steps each; `value` is the median one (value_min / value_max beside it); "
                    "default 3 with --full, else 1")
    ap.add_argument("--e2e-batches", type=int, default=400, help="batches of the host-fed steady-state region (0 = skip)")
    ap.add_argument("--sustained-seconds", type=float, default=5.0, help="wall time of the `sustained` region: the host-fed steady state for that long, "
                    "frames/s of its first and last second, clocks and power from sysfs (0 = skip)")
    ap.add_argument("--pipe-depth", type=int, default=4)
    ap.add_argument("--scan-threads", type=int, default=1, help="host threads of the pipe (the frame walk takes 0.27 ms of one core per 10 000-frame batch)")
    ap.add_argument("--no-config5", action="store_true", help="skip the mixed corpus (BASELINE configs[4]): its streams take ~20 s to synthesise")
    ap.add_argument("--no-single-file-100k", action="store_true")
    ap.add_argument("--cpu-frames", type=int, default=10000, help="frames per pass of the CPU baseline (rank 0, N=1)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="the CPU baseline repeats its pass until this much time has gone by")
    ap.add_argument("--cpu-seconds-all", type=float, default=6.0, help="duration of the all-cores run of the CPU baseline (0 = skip)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-short-files", action="store_true",
                    help="skip the e2e comparison of 250 short files (hundreds of tiny launches of every kernel: the rocprofv3 "
                         "runs pass this so that the per-kernel averages of the trace describe the full-size launches)")
    ap.add_argument("--no-overlap", action="store_true",
                    help="run the Huffman front end of batch k+1 after, not under, the transform kernels of batch k")
    ap.add_argument("--huffman-under", choices=("rate", "decode"), default="decode",
                    help="where the Huffman decode of batch k+1 starts: under the decode transforms of batch k (default since r02e: with the "
                         "tail of batch k-1 on the third stream the step takes the same time either way, and the rate loop -- the kernel the "
                         "roofline is computed from -- runs undisturbed), or under its rate loop (r02d and before)")
    ap.add_argument("--pack-overlap", action="store_true", help="(default since r02e; kept for old command lines)")
    ap.add_argument("--lean-sync", choices=("on", "off"), default="on", help="region (i): the rate loop's dispatch signals the side streams itself and the main "
                    "stream's waits stand together in front of it (MP3S_OPT_RATE_SIGNALS, mp3s_ctx_wait_last)")
    ap.add_argument("--no-tail-stream", action="store_true", help="chain check and bit packing of batch k on the main stream instead of a third one")
    ap.add_argument("--resident-only", action="store_true", help="region (i) only (profiling runs)")
    ap.add_argument("--dom-events-every", type=int, default=8, help="the timed region's HIP event pair around the dominant kernel on every N-th step: "
                    "a pair is two packets in the queue, 0.015 ms of stream time (round 5, 100 steps: on every fourth step 0.533-0.536 ms per step, on every "
                    "eighth 0.524, on every sixteenth 0.526: docs/LOG.md); 25 pairs in the default 200 steps")
    ap.add_argument("--no-live-pmc", action="store_true", help="roofline.traffic / roofline_alu from the committed profiles/*_latest.json instead of three "
                    "rocprofv3 --pmc passes run as child processes before this one touches the GPU (rank 0, one GPU, full runs only)")
    ap.add_argument("--decode-stream", choices=("on", "off"), default="off",
                    help="the decode transforms of batch k+1 on a context of their own, under the encode transforms and the rate loop of batch k")
    args = ap.parse_args()
    if args.regions is None:
        args.regions = 3 if args.full else 1

    # `python bench.py --gpus N` on its own (no torch.distributed.run in front): start the N ranks from here.  The parent
    # makes no GPU call and never exec()s; it relays rank 0's one json line and returns the worst exit code.
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import launch_ranks
        sys.exit(launch_ranks.launch([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != max(args.gpus, 1) and rank == 0:
        print(f"bench.py: --gpus {args.gpus} but the launcher set WORLD_SIZE={world}: running {world} rank(s)", file=sys.stderr)
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1:
        import torch.distributed as dist  # control plane only (barrier + max); no tensors on the data path
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # (the gloo transport announces its connections on stdout, which belongs to the ONE json line of rank 0: stderr for the time being)
        sys.stdout.flush()
        keep_out = os.dup(1)
        os.dup2(2, 1)
        try:
            dist.init_process_group(backend="gloo", rank=rank, world_size=world)
            dist.barrier()
        finally:
            sys.stdout.flush()
            os.dup2(keep_out, 1)
            os.close(keep_out)

    def reduce_max(x):
        if dist is None:
            return float(x)
        import torch
        t = torch.tensor([float(x)], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t[0])

    # every comparison behind `parity_checked`, by name: a false flag says in `parity_failures` whether BYTES differed ("bytes: ...") or a job took
    # another path than the default settings give it ("path: ...": e.g. MP3S_FILE_PIPELINE=0 in the environment -- tools/option_sweep.sh)
    parity_failures = []

    def note(label, ok):
        if not ok and label not in parity_failures:
            parity_failures.append(label)
        return bool(ok)

    def reduce_all_ok(ok):
        if dist is None:
            return bool(ok)
        import torch
        t = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(t[0] > 0.5)

    # the counters behind roofline.traffic and roofline_alu, measured in THIS run (child processes, before the GPU is touched here)
    pmc_live, pmc_note = None, "committed profile (--no-live-pmc, --resident-only, or more than one rank)"
    if args.full and world == 1 and rank == 0 and not args.no_live_pmc and not args.resident_only:
        pmc_live, pmc_note = live_pmc(args.frames)
    from mp3stego import _lib
    from synth_pcm import synth_pcm
    L = _lib.lib()
    # one rank per GPU; MP3STEGO_DEVICE pins every rank to one device (launch-path checks on a 1-GPU box)
    dev = int(os.environ.get("MP3STEGO_DEVICE", local_rank))
    ctx = _lib.Context(dev)
    n = args.frames

    # ---------------------------------------------------------------- build the resident batch (untimed)
    t_prep = time.time()
    ctx.set_option("file_pipeline", 0)     # (the preparation's one-file calls as full-size launches: the profiles of a --resident-only run hold nothing else)
    pcm_src = synth_pcm(n, seed=0x9E3779B97F4A7C15 + rank)
    hide = bits_of(MESSAGE)
    payload = MESSAGE.split("#", 1)[1]
    enc0 = ctx.encode_pcm(pcm_src, 44100, 128, None)           # the input stream: 10k frames @128 kbps
    mp3_in = bytes(enc0["mp3"])
    parsed = _lib.parse_stream(mp3_in)                          # host front end incl. Huffman (the checker for `is`)
    assert parsed["n_frames"] == n
    scanned = _lib.scan_stream(mp3_in)                          # host byte-level scan (what stays on the host)
    assert scanned["gpu_ok"] and scanned["n_frames"] == n
    d_blob = ctx.to_device(scanned["blob"])
    d_side = ctx.to_device(scanned["side"])
    # two sets of Huffman outputs: the front end of the next batch fills one while the transforms read the other
    d_is2 = [ctx.alloc(n * 2304 * 2), ctx.alloc(n * 2304 * 2)]
    d_si2 = [ctx.alloc(n * 4 * 72), ctx.alloc(n * 4 * 72)]
    d_hst2 = [ctx.alloc(16), ctx.alloc(16)]
    aux = None if args.no_overlap else _lib.Context(ctx.device)   # second stream on the same device
    # third stream: the tail of batch k (selection, scatter, chain check: four small launches, and the bit packer) runs under the decode
    # transforms of batch k+1, as in the library's pipe (csrc/pipe_jobs.cpp: s_tail) -- the small launches and their gaps are 5 %
    # of a step when they sit in front of the next batch (0.829 -> 0.785 ms per step)
    aux2 = _lib.Context(ctx.device) if not (args.no_tail_stream or args.no_overlap) else None
    # fourth stream: the int16 decode transforms wait for scalar operands half of the time (45 % of their issue slots busy), the
    # encode transforms and the rate loop are bound by them (75 - 85 %): the decode transforms of batch k+1 under the encode side of batch k
    dctx = _lib.Context(ctx.device) if (args.decode_stream == "on" and aux is not None) else None
    d_pcm2 = [ctx.alloc(n * 2304 * 2), ctx.alloc(n * 2304 * 2)] if dctx is not None else None
    d_hdr = ctx.to_device(parsed["hdr"])
    rf, _pad = _lib.rate_frames(44100, 128, 2, n)
    # the message array of a batch: the eight 3-bit patterns the variants read, then the message
    hide_all = np.concatenate([_lib.select_patterns(), np.asarray(hide, dtype=np.uint8)])
    rf["hide_end"] = len(hide_all)
    d_rf = ctx.to_device(rf)
    d_hide = ctx.to_device(hide_all)
    units = n * 4
    d_pcm = ctx.alloc(n * 2304 * 2)
    d_pcm32 = ctx.alloc(n * 2304 * 4)
    d_mdct2 = [ctx.alloc(n * 2304 * 4), ctx.alloc(n * 2304 * 4)]   # (the tail of batch k may read its spectra while batch k + 1 writes its own)
    d_mdct = d_mdct2[0]
    d_ix = ctx.alloc(n * 2304 * 2)
    d_out = ctx.alloc(units * 72)
    d_en = ctx.alloc(units * 22 * 4)
    slots = (128 * 1000 * 1152 // 8) // 44100
    frame_off = np.concatenate([[0], np.cumsum(slots + _pad)]).astype(np.uint32)
    d_off = ctx.to_device(frame_off)
    d_pad = ctx.to_device(_pad.astype(np.uint8))
    d_mp3 = ctx.alloc(int(frame_off[-1]) + 16)
    d_sc = ctx.alloc(n * 8 * 4)
    d_pst = ctx.alloc(16)
    # the serial chains.  The message cursor is decided on the device (what the library's own pipeline does for a short
    # message): the units the message can reach run once per possibility as extra entries of the rate-loop launch, a
    # small kernel walks the chain and puts the entry each unit really sees in its place, and the chain check confirms.
    seg = np.zeros(1, dtype=_lib.CHAIN_SEG_DTYPE)
    seg["n_frames"], seg["hide_base"], seg["hide_begin"], seg["hide_end"] = n, 32, 32, len(hide_all)
    d_seg = ctx.to_device(seg)
    spans, ent_unit, ent_cursor = _lib.select_plan(seg, max(units // 2, 8192))
    n_ent, max_reach = len(ent_unit), int(spans["reach"].max())
    assert n_ent > 0, "the bench payload is a short message: the device decides its cursor chain"
    d_spans, d_eu, d_ec = ctx.to_device(spans), ctx.to_device(ent_unit), ctx.to_device(ent_cursor)
    d_ixv, d_outv, d_env = ctx.alloc(n_ent * 1152), ctx.alloc(n_ent * 72 + ((n_ent + 15) & ~15)), ctx.alloc(n_ent * 88)
    d_cur = ctx.to_device(np.full(units, _lib.NO_CURSOR, dtype=np.int32))
    d_cur0 = ctx.to_device(np.full(units, _lib.NO_CURSOR, dtype=np.int32))   # what every step starts from (the library uploads fresh cursors with every job)
    d_verdict = ctx.alloc(16)
    d_segout = ctx.alloc(80)

    # the library's own answer for the same job (device pipeline of mp3s_encode_pcm: same kernels, same chain check); --full checks against it
    if args.full:
        pcm16 = ctx.decode_stream(mp3_in, _lib.MP3S_PCM_I16)["pcm"]
        final = ctx.encode_pcm(pcm16, 44100, 128, hide)
        gr = final["gr"]
    prep_s = time.time() - t_prep
    ctx.set_option("file_pipeline", 1)

    state = {"k": 0, "lean": args.lean_sync == "on" and aux is not None and aux2 is not None and dctx is None and args.huffman_under == "decode"}
    if state["lean"]:
        ctx.set_option("rate_signals", 1)

    def front_end(c, k):
        b = k & 1
        _lib.check(L.mp3s_huffman_decode_dev(c.handle, d_blob, d_side, n, 2, scanned["max_part2_3_length"],
                                             d_is2[b], d_si2[b], d_hst2[b]))

    def decode_side(k):
        b = k & 1
        dctx.wait_for(aux)                          # Huffman(k) done
        _lib.check(L.mp3s_decode_transform_dev(dctx.handle, d_is2[b], d_si2[b], d_hdr, n, 2, 0, _lib.MP3S_PCM_I16, d_pcm2[b]))

    def step4():
        # the same step with the decode transforms on a context of their own, one batch ahead of the encode side
        k = state["k"]; state["k"] = k + 1
        b = k & 1
        if k == 0 or state.get("restart"):
            front_end(aux, k); state["restart"] = False
            decode_side(k)
        ctx.wait_for(dctx)                          # decode(k) done: its PCM is there
        if not state.get("last"):
            aux.wait_for(dctx)                      # decode(k-1) has read the Huffman outputs batch k+1 overwrites
            front_end(aux, k + 1)
            dctx.wait_for(ctx)                      # the encode transforms of batch k-1 have read the PCM buffer batch k+1 writes
            decode_side(k + 1)
        d_mdct = d_mdct2[b]
        _lib.check(L.mp3s_encode_transform_dev(ctx.handle, d_pcm2[b], d_hdr, n, d_mdct))
        if aux2 is not None:
            ctx.wait_for(aux2)
        _lib.check(L.mp3s_rate_variants_dev(ctx.handle, d_mdct, d_rf, n, d_hide, len(hide_all), d_cur, d_eu, d_ec, n_ent, d_ix, d_out, d_en,
                                            d_ixv, d_outv, d_env))
        pk = ctx
        if aux2 is not None:
            aux2.wait_for(ctx)
            pk = aux2
        _lib.check(L.mp3s_select_dev(pk.handle, d_hide, d_cur, d_seg, d_spans, 1, max_reach, d_eu, d_ec, n_ent, d_ix, d_out, d_en, d_ixv, d_outv, d_env))
        _lib.check(L.mp3s_chain_redo_dev(pk.handle, d_mdct, d_rf, n, d_hide, len(hide_all), d_cur, d_seg, 1, d_ix, d_out, d_en, d_verdict, d_segout))
        _lib.check(L.mp3s_pack_frames_dev(pk.handle, d_ix, d_out, d_en, n, 44100, 128, d_off, d_pad, d_mp3, d_sc, d_pst))
        _lib.check(L.mp3s_dev_copy(pk.handle, d_cur, d_cur0, units * 4))     # (see step)

    def step():
        if dctx is not None:
            return step4()
        # One step = one batch through the whole device pipeline.  With the second stream the batches are software
        # pipelined: the latency-bound Huffman decode of batch k+1 runs under the encode half of batch k.  Every
        # batch still gets its own Huffman launch inside the timed region (the first one is issued by the first step).
        k = state["k"]; state["k"] = k + 1
        b = k & 1
        # `lean`: the rate loop's dispatch signals the order event itself (MP3S_OPT_RATE_SIGNALS) and both side streams wait for THAT
        # (wait_last: no record packet on the main stream), and the main stream's wait for the Huffman decode of batch k + 1 stands in
        # front of the rate loop of batch k, beside its wait for the tail of batch k - 1: nothing lies between the rate loop and the decode
        # behind it.  (A record or a wait is a packet of its own in the queue and costs the stream 7-8 us: tools/timeline.sh.)
        lean = state["lean"]
        first = False
        if aux is None:
            front_end(ctx, k)
        else:
            if k == 0 or state.get("restart"):
                front_end(aux, k); state["restart"] = False
                ctx.wait_for(aux)                   # Huffman(k) done
                first = lean
            elif not lean:
                ctx.wait_for(aux)                   # Huffman(k) done
        if aux is not None and not state.get("last") and args.huffman_under == "decode" and not first:
            if lean:
                aux.wait_last(ctx)                  # batch k-1 is through (its rate loop's own signal): its Huffman outputs may be overwritten
            else:
                aux.wait_for(ctx)                   # batch k-1 is through: its Huffman outputs may be overwritten
            front_end(aux, k + 1)
            if lean:
                aux.wait_for(aux2)                  # ... and behind it the front stream waits for the tail of batch k-1: the main stream's ONE wait (below) is for both
        _lib.check(L.mp3s_decode_transform_dev(ctx.handle, d_is2[b], d_si2[b], d_hdr, n, 2, 0, _lib.MP3S_PCM_I16, d_pcm))
        if first and not state.get("last"):
            # (a run's first step: no rate loop stands in front whose end would release the next Huffman decode -- released at once it
            #  takes its CUs before this step's decode gets there, which then runs beside it at half speed (tools/timeline_head.sh).  Behind the decode.)
            aux.wait_for(ctx)
            front_end(aux, k + 1)
            aux.wait_for(aux2)
        d_mdct = d_mdct2[b]
        _lib.check(L.mp3s_encode_transform_dev(ctx.handle, d_pcm, d_hdr, n, d_mdct))
        if aux is not None and not state.get("last") and args.huffman_under == "rate":
            aux.wait_for(ctx)                       # decode(k-1) has read its inputs; start under the rate loop, the longest kernel
            front_end(aux, k + 1)
        if aux2 is not None and (not lean or state.get("last")):
            ctx.wait_for(aux2)                      # the packer of batch k-1 has read what the rate loop is about to overwrite
        if lean and not state.get("last"):
            ctx.wait_for(aux)                       # Huffman(k+1) done AND the tail of batch k-1 through: the decode of batch k+1 follows this rate loop directly
        _lib.check(L.mp3s_rate_variants_dev(ctx.handle, d_mdct, d_rf, n, d_hide, len(hide_all), d_cur, d_eu, d_ec, n_ent, d_ix, d_out, d_en,
                                            d_ixv, d_outv, d_env))
        pk = ctx
        if aux2 is not None:
            if lean:
                aux2.wait_last(ctx)                 # the rate loop of batch k is through: its tail goes on the third stream
            else:
                aux2.wait_for(ctx)                  # the rate loop of batch k is through: its tail goes on the third stream
            pk = aux2
        _lib.check(L.mp3s_select_dev(pk.handle, d_hide, d_cur, d_seg, d_spans, 1, max_reach, d_eu, d_ec, n_ent, d_ix, d_out, d_en, d_ixv, d_outv, d_env))
        _lib.check(L.mp3s_chain_redo_dev(pk.handle, d_mdct, d_rf, n, d_hide, len(hide_all), d_cur, d_seg, 1, d_ix, d_out, d_en, d_verdict, d_segout))
        _lib.check(L.mp3s_pack_frames_dev(pk.handle, d_ix, d_out, d_en, n, 44100, 128, d_off, d_pad, d_mp3, d_sc, d_pst))
        # "behind every message" for every unit again: nothing of this step's cursors is reused by the next one (the array starts
        # out that way; the copy rides at the end of the tail, whose stream the next rate loop waits for, not in front of that loop)
        _lib.check(L.mp3s_dev_copy(pk.handle, d_cur, d_cur0, units * 4))

    def barrier():
        ctx.sync()
        if aux is not None:
            aux.sync()
        if aux2 is not None:
            aux2.sync()
        if dctx is not None:
            dctx.sync()
        if dist is not None:
            dist.barrier()

    dom = None

    def run(steps, events_every=0):
        state["restart"] = True                      # the first step of a run issues its own front end
        for i in range(steps):
            state["last"] = i == steps - 1           # ... and the last one does not start a batch nobody finishes
            if events_every > 1:                     # (the timed region: event pairs on a sample of its steps; a mask, nothing is waited for)
                for c in (ctx, aux, aux2, dctx):
                    if c is not None:
                        c.profile_select([dom] if i % events_every == 0 else [])
            step()

    run(args.warmup)
    barrier()

    def collect():
        pr = ctx.profile_collect()
        on_main = {kname for kname, (ms, cnt) in pr.items() if cnt}          # launched on the main stream
        for c in (aux, aux2, dctx):
            if c is not None:
                for kname, (ms, cnt) in c.profile_collect().items():
                    pr[kname] = (pr[kname][0] + ms, pr[kname][1] + cnt)
        return pr, on_main

    # ---- untimed pass with an event pair around every kernel (--full): the per-kernel table and the choice of the dominant one.
    #      (An event pair costs stream time -- about 0.05 ms per step for all kernels -- so the timed region below
    #      carries them only around the dominant kernel, whose duration the roofline is computed from.)  A plain run takes the same
    #      steps without event pairs (behind the W = 5 warm-up steps alone, its region of the driver's 20 steps read 2-5 % low).
    if args.full:
        for c in (ctx, aux, aux2, dctx):
            if c is not None:
                c.profile_select(None)
                c.profile_enable(True)
    n_prof = max(3, min(10, args.steps))
    run(n_prof)
    barrier()
    if args.full:
        prof_all, main_kernels = collect()
        per_step = {k: ms / n_prof for k, (ms, cnt) in prof_all.items()}          # ms per step
        # the dominant kernel is picked among those on the main stream: the front end on the second stream runs under
        # them (its own duration is stretched by sharing the CUs and is not what bounds the step)
        dom = max((kname for kname in per_step if kname in main_kernels), key=per_step.get)
        # ---- timed region (i): K steps, HIP events around the dominant kernel only
        for c in (ctx, aux, aux2, dctx):
            if c is not None:
                c.profile_select([dom])
                c.profile_enable(True)
    # The contract's region -- barrier, EXACTLY K steps, barrier -- is timed `--regions` times back to back (default 3 with --full, else 1); `value` is
    # the median region, value_min / value_max the others: one region of the driver's 20 steps is 10 ms, of which 0.3-0.4 are the three streams
    # filling and draining, and moved between 18.2 and 19.2 M frames/s from one machine to the next (round-5 verdict, item 3).
    walls, gpu_mss = [], []
    # The W warm-up steps once more, directly in front of the first region (no event pairs): between the warm-up at the top and this point lie
    # the per-kernel pass, its collection and a few ms of host work with the device idle, and the first of three regions read 0.4-2 % below the
    # other two every time (value_regions, r06) -- the later regions start the moment the one before has ended.  A plain run times ONE region,
    # and the median of --full's three never is the first: behind W = 5 here (20 untimed steps in all) its region of the driver's 20 steps
    # read 0.5-2 % below --full's median, as --full's first region does; it warms up on PLAIN_SETTLE_STEPS here instead, as many steps as stand
    # in front of --full's second region at --steps 20 --warmup 5 (then 0.5183 ms per step against the median region's 0.5206, five runs each, alternating).
    if args.full:
        for c in (ctx, aux, aux2, dctx):
            if c is not None:
                c.profile_select([])
    run(args.warmup if args.full else max(args.warmup, PLAIN_SETTLE_STEPS))
    if args.full:
        for c in (ctx, aux, aux2, dctx):
            if c is not None:
                c.profile_select([dom])
    for _ in range(max(1, args.regions)):
        barrier()
        t0 = time.perf_counter()
        ctx.timer_start()
        run(args.steps, max(1, args.dom_events_every) if args.full else 0)
        gpu_mss.append(ctx.timer_stop())
        barrier()
        walls.append(time.perf_counter() - t0)
    order = sorted(range(len(walls)), key=lambda i: walls[i])
    wall, gpu_ms = walls[order[len(order) // 2]], gpu_mss[order[len(order) // 2]]
    if args.full:
        prof, _ = collect()
        for c in (ctx, aux, aux2, dctx):
            if c is not None:
                c.profile_enable(False)
                c.profile_select(None)
    d_is, d_si, d_hst = d_is2[(state["k"] - 1) & 1], d_si2[(state["k"] - 1) & 1], d_hst2[(state["k"] - 1) & 1]
    d_pcm_last = d_pcm if dctx is None else d_pcm2[(state["k"] - 1) & 1]
    max_step = reduce_max(wall / args.steps)
    value = n * world / max_step
    verdict = ctx.download(d_verdict, np.int32, (2,))
    segout = ctx.download(d_segout, _lib.CHAIN_SEG_OUT_DTYPE, (1,))
    if args.dump_outputs and rank == 0:
        # (a caller gets the stream without its last len % 4 bytes: the library writes whole words, as the reference does -- the check below)
        dump_outputs(args.dump_outputs, ctx.download(d_mp3, np.uint8, ((int(frame_off[-1]) // 4) * 4,)), int(segout["cursor"][0]) - 32,
                     ctx.download(d_pcm_last, np.int16, (n * 1152, 2)))
    config = {"workload": f"{n}-frame full decode->stego-embed->re-encode pipeline per MI355X (BASELINE "
                          "configs[2]); MP3 main data + side info resident in HBM, MP3 frames out; the message cursor chain is "
                          "decided and the serial chains of the rate loop are checked on the device inside every step", "frames_per_gpu": n,
              "sample_rate": 44100, "channels": 2, "bitrate_kbps": 128, "message_bits": int(len(hide)),
              "chain_verdict_units_to_redo": int(verdict[0]), "message_variant_entries": n_ent}
    if not args.full:
        # ---------------------------------------------------------------- a plain run ends here: the headline and what it was measured on
        if rank == 0:
            config["parallelism"] = f"frames sharded over {world} GPU(s), no collective"
            print(json.dumps({                      # (--full prints these fields and everything else it measures: the block at the end)
                "metric": METRIC, "value": round(value, 1), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
                "warmup": args.warmup, "ms_per_step": round(max_step * 1e3, 4), "higher_is_better": True,
                "scaling": "weak", "vs_baseline": None, "dtype": "f64 (decode) / int32 (encode)", "data": "synthetic", "config": config,
                "full": False, "timed_regions": len(walls), "gpu_event_ms_per_step": round(gpu_ms / args.steps, 4), "timed_region_s": round(wall, 4),
                "front_end_overlap": aux is not None, "tail_stream": aux2 is not None, "prep_s": round(prep_s, 2), "device": ctx.device_name()}))
        for c in (aux, aux2, dctx):
            if c is not None:
                c.close()
        ctx.close()
        if dist is not None:
            dist.destroy_process_group()
        return

    # ---------------------------------------------------------------- verify the timed work (untimed)
    got_gr = ctx.download(d_out, _lib.GR_OUT_DTYPE, (units,))
    got_ix = ctx.download(d_ix, np.int16, (n, 2, 2, 576))
    got_pcm = ctx.download(d_pcm_last, np.int16, (n * 1152, 2))
    got_mp3 = ctx.download(d_mp3, np.uint8, (int(frame_off[-1]),)).tobytes()
    same = note("bytes: resident step, chain verdict", int(verdict[0]) == 0 and int(verdict[1]) == 0)          # the chain check agrees: the step was the whole job
    same = note("bytes: resident step, message cursor", int(segout["cursor"][0]) - 32 == int(final["hide_offset"])) and same
    same = note("bytes: resident step, PCM and MP3", bool(np.array_equal(got_pcm, pcm16)) and got_mp3[:(len(got_mp3) // 4) * 4] == final["mp3"]) and same
    same = note("bytes: resident step, Huffman values", bool(np.array_equal(ctx.download(d_is, np.int16, (n, 2, 2, 576)), parsed["is"]))) and same
    same = note("bytes: resident step, kernel status words", int(ctx.download(d_hst, np.int32, (1,))[0]) == 0 and int(ctx.download(d_pst, np.int32, (1,))[0]) == 0) and same
    for k in ("part2_3_length", "big_values", "count1", "table_select", "count1table_select", "region0_count",
              "region1_count", "n_tables", "quantizer_step", "address"):
        same = note("bytes: resident step, GrInfo." + k, bool(np.array_equal(got_gr[k], gr[k]))) and same
    mp3_final = final["mp3"]
    # oracle check on a bounded prefix (the codec is causal: the first frames of the stream depend on nothing later)
    import oracle_lib as O
    k = 64
    o_dec = O.decode(mp3_in[:int(parsed["frame_size"][:k + 1].sum())])
    o_pcm = O.pcm_to_i16(o_dec["pcm"])[:k * 1152]
    o_enc = O.encode(o_pcm, 44100, 128, hide)
    oracle_ok = bool(np.array_equal(o_pcm, got_pcm[:k * 1152])) and \
        bool(np.array_equal(o_enc["ix"].astype(np.int16)[:k - 1], got_ix[:k - 1])) and \
        mp3_final[:len(o_enc["mp3"]) - 8] == o_enc["mp3"][:len(o_enc["mp3"]) - 8]

    value_min = n * world / reduce_max(max(walls) / args.steps)
    value_max = n * world / reduce_max(min(walls) / args.steps)
    value_regions = [round(n * world / reduce_max(w / args.steps), 1) for w in walls]       # (in the order they were timed)

    # ---------------------------------------------------------------- the same step on FOUR streams (reported beside `value`, not as it)
    four = None
    if dctx is None and aux is not None and aux2 is not None and not args.resident_only:
        dctx = _lib.Context(ctx.device)
        d_pcm2 = [ctx.alloc(n * 2304 * 2), ctx.alloc(n * 2304 * 2)]
        dctx.profile_select([dom]); ctx.profile_select([dom])
        run(args.warmup + 2)
        barrier()
        dctx.profile_enable(True); ctx.profile_enable(True)
        t0 = time.perf_counter()
        run(args.steps)
        barrier()
        w4 = time.perf_counter() - t0
        p4 = ctx.profile_collect()
        for c in (ctx, dctx):
            c.profile_enable(False); c.profile_select(None)
        ok4 = int(ctx.download(d_verdict, np.int32, (2,))[0]) == 0 and ctx.download(d_mp3, np.uint8, (int(frame_off[-1]),)).tobytes() == got_mp3
        same = note("bytes: four-stream step", ok4) and same
        t4 = reduce_max(w4 / args.steps)
        four = {"frames_per_s": round(n * world / t4, 1), "ms_per_step": round(t4 * 1e3, 4), "steps": args.steps,
                "dominant_kernel_ms_per_launch": round(p4[dom][0] / max(p4[dom][1], 1), 4),
                "what": "the same step with the decode transforms of batch k+1 on a fourth context, under the encode transforms and the rate loop of batch k "
                        "(they wait for scalar operands half of the time, the encode side is bound by the vector units): +2-3 % frames per second over "
                        "200 steps, less than `value` over the driver's 20 (a longer fill and drain); every kernel -- the rate loop too -- takes longer "
                        "beside the others, which is why `value` and the roofline stay with three streams"}
        dctx.close(); dctx = None

    # the resident steps are over: their helper contexts (second / third / fourth stream) go now -- the host-fed regions below are what
    # a caller's process looks like, one context and the library's own streams (every stream a process holds takes part in the
    # runtime's mapping of streams onto hardware queues)
    front_end_overlap, tail_stream = aux is not None, aux2 is not None
    barrier()
    for c in (aux, aux2, dctx):
        if c is not None:
            c.close()
    aux = aux2 = dctx = None
    # ---------------------------------------------------------------- decode only (BASELINE config 2), resident, kernel-only
    decode_only = None
    if not args.resident_only:
        # as in region (i): the Huffman decode of batch k + 1 on a second context's stream, under the transforms of batch k, two sets of
        # `is` / side records taken in turn (every batch gets its own Huffman launch inside the timed loop); `serial_ms_per_step` = both on one stream
        hctx = None if args.no_overlap else _lib.Context(ctx.device)
        dstate = {"i": 0, "fmt": _lib.MP3S_PCM_F32, "out": d_pcm32}

        def dec_step():
            fmt, d_out = dstate["fmt"], dstate["out"]
            i = dstate["i"]; dstate["i"] = i + 1
            if hctx is None:
                _lib.check(L.mp3s_huffman_decode_dev(ctx.handle, d_blob, d_side, n, 2, scanned["max_part2_3_length"], d_is2[0], d_si2[0], d_hst2[0]))
                _lib.check(L.mp3s_decode_transform_dev(ctx.handle, d_is2[0], d_si2[0], d_hdr, n, 2, 0, fmt, d_out))
                return
            cur, nxt = i & 1, (i + 1) & 1
            if i == 0:
                _lib.check(L.mp3s_huffman_decode_dev(hctx.handle, d_blob, d_side, n, 2, scanned["max_part2_3_length"], d_is2[cur], d_si2[cur], d_hst2[cur]))
            ctx.wait_for(hctx)                      # batch i's Huffman output is there
            hctx.wait_for(ctx)                      # ... and the transforms that read the other set are through
            _lib.check(L.mp3s_huffman_decode_dev(hctx.handle, d_blob, d_side, n, 2, scanned["max_part2_3_length"], d_is2[nxt], d_si2[nxt], d_hst2[nxt]))
            _lib.check(L.mp3s_decode_transform_dev(ctx.handle, d_is2[cur], d_si2[cur], d_hdr, n, 2, 0, fmt, d_out))

        def dec_sync():
            ctx.sync()
            if hctx is not None:
                hctx.sync()

        def dec_serial(k):
            t0 = time.perf_counter()
            for _ in range(k):
                _lib.check(L.mp3s_huffman_decode_dev(ctx.handle, d_blob, d_side, n, 2, scanned["max_part2_3_length"], d_is2[0], d_si2[0], d_hst2[0]))
                _lib.check(L.mp3s_decode_transform_dev(ctx.handle, d_is2[0], d_si2[0], d_hdr, n, 2, 0, dstate["fmt"], dstate["out"]))
            ctx.sync()
            return (time.perf_counter() - t0) / k * 1e3
        for _ in range(3):
            dec_step()
        dec_sync()
        kd = max(20, args.steps // 2)
        dms_serial = dec_serial(kd)
        dstate["i"] = 0
        t0 = time.perf_counter()
        for _ in range(kd):
            dec_step()
        dec_sync()
        dms_overlap = (time.perf_counter() - t0) / kd * 1e3
        dms = min(dms_overlap, dms_serial)           # (the better of the two arrangements, named in the record)
        f32 = ctx.download(d_pcm32, np.float32, (n * 1152, 2))
        f64 = ctx.decode_stream(mp3_in, _lib.MP3S_PCM_F64)["pcm"]
        same = note("bytes: decode_only float32 exact", bool(np.array_equal(f32, f64.astype(np.float32)))) and same
        del f64
        # ... and with MP3S_OPT_FLOAT_FAST: float32 through the mirrored, fused IMDCT and the split synthesis (within 1e-5, not bit-identical)
        ctx.set_option("float_fast", 1)
        dstate["i"] = 0
        for _ in range(3):
            dec_step()
        dec_sync()
        dms_fast_serial = dec_serial(kd)
        dstate["i"] = 0
        t0 = time.perf_counter()
        for _ in range(kd):
            dec_step()
        dec_sync()
        dms_fast_overlap = (time.perf_counter() - t0) / kd * 1e3
        dms_fast = min(dms_fast_overlap, dms_fast_serial)
        f32f = ctx.download(d_pcm32, np.float32, (n * 1152, 2))
        ctx.set_option("float_fast", 0)
        # ... and to int16, the reference's own decode product (MP3_Parser.py:91: the WAV it writes is (pcm * 32767).astype(int16)): the stream
        # kernel behind its guard + the fix-up kernel, bit-identical
        dstate.update(i=0, fmt=_lib.MP3S_PCM_I16, out=d_pcm)
        for _ in range(3):
            dec_step()
        dec_sync()
        dms_i16_serial = dec_serial(kd)
        dstate["i"] = 0
        t0 = time.perf_counter()
        for _ in range(kd):
            dec_step()
        dec_sync()
        dms_i16_overlap = (time.perf_counter() - t0) / kd * 1e3
        dms_i16 = min(dms_i16_overlap, dms_i16_serial)
        same = note("bytes: decode_only int16", bool(np.array_equal(ctx.download(d_pcm, np.int16, (n * 1152, 2)), np.asarray(pcm16).reshape(-1, 2)))) and same
        dstate.update(i=0, fmt=_lib.MP3S_PCM_F32, out=d_pcm32)
        f64r = f32.astype(np.float64)        # (the exact kernels' float32 = the reference's float64 rounded once: the comparison is against that)
        dd = np.abs(f32f.astype(np.float64) - f64r)
        bigm = np.abs(f64r) > 1e-6
        fast_err = {"max_abs": float(dd.max()), "max_rel_where_abs_above_1e-6": float((dd[bigm] / np.abs(f64r[bigm])).max()),
                    "samples_that_differ": int((f32f != f32).sum()), "samples": int(f32.size)}
        same = note("tolerance: decode_only float32 fast within 1e-5", bool(np.allclose(f32f, f64r, rtol=1e-5, atol=1e-9))) and same
        del f32f, f64r, dd, bigm
        decode_only = {"workload": f"{n} frames, Huffman decode + decode transforms -> float32 PCM, resident (BASELINE configs[1])",
                       "float_fast": {"ms_per_step": round(dms_fast, 4), "frames_per_s": round(n / (dms_fast * 1e-3), 1), "serial_ms_per_step": round(dms_fast_serial, 4),
                                      "overlapped_ms_per_step": round(dms_fast_overlap, 4), "error_vs_exact_float32": fast_err,
                                      "what": "MP3S_OPT_FLOAT_FAST = 1: the same step through the fast sums, unguarded; default (the numbers beside this) = bit-identical to the reference"},
                       "frames_per_s": round(n / (dms * 1e-3), 1), "ms_per_step": round(dms, 4), "serial_ms_per_step": round(dms_serial, 4), "overlapped_ms_per_step": round(dms_overlap, 4), "steps": kd,
                       "arrangements": "serial = Huffman decode and transforms of a batch on one stream; overlapped = the Huffman decode of batch k + 1 on a second "
                                       "context's stream under the transforms of batch k (as in region (i)); ms_per_step = the faster of the two",
                       "hbm_gbs_algorithmic": round(B_DEC * n / (dms * 1e-3) / 1e9, 2),
                       "hbm_frac": round(B_DEC * n / (dms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                       "headline": "the config-2 number is frames_per_s / ms_per_step / hbm_frac on THIS level: the default, float32 bit-identical to the "
                                   "reference's float64 rounded once (the exact kernels); float_fast is the option within north_star's 1e-5; `int16` is the same step to the "
                                   "samples the reference's decoder actually writes (its WAV), bit-identical through the guarded stream kernel",
                       }
        decode_only["float_fast"]["hbm_frac"] = round(B_DEC * n / (dms_fast * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)
        decode_only["int16"] = {"ms_per_step": round(dms_i16, 4), "frames_per_s": round(n / (dms_i16 * 1e-3), 1), "serial_ms_per_step": round(dms_i16_serial, 4),
                                "overlapped_ms_per_step": round(dms_i16_overlap, 4), "hbm_frac": round(9520 * n / (dms_i16 * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                                "what": "the same step to int16 PCM -- the reference's own decode product (MP3_Parser.py:91 writes (pcm * 32767).astype(int16) as the WAV): "
                                        "k_dec_stream behind its guard + k_dec_fixup, bit-identical; 9 520 algorithmic bytes per frame (4 912 in + 4 608 out)"}
        if hctx is not None:
            hctx.close()

    # ---------------------------------------------------------------- regions (ii) and (iii): host-fed
    regions, e2e_steady, short_files, long_message, sustained, octx = {}, None, None, None, None, None
    if not args.resident_only:
        # ONE file per call (the reference's call shape): the file goes through the overlapped stages as chunks.  On a context of the
        # caller's own, made here -- a context's pipe chooses its streams when it is made, and this process held three more contexts
        # while the resident steps ran (the main context's pipe dates from then)
        octx = _lib.Context(dev)
        t0 = time.perf_counter()
        hid = octx.hide_message(mp3_in, payload)                  # the first call makes the pipe
        t_first = time.perf_counter() - t0
        same = note("bytes: hide_message against the resident result", bytes(hid["data"]) == bytes(final["mp3"])) and same
        ref_out = bytes(hid["data"])
        del hid
        frs = octx.run_stats()
        first_call = {"ms": round(t_first * 1e3, 3), "rehearsal_ms": round(frs["rehearsal_us"] / 1e3, 3), "rehearsals": frs["rehearsals"],
                      "lanes": frs["lanes"], "queue_shared": frs["queue_shared"],
                      "what": "the first hide_message of a fresh context: pipe creation (three slots of page-locked staging + device buffers) + the rehearsal "
                              "that chooses its streams (at most 12 miniature jobs / 15 ms, judged against the same miniature on one stream) + the call"}
        k1 = 30
        rs0 = octx.run_stats()
        t0 = time.perf_counter()
        for _ in range(k1):
            r = octx.hide_message(mp3_in, payload)
        t_one = (time.perf_counter() - t0) / k1
        rs1 = octx.run_stats()
        same = note("bytes: one file per call", bytes(r["data"]) == ref_out) and note("path: one file per call went through the file pipeline", rs1["files"] - rs0["files"] == k1) and same
        del r
        # (the main context, whose pipe was made beside the helper contexts of the resident steps: reported, not used)
        r = ctx.hide_message(mp3_in, payload)
        t0 = time.perf_counter()
        for _ in range(k1):
            r = ctx.hide_message(mp3_in, payload)
        t_main = (time.perf_counter() - t0) / k1
        same = note("bytes: one file per call (variant)", bytes(r["data"]) == ref_out) and same
        del r
        first_call["ms_per_call_on_the_context_of_the_resident_steps"] = round(t_main * 1e3, 4)
        # ... and through the drop-in facade: Steganography.hide_message(quiet=True), files on a RAM disk where there is one
        import shutil
        import tempfile
        from mp3stego import Steganography
        tdir = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None)
        t_fac = t_fac_new = None
        try:
            src, dst = os.path.join(tdir, "in.mp3"), os.path.join(tdir, "out.mp3")
            open(src, "wb").write(mp3_in)
            st = Steganography(quiet=True)
            st.hide_message(src, dst, payload)
            t0 = time.perf_counter()
            for _ in range(10):
                st.hide_message(src, dst, payload)
            t_fac = (time.perf_counter() - t0) / 10
            same = note("bytes: the facade's output file", open(dst, "rb").read() == ref_out) and same
            # ... into a file that is not there yet (the library writes the result chunk by chunk under the device's work; over a file that holds
            # something -- above -- it is written when the call has succeeded, as the reference leaves such a file alone when its encode fails)
            ts = []
            for _ in range(10):
                os.remove(dst)
                t0 = time.perf_counter()
                st.hide_message(src, dst, payload)
                ts.append(time.perf_counter() - t0)
            t_fac_new = sorted(ts)[len(ts) // 2]
            same = note("bytes: the facade's output file", open(dst, "rb").read() == ref_out) and same
        finally:
            shutil.rmtree(tdir, ignore_errors=True)
        regions["single_file_10k"] = {"ms_per_batch": round(t_one * 1e3, 4), "frames_per_s": round(n / t_one, 1), "batches": k1, "first_call": first_call,
                                      "chunks_per_file": round((rs1["chunks"] - rs0["chunks"]) / k1, 2),
                                      "facade_ms_per_file": round(t_fac * 1e3, 4) if t_fac else None,
                                      "facade_new_file_ms": round(t_fac_new * 1e3, 4) if t_fac else None,
                                      "what": "Context.hide_message(bytes) = ONE mp3s_hide_message call per file, a loop of them: the file's chunks through walk || upload || "
                                              "parse + Huffman || kernels || download; facade_ms_per_file = Steganography.hide_message(quiet=True) on files (read + the same call + write)"}
        # the same file with the stages one after the other (round 2's path, kept as the fallback)
        octx.set_option("file_pipeline", 0)
        r = octx.hide_message(mp3_in, payload)
        t0 = time.perf_counter()
        for _ in range(k1):
            r = octx.hide_message(mp3_in, payload)
        t_seq = (time.perf_counter() - t0) / k1
        same = note("bytes: one file per call (variant)", bytes(r["data"]) == ref_out) and same
        del r
        octx.set_option("file_pipeline", 1)
        regions["bytes_to_bytes_one_at_a_time"] = {"ms_per_batch": round(t_seq * 1e3, 4), "frames_per_s": round(n / t_seq, 1), "batches": k1,
                                                   "what": "mp3s_hide_message with MP3S_OPT_FILE_PIPELINE = 0: host scan + upload + kernels + download, nothing overlapped (round 2's path)"}
        if not args.no_single_file_100k and n >= 1000:
            # a 100 000-frame file: the stream's complete frames ten times over (every frame of this encoder stands alone: main_data_begin = 0)
            fsz = parsed["frame_size"].astype(np.int64)
            reps = max(1, 100000 // (n - 1))
            big = mp3_in[:int(fsz[:n - 1].sum())] * reps
            nbig = (n - 1) * reps
            octx.set_option("file_pipeline", 0)
            big_ref = octx.hide_message(big, payload)
            big_out = bytes(big_ref["data"]); del big_ref
            octx.set_option("file_pipeline", 1)
            r = octx.hide_message(big, payload)
            rs0 = octx.run_stats()
            kb = 8
            t0 = time.perf_counter()
            for _ in range(kb):
                r = octx.hide_message(big, payload)
            t_big = (time.perf_counter() - t0) / kb
            rs1 = octx.run_stats()
            same = note("bytes: 100 000-frame file", same_bytes(r["data"], big_out)) and note("path: 100 000-frame file went through the file pipeline", rs1["files"] - rs0["files"] == kb) and same
            del r
            r = octx.decode_file(big); del r                      # (the first call pins its 460 MB result block)
            t0 = time.perf_counter()
            for _ in range(3):
                r = octx.decode_file(big); del r
            t_bigdec = (time.perf_counter() - t0) / 3
            regions["single_file_100k"] = {"ms_per_batch": round(t_big * 1e3, 3), "frames_per_s": round(nbig / t_big, 1), "batches": kb, "frames": nbig,
                                           "bytes": len(big), "chunks_per_file": round((rs1["chunks"] - rs0["chunks"]) / kb, 2),
                                           "decode_file_ms": round(t_bigdec * 1e3, 3), "decode_file_frames_per_s": round(nbig / t_bigdec, 1),
                                           "what": "one mp3s_hide_message call on a 42 MB file, bytes -> bytes (compared with the stages-one-after-the-other result); "
                                                   "decode_file = MP3 -> WAV of the same file (460 MB of PCM down)"}
            del big, big_out
        kd = 10
        r = octx.decode_stream(mp3_in, _lib.MP3S_PCM_I16); del r
        t0 = time.perf_counter()
        for _ in range(kd):
            r = octx.decode_stream(mp3_in, _lib.MP3S_PCM_I16)
            del r
        t_dec = (time.perf_counter() - t0) / kd
        regions["decode_stream_bytes_to_pcm"] = {"ms_per_batch": round(t_dec * 1e3, 4), "frames_per_s": round(n / t_dec, 1), "batches": kd,
                                                 "what": "mp3s_decode_stream in a loop (46 MB of int16 PCM down per batch)"}
        # a message the cursor guess cannot cover: the chain is resolved by the message-variant launches (host walk)
        long_text = "".join(chr(32 + (i * 7) % 90) for i in range(1700))
        r = octx.hide_message(mp3_in, long_text)
        long_ref = bytes(r["data"]); del r
        t0 = time.perf_counter()
        for _ in range(5):
            r = octx.hide_message(mp3_in, long_text)
        t_long = (time.perf_counter() - t0) / 5
        long_message = {"message_bytes": len(long_text), "ms_per_batch": round(t_long * 1e3, 3), "frames_per_s": round(n / t_long, 1),
                        "too_long": bool(r["too_long"]),
                        "what": "a 1 700-byte message (reach 4 889 units: 39 826 variant entries behind the 40 000 units of the rate-loop launch, five rounds of the selection), mp3s_hide_message one call at a time, nothing overlapped"}
        del r
        # the pipe owns its context
        pctx = _lib.Context(dev)
        max_job = len(mp3_in) + (1 << 16)
        # (ii) upload + kernels + download of one batch at a time, device-side span from HIP events
        pipe = _lib.Pipe(pctx, depth=1, max_job_bytes=max_job, scan_threads=1)
        spans = []
        for i in range(24):
            assert pipe.submit([mp3_in], [payload]) is not None
            _t, res = pipe.collect()
            if i >= 4:
                spans.append(pipe.stats()["last_device_span_ms"])
            same = note("bytes: pipe job", bytes(res[0]["data"]) == ref_out) and same
            del res
        st1 = pipe.stats()
        pipe.close()
        same = note("path: 24 pipe jobs final after the first pass", st1["fast"] == 24) and same
        regions["h2d_kernels_d2h"] = {"ms_per_batch": round(float(np.mean(spans)), 4), "frames_per_s": round(n / (float(np.mean(spans)) * 1e-3), 1),
                                      "batches": len(spans),
                                      "what": "one batch at a time from page-locked staging: first uploaded byte to last downloaded byte (HIP events)",
                                      "host_scan_ms_per_batch": round(st1["scan_ms"] / st1["collected"], 4)}
        # (iii) steady state: several batches in flight
        if args.e2e_batches > 0:
            pipe = _lib.Pipe(pctx, depth=args.pipe_depth, max_job_bytes=max_job, scan_threads=args.scan_threads)

            def pump(batches, check_every):
                ok, sub, got = True, 0, 0
                while got < batches:
                    while sub < batches and pipe.submit([mp3_in], [payload]) is not None:
                        sub += 1
                    _t, res = pipe.collect()
                    if got % check_every == 0 or got == batches - 1:
                        ok = ok and same_bytes(res[0]["data"], ref_out)
                    del res
                    got += 1
                return ok
            same = note("bytes: e2e warm-up batches", pump(12, 1)) and same                                   # warm-up: result blocks, pool sizes; every batch compared
            if dist is not None:
                dist.barrier()
            s0 = pipe.stats()
            t0 = time.perf_counter()
            ok = pump(args.e2e_batches, 16)
            t_e2e = time.perf_counter() - t0
            s1 = pipe.stats()
            pipe.close()
            same = note("bytes: e2e batches", ok) and note("path: every e2e batch final after the first pass", (s1["fast"] - s0["fast"]) == args.e2e_batches) and same
            t_max = reduce_max(t_e2e)
            nb = args.e2e_batches
            e2e_steady = {"frames_per_s": round(n * nb * world / t_max, 1), "ms_per_batch": round(t_max / nb * 1e3, 4), "steps": nb,
                          "in_flight": args.pipe_depth, "scan_threads": args.scan_threads,
                          "host_scan_ms_per_batch": round((s1["scan_ms"] - s0["scan_ms"]) / nb, 4),
                          "host_issue_ms_per_batch": round((s1["issue_ms"] - s0["issue_ms"]) / nb, 4),
                          "bytes_in_per_batch": len(mp3_in), "bytes_out_per_batch": len(ref_out),
                          "what": "MP3 bytes -> MP3 bytes with the message hidden, mp3s_pipe_*: host scan (worker threads, into page-locked "
                                  "staging) || hipMemcpyAsync up || kernels || hipMemcpyAsync down; every 16th result compared with the one-shot call"}
        # ---- sustained: the same host-fed steady state for >= 5 s of wall time, with the card's clocks and power beside it
        if args.e2e_batches > 0 and args.sustained_seconds > 0:
            pipe = _lib.Pipe(pctx, depth=args.pipe_depth, max_job_bytes=max_job, scan_threads=args.scan_threads)
            mon = GpuMonitor(ctx.device_pci()).start()
            ok, sub, got = True, 0, 0
            for _ in range(args.pipe_depth):
                if pipe.submit([mp3_in], [payload]) is not None:
                    sub += 1
            if dist is not None:
                dist.barrier()
            stamps = []
            t0 = time.perf_counter()
            t_end = t0 + args.sustained_seconds
            while True:
                _t, res = pipe.collect()
                now = time.perf_counter()
                stamps.append(now)
                if got % 64 == 0:
                    ok = ok and same_bytes(res[0]["data"], ref_out)
                del res
                got += 1
                if now >= t_end:
                    break
                if pipe.submit([mp3_in], [payload]) is not None:
                    sub += 1
            t1 = stamps[-1]
            while pipe.collect() is not None:          # drain (outside the clock)
                pass
            mon.stop()
            pipe.close()
            same = note("bytes: host-fed region", ok) and same
            st = np.asarray(stamps)
            first_n, last_n = int((st <= t0 + 1.0).sum()), int((st > t1 - 1.0).sum())
            t_sus = reduce_max(t1 - t0)
            sustained = {"seconds": round(t_sus, 3), "batches": got, "frames_per_s": round(n * got * world / t_sus, 1), "ms_per_batch": round(t_sus / got * 1e3, 4),
                         "frames_per_s_first_second": round(n * first_n * world / 1.0, 1), "frames_per_s_last_second": round(n * last_n * world / 1.0, 1),
                         "last_over_first": round(last_n / max(first_n, 1), 4),
                         "device": mon.summary(t0, t1),
                         "what": "e2e_steady kept up for --sustained-seconds of wall time (MP3 bytes -> MP3 bytes through mp3s_pipe_*, every 64th result compared); "
                                 "clocks / power / busy from sysfs of the card, sampled every 0.2 s by a thread that makes no GPU call"}
        # config 2 host-fed: MP3 bytes -> WAV bytes (46 MB of int16 PCM down per batch), steady state
        if args.e2e_batches > 0:
            wav_ref = bytes(ctx.decode_file(mp3_in)["data"])
            pipe = _lib.Pipe(pctx, depth=args.pipe_depth, max_job_bytes=max_job, scan_threads=args.scan_threads)
            nbd = max(40, args.e2e_batches // 4)

            def pump_dec(batches, check_every):
                ok, sub, got = True, 0, 0
                while got < batches:
                    while sub < batches and pipe.submit_decode([mp3_in]) is not None:
                        sub += 1
                    _t, res = pipe.collect()
                    if got % check_every == 0 or got == batches - 1:
                        ok = ok and same_bytes(res[0]["data"], wav_ref)
                    del res
                    got += 1
                return ok
            same = note("bytes: decode_steady warm-up", pump_dec(8, 1)) and same
            t0 = time.perf_counter()
            ok = pump_dec(nbd, 64)
            t_dec_steady = reduce_max(time.perf_counter() - t0)
            sd = pipe.stats()
            pipe.close()
            same = note("bytes: decode_steady batches", ok) and note("path: no decode job through the host parser", sd["slow"] == 0) and same
            regions["decode_steady"] = {"frames_per_s": round(n * nbd * world / t_dec_steady, 1), "ms_per_batch": round(t_dec_steady / nbd * 1e3, 4), "batches": nbd,
                                        "pcm_mb_down_per_batch": round(n * 2304 * 2 / 1e6, 1), "pcie_gbs_down": round(n * 2304 * 2 * nbd / t_dec_steady / 1e9, 1),
                                        "what": "BASELINE configs[1] host-fed: MP3 bytes -> WAV bytes (int16) through mp3s_pipe_submit_decode, several batches in "
                                                "flight; the download of one batch's PCM runs under the kernels of the next"}
        # the long message through the pipe: every job's verdict says "guess failed" and the host resolves the chains on
        # the job's own device buffers at collect time (scan, decode and transforms are not redone)
        if args.e2e_batches > 0:
            pipe = _lib.Pipe(pctx, depth=args.pipe_depth, max_job_bytes=max_job, scan_threads=args.scan_threads)
            nbl = max(20, args.e2e_batches // 8)
            ok, sub, got = True, 0, 0
            t0 = None
            while got < nbl + 4:
                while sub < nbl + 4 and pipe.submit([mp3_in], [long_text]) is not None:
                    sub += 1
                _t, res = pipe.collect()
                if got % 8 == 0 or got == nbl + 3:
                    ok = ok and same_bytes(res[0]["data"], long_ref)
                del res
                got += 1
                if got == 4:
                    t0 = time.perf_counter()
            t_ls = reduce_max(time.perf_counter() - t0)
            sl = pipe.stats()
            pipe.close()
            same = note("bytes: host-fed region", ok) and same
            long_message["steady"] = {"ms_per_batch": round(t_ls / nbl * 1e3, 4), "frames_per_s": round(n * nbl * world / t_ls, 1), "batches": nbl,
                                      "resolved": sl["resolved"], "synchronous": sl["slow"],
                                      "what": "the same message through mp3s_pipe_*: decided on the device in the overlapped stages (resolved = jobs that still needed the host at collect time)"}
        pctx.close()
        # many short files: the stream cut into 40-frame files, one device batch vs one call per file
        if not args.no_short_files:
            fs = parsed["frame_size"].astype(np.int64)
            cuts = np.concatenate([[0], np.cumsum(fs)])
            shorts = [mp3_in[int(cuts[a]):int(cuts[min(a + 40, n)])] for a in range(0, n, 40)]
            notes = ["note %d" % i for i in range(len(shorts))]
            _ = ctx.hide_messages(shorts, notes)
            t_b0 = time.time()
            batch_out = ctx.hide_messages(shorts, notes)
            t_batch = time.time() - t_b0
            t_l0 = time.time()
            loop_out = [ctx.hide_message(f, m) for f, m in zip(shorts, notes)]
            t_loop = time.time() - t_l0
            same = note("bytes: short files, batch against loop", all(not isinstance(b, Exception) and b["data"] == l["data"] for b, l in zip(batch_out, loop_out))) and same
            short_files = {"files": len(shorts), "frames_each": 40, "hide_messages_one_batch_s": round(t_batch, 4),
                           "hide_message_per_file_loop_s": round(t_loop, 4), "batch_files_per_s": round(len(shorts) / t_batch, 1)}
    # ---------------------------------------------------------------- BASELINE configs[4]: the mixed corpus
    config5 = None
    if not args.resident_only and not args.no_config5 and rank == 0 and world == 1:
        config5, ok5 = run_config5(octx if octx is not None else ctx, _lib, O, synth_pcm, min(n, 10000))
        same = note("bytes: config 5", ok5) and same
    # ---------------------------------------------------------------- the ranks of one host side by side
    hosts = gather_rank_hosts(dist, world, rank_host_record(rank, args.scan_threads, e2e_steady, ctx.host_share))
    same = reduce_all_ok(note("bytes: oracle on the first 64 frames", oracle_ok) and same)

    # ---------------------------------------------------------------- rooflines of the dominant kernel
    # duration of the dominant kernel per batch, from the event pairs of the TIMED region
    dom_ms_launch = prof[dom][0] / max(prof[dom][1], 1)
    achieved = B_PIPE * n / (dom_ms_launch * 1e-3) / 1e9
    traffic, traffic_source = None, None
    if pmc_live and dom in pmc_live and "hbm_bytes" in pmc_live[dom]:
        traffic, traffic_source = round(pmc_live[dom]["hbm_bytes"]), pmc_note
    tj = os.path.join(ROOT, "profiles", "traffic_latest.json")
    if traffic is None and os.path.exists(tj):
        traffic_source = "profiles/traffic_latest.json (committed; live measurement: %s)" % pmc_note
        try:
            tr = json.load(open(tj))
            # PMC bytes per launch (2 x FETCH_SIZE + WRITE_SIZE, separate rocprofv3 --pmc passes) measured on the
            # `frames` batch recorded in the file; scaled to this run's batch
            traffic = tr.get(dom)
            if traffic is not None:
                traffic = round(traffic * n / tr.get("frames", 10000))
        except Exception:
            traffic = None
    copy_gbs = None
    try:
        copy_gbs = round(ctx.bench_copy(1 << 30, 20), 1)
    except Exception:
        copy_gbs = None
    roofline = {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic, "traffic_source": traffic_source,
                "algorithmic_bytes_per_launch": B_PIPE * n, "kernel_ms_per_launch": round(dom_ms_launch, 4),
                "copy_kernel_gbs": copy_gbs,
                "hbm_bytes_per_launch_by_kernel": ({k: round(v["hbm_bytes"]) for k, v in sorted(pmc_live.items()) if k.startswith("k_") and k != "k_copy16" and "hbm_bytes" in v}
                                                   if pmc_live else None),
                "note": "fixed-size fp64/int32 transforms in the reference's exact operation order are ALU-bound, "
                        "not HBM-bound (see DESIGN.md and roofline_alu); frac is reported as the contract defines it; "
                        "copy_kernel_gbs = what a plain device copy achieves on this device (read + write)"}
    step_hbm_bytes = sum(roofline["hbm_bytes_per_launch_by_kernel"].values()) if roofline["hbm_bytes_per_launch_by_kernel"] else None
    # what actually binds: VALU issue.  Wave instructions of the dominant kernel per launch from the committed PMC summary
    # (SQ_INSTS_VALU, same passes as `traffic`), against the rate the SIMDs can issue them at
    roofline_alu = None
    pj = os.path.join(ROOT, "profiles", "pmc_latest.json")
    if (pmc_live and dom in pmc_live and "SQ_INSTS_VALU" in pmc_live[dom]) or os.path.exists(pj):
        try:
            if pmc_live and dom in pmc_live and "SQ_INSTS_VALU" in pmc_live[dom]:
                pm = dict(pmc_live, frames=n, source=pmc_note)
            else:
                pm = json.load(open(pj))
            insts = pm[dom]["SQ_INSTS_VALU"] * n / pm.get("frames", 10000)
            peak = N_SIMD * CLOCK_GHZ / CLK_PER_VALU                      # G wave-instructions / s
            ach = insts / (dom_ms_launch * 1e-3) / 1e9
            roofline_alu = {"bound": "valu_issue", "kernel": dom, "achieved": round(ach, 2), "peak": round(peak, 1),
                            "unit": "G wave-instructions/s", "frac": round(ach / peak, 4),
                            "valu_wave_instructions_per_launch": round(insts), "salu_wave_instructions_per_launch":
                            round(pm[dom].get("SQ_INSTS_SALU", 0) * n / pm.get("frames", 10000)),
                            "waves_per_launch": round(pm[dom].get("SQ_WAVES", 0) * n / pm.get("frames", 10000)),
                            "peak_is": f"{N_SIMD} SIMDs x {CLOCK_GHZ} GHz / {CLK_PER_VALU} clk per wave instruction (fp64 and 32-bit "
                                       "multiplies issue at >= 4 clk per wave64 on a SIMD-32: tools/ubench/valu_rates.hip measures 4.5)",
                            "pmc_source": pm.get("source", "profiles/pmc_latest.json"),
                            # the same achieved rate against the three peaks one can argue for, side by side: the guide's 2 clocks per wave
                            # instruction (MI355X_MICROARCH.md), the flat 4 clocks above, and the kernel's own mix below
                            "frac_at_2_clk": round(ach / (N_SIMD * CLOCK_GHZ / 2.0), 4), "frac_at_4_clk": round(ach / peak, 4)}
            # ... and against the rate its OWN instruction mix can issue at: the listing's vector instructions by class (tools/kernel_mix.py)
            # times the measured cost of each class (tools/ubench/issue_rates.hip: plain 32-bit VOP1/VOP2 1.2 ns per wave instruction and SIMD,
            # VOP3 / DPP / compares / multiplies / fp64 1.9, v_mad_u64_u32 2.3, lane reads 2.4 -- five waves per SIMD, whatever the clock was)
            try:
                rates = json.load(open(os.path.join(ROOT, "profiles", "r05_issue_rates.json")))
                mix = json.load(open(os.path.join(ROOT, "profiles", "r06_kernel_mix.json")))[dom]
                ns = {"full": rates["v_add_u32"]["ns_5"], "half": rates["v_bfe_u32"]["ns_5"], "mad64": rates["v_mad_u64_u32"]["ns_5"], "lane": rates["v_readlane_b32"]["ns_5"]}
                mean_ns = sum(mix.get(c, 0) * ns[c] for c in ns) / max(1, sum(mix.get(c, 0) for c in ns))
                peak_mix = N_SIMD / mean_ns                                   # G wave-instructions / s
                roofline_alu.update({"peak_of_its_mix": round(peak_mix, 1), "frac_of_its_mix": round(ach / peak_mix, 4),
                                     "mix": {c: mix.get(c, 0) for c in ns}, "ns_per_wave_instruction_by_class": {c: round(v, 3) for c, v in ns.items()},
                                     "mean_ns_per_wave_instruction": round(mean_ns, 3),
                                     "mix_source": "profiles/r06_kernel_mix.json (the LISTING's instructions by class, not executed counts: the counters of this chip "
                                                   "count vector instructions by data type, not by encoding -- see valu_by_type -- so the mix-weighted "
                                                   "peak is an estimate that brackets between frac_at_4_clk and 1) x profiles/r05_issue_rates.json (measured)"})
                bytype = {k[len("SQ_INSTS_VALU_"):]: round(v * n / pm.get("frames", 10000)) for k, v in pm[dom].items() if k.startswith("SQ_INSTS_VALU_")}
                if bytype:
                    roofline_alu["valu_by_type"] = bytype            # EXECUTED wave instructions per launch by the hardware's own classes
            except Exception:
                pass
        except Exception:
            roofline_alu = None

    # ---------------------------------------------------------------- CPU baseline (oracle = port), rank 0, N = 1
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        m = min(args.cpu_frames, n)
        sub = mp3_in[:int(parsed["frame_size"][:m].sum())]
        t0 = time.perf_counter()
        passes, done = 0, 0
        while passes == 0 or time.perf_counter() - t0 < args.cpu_seconds:
            od = O.decode(sub)
            op = O.pcm_to_i16(od["pcm"])
            oe = O.encode(op, 44100, 128, hide)
            assert oe["rc"] == 0
            passes += 1
            done += od["n_frames"]
        dt = time.perf_counter() - t0
        cpu = {"value": round(done / dt, 1), "unit": "frames/s", "cores": 1, "kind": "port",
               "sample": f"{passes} pass(es) over the first {od['n_frames']} frames of the same stream: oracle decode (incl. "
                         f"Huffman) + int16 PCM + oracle encode (incl. bit packing), single thread, {dt:.1f} s",
               "host_cpus": os.cpu_count()}
        # the same port on all host cores -- a child process (this one holds a GPU context and must not
        # fork) that forks one worker per core, each looping over its own 400-frame cut of the stream
        if args.cpu_seconds_all > 0 and n > 400:
            import subprocess
            import tempfile
            # optional extra: whatever goes wrong in the child (timeout, a box that cannot fork that many workers) must
            # not cost the bench line, whose timed region is already over
            r = None
            try:
                with tempfile.TemporaryDirectory() as td:
                    open(os.path.join(td, "s.mp3"), "wb").write(mp3_in)
                    np.save(os.path.join(td, "h.npy"), np.asarray(hide, dtype=np.uint8))
                    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cpu_all_cores.py"), os.path.join(td, "s.mp3"),
                                        os.path.join(td, "h.npy"), str(args.cpu_seconds_all)], capture_output=True, text=True, timeout=300)
                cpu["all_cores"] = json.loads(r.stdout.strip().splitlines()[-1])
                cpu["all_cores"]["x_one_thread"] = round(cpu["all_cores"]["value"] / cpu["value"], 1)
            except Exception as e:                                   # noqa: BLE001
                tail = ((r.stderr or r.stdout) if r is not None else "")[-300:]
                cpu["all_cores"] = {"error": f"{type(e).__name__}: {e}"[:200], "child_output": tail}

    if rank == 0:
        out = {
            "metric": METRIC, "value": round(value, 1), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(max_step * 1e3, 4), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f64 (decode) / int32 (encode)", "data": "synthetic",
            "config": dict(config, pipeline_rate_passes=int(final["rate_passes"]), parallelism=f"frames sharded over {world} GPU(s), no collective"),
            "full": True, "timed_regions": len(walls), "value_min": round(value_min, 1), "value_max": round(value_max, 1), "value_regions": value_regions,
            "value_spread": round((value_max - value_min) / value, 4),
            # the evidence the nested objects below hold, once more as scalars (a reader that keeps scalars only sees them)
            "sustained_frames_per_s": sustained["frames_per_s"] if sustained else None,
            "e2e_steady_frames_per_s": e2e_steady["frames_per_s"] if e2e_steady else None,
            "cpu_all_cores_frames_per_s": (cpu or {}).get("all_cores", {}).get("value") if cpu else None,
            "cpu_all_cores": (cpu or {}).get("all_cores", {}).get("cores") if cpu else None,
            "step_hbm_bytes": step_hbm_bytes,
            "decode_only_float32_exact_ms": decode_only["ms_per_step"] if decode_only else None,
            "decode_only_float32_fast_ms": decode_only["float_fast"]["ms_per_step"] if decode_only and "float_fast" in decode_only else None,
            "decode_only_int16_ms": decode_only["int16"]["ms_per_step"] if decode_only and "int16" in decode_only else None,
            "facade_ms_per_file": (regions or {}).get("single_file_10k", {}).get("facade_ms_per_file") if regions else None,
            "facade_new_file_ms": (regions or {}).get("single_file_10k", {}).get("facade_new_file_ms") if regions else None,
            "c_call_ms_per_file": (regions or {}).get("single_file_10k", {}).get("ms_per_batch") if regions else None,
            "first_call_ms": (regions or {}).get("single_file_10k", {}).get("first_call", {}).get("ms") if regions else None,
            "dominant_kernel_ms": round(dom_ms_launch, 4),
            "sustained": sustained,
            "roofline": roofline,
            "roofline_alu": roofline_alu,
            "cpu_baseline": cpu,
            "e2e_steady": e2e_steady,
            "decode_only": decode_only,
            "value_four_streams": four,
            "regions": regions,
            "long_message": long_message,
            "kernels_ms_per_step": {k: round(v, 4) for k, v in per_step.items()},
            "kernels_ms_note": f"event pairs around every kernel, separate untimed pass of {n_prof} steps; the timed region "
                               f"carries them around the dominant kernel only, on every {max(1, args.dom_events_every)}. step "
                               "(all kernels: about 0.05 ms per step).  The rate loop's pair is the dispatch's own start and stop event "
                               "(hipExtLaunchKernelGGL): the kernel's time stamps, no record packets around it -- it agrees with rocprofv3's kernel trace",
            "dominant_kernel_launches_timed": int(prof[dom][1]),
            "hot_path_value": round(n * world / (sum(v for k, v in per_step.items()
                                                       if k not in ("k_dec_huffman", "k_enc_pack")) * 1e-3), 1),
            "gpu_event_ms_per_step": round(gpu_ms / args.steps, 4),
            "timed_region_s": round(wall, 4),
            "front_end_overlap": front_end_overlap, "tail_stream": tail_stream,
            "parity_checked": bool(same), "parity_failures": parity_failures,
            "short_files": short_files,
            "config5": config5,
            "ranks_on_this_host": hosts,
            "prep_s": round(prep_s, 2),
            "device": ctx.device_name(),
        }
        print(json.dumps(out))
    for c in (aux, aux2, dctx, octx):
        if c is not None:
            c.close()
    ctx.close()
    if dist is not None:
        dist.destroy_process_group()
    if not same:
        sys.exit(3)


if __name__ == "__main__":
    main()
