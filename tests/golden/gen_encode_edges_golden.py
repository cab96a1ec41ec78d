#!/usr/bin/env python3
"""Golden for the encode transform where its int32 arithmetic wraps: the upstream reference's encoder on every stream of
tests/encode_edges.py, each alone, at 128 kbit/s, and six of them at 32 kbit/s as well.  Runs the reference (build container only,
refshim.py) through encode_instrumented of gen_golden.py; nothing of it is copied.

    python tests/golden/gen_encode_edges_golden.py      ->  tests/golden/g17_encode_edges.npz

Per run (stream, bit rate): a sha256 of every frame's __mdct_freq, every GrInfo field, table_select, scfsi, the frame sizes, hide_off and
padding of every frame, a sha256 of ix and of the MP3, the MP3's length.  Per stream: a sha256 of the PCM, and the whole __mdct_freq of the
frames in which the model of tests/encode_edges.py reports a value outside int32 (a failing test can then name the line).  Where the
reference raises -- its rate loop does, on a step outside steptab -- the run records the exception's type name and the frame, nothing of
the frames behind it, and the stream's __mdct_freq comes from a second pass in which __iteration_loop and __format_bitstream do nothing:
__mdct_sub is the reference's own either way.  The runs of a stream must agree on __mdct_freq (the transform reads neither rate).  Runs go
through parallel processes."""
import concurrent.futures
import multiprocessing
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (HERE, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import encode_edges as E  # noqa: E402
from gen_decode_edges_golden import save_npz, SIZE_LIMIT  # noqa: E402

OUT = os.path.join(HERE, "g17_encode_edges.npz")


def _encode(G, wav, mp3p, kbps):
    """encode_instrumented with a count of the frames that were finished -> (records or None, mp3, exception's name, frame it rose in)"""
    RE = G.RE
    inner = RE.MP3Encoder._MP3Encoder__encode_buffer_internal
    done = [0]

    def counted(self):
        r = inner(self)
        done[0] += 1
        return r

    RE.MP3Encoder._MP3Encoder__encode_buffer_internal = counted
    try:
        enc, mp3 = G.encode_instrumented(wav, mp3p, kbps, "")
        return enc, mp3, "", -1
    except Exception as e:                                              # noqa: BLE001 -- what the reference raises is what is recorded
        return None, b"", type(e).__name__, done[0]
    finally:
        RE.MP3Encoder._MP3Encoder__encode_buffer_internal = inner


def _transform_only(G, wav, mp3p, kbps):
    """__mdct_freq of every frame with the rate loop and the bit stream writer switched off"""
    M = G.RE.MP3Encoder
    saved = M._MP3Encoder__iteration_loop, M._MP3Encoder__format_bitstream
    M._MP3Encoder__iteration_loop = M._MP3Encoder__format_bitstream = lambda self: None
    try:
        return G.encode_instrumented(wav, mp3p, kbps, "")[0]["mdct_freq"]
    finally:
        M._MP3Encoder__iteration_loop, M._MP3Encoder__format_bitstream = saved


def _run(job):
    name, kbps = job
    import gen_golden as G                                              # (imports the reference)
    import oracle_lib
    t0 = time.time()
    s = E.streams()[name]
    with tempfile.TemporaryDirectory() as td:
        wav, mp3p = os.path.join(td, "in.wav"), os.path.join(td, "out.mp3")
        with open(wav, "wb") as f:
            f.write(oracle_lib.wav_bytes(s.pcm, s.rate))
        enc, mp3, err, at = _encode(G, wav, mp3p, kbps)
        mdct = enc["mdct_freq"] if enc is not None else _transform_only(G, wav, mp3p, kbps)
    assert mdct.shape == (E.FRAMES, 2, 2, 576) and mdct.dtype == np.int32
    out = {"mdct": mdct, "raises": err, "raises_at": at}
    if enc is not None:
        assert list(G.GI_FIELDS) == bytes(enc["gi_fields"]).decode().split(",")
        out.update({k: enc[k] for k in ("gi", "table_select", "scfsi", "written", "hide_off", "padding")})
        out["ix_sha256"] = E.sha256(np.ascontiguousarray(enc["ix"], dtype="<i2").tobytes())
        out["mp3_sha256"], out["mp3_len"] = E.sha256(mp3), len(mp3)
    print("%-20s %3d kbit/s  %s  %.0fs" % (name, kbps, "raises %s in frame %d" % (err, at) if err else "%d bytes" % len(mp3), time.time() - t0), flush=True)
    return out, list(G.GI_FIELDS)


def main():
    t0 = time.time()
    S, runs = E.streams(), E.runs()
    names = list(S)
    procs = max(1, min(int(os.environ.get("MP3S_GEN_JOBS", "8")), os.cpu_count() or 1))
    with concurrent.futures.ProcessPoolExecutor(procs, multiprocessing.get_context("spawn")) as pool:
        res = list(pool.map(_run, runs))
    fields = res[0][1]
    n, F = len(runs), E.FRAMES
    out = {"names": np.array(names), "rate": np.array([S[k].rate for k in names], dtype=np.int32),
           "pcm_sha256": np.stack([E.sha256(np.ascontiguousarray(S[k].pcm, dtype="<i2").tobytes()) for k in names]),
           "run_stream": np.array([names.index(k) for k, _ in runs], dtype=np.int32), "run_kbps": np.array([b for _, b in runs], dtype=np.int32),
           "raises": np.array([r["raises"] for r, _ in res]), "raises_at": np.array([r["raises_at"] for r, _ in res], dtype=np.int32),
           "mdct_sha256": np.stack([np.stack([E.sha256(np.ascontiguousarray(f, dtype="<i4").tobytes()) for f in r["mdct"]]) for r, _ in res]),
           "gi_fields": np.array(fields),
           "gi": np.zeros((n, F, 2, 2, len(fields)), dtype=np.int32), "table_select": np.zeros((n, F, 2, 2, 3), dtype=np.int32),
           "scfsi": np.zeros((n, F, 2, 4), dtype=np.int32), "written": np.zeros((n, F), dtype=np.int32), "hide_off": np.zeros((n, F), dtype=np.int32),
           "padding": np.zeros((n, F), dtype=np.int32), "ix_sha256": np.zeros((n, 32), dtype=np.uint8), "mp3_sha256": np.zeros((n, 32), dtype=np.uint8),
           "mp3_len": np.zeros(n, dtype=np.int64)}
    first = {}
    for i, ((name, _), (r, _)) in enumerate(zip(runs, res)):
        if name in first:
            assert np.array_equal(r["mdct"], res[first[name]][0]["mdct"]), "%s: __mdct_freq depends on the bit rate" % name
        first.setdefault(name, i)
        if not r["raises"]:
            for k in ("gi", "table_select", "scfsi", "written", "hide_off", "padding", "ix_sha256", "mp3_sha256", "mp3_len"):
                out[k][i] = r[k]
    full, where = [], []
    for si, name in enumerate(names):                                   # the frames the model flags, whole
        m = E.stream_model(name)
        for f in range(F):
            if m["sum_out"][f].any() or m["bfly_out"][f].any():
                full.append(res[first[name]][0]["mdct"][f])
                where.append((si, f))
    out["mdct_full"], out["mdct_full_at"] = np.stack(full), np.array(where, dtype=np.int32)
    save_npz(OUT, out)
    size = os.path.getsize(OUT)
    assert size <= SIZE_LIMIT, size
    print("wrote", OUT, size, "bytes: %d streams, %d runs (%d raise), %d whole frames in %.0fs with %d processes" % (
        len(names), n, sum(1 for r, _ in res if r["raises"]), len(full), time.time() - t0, procs))


if __name__ == "__main__":
    main()
