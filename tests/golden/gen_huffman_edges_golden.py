#!/usr/bin/env python3
"""Golden for the Huffman / scalefactor decode at its bit-stream edges: the upstream reference's own side-info parser, __unpack_scale_fac
and __unpack_samples (decoder/Frame.py:318-559) over every stream of tests/huffman_edges.py.  Runs the reference (build container only,
refshim.py); nothing of it is copied: it is imported, and its functions are called.

    python tests/golden/gen_huffman_edges_golden.py      ->  tests/golden/g16_huffman_edges.npz

A Frame object is driven as MP3Parser drives it (MP3_Parser.py:36-80), but stops behind __set_main_data: init_header_params,
set_frame_size, side_info.set_side_info, _Frame__set_main_data.  Per stream the fixture holds a digest of the builder's bytes, the
int16 spectra [frames][2][2][576], scale_fac_l / scale_fac_s as the reference's arrays hold them behind each frame, and -- where the
reference raises -- the exception's type name and the frame at which it raises (the frames in front of it are recorded).  For the streams
the builder marks, a second Frame object runs the full init_frame_params: per frame a 64-bit blake2b of the float64 PCM bytes.  The
reference's code books are probed with an all-zeros and an all-ones window: `probe_nomatch` lists the (book, window) pairs that no entry
matches.  Streams run in parallel processes."""
import concurrent.futures
import multiprocessing
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (HERE, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import huffman_edges as H  # noqa: E402
from gen_decode_edges_golden import save_npz, SIZE_LIMIT  # noqa: E402

OUT = os.path.join(HERE, "g16_huffman_edges.npz")

_RF = None


def _init():
    global _RF
    from refshim import load_reference
    load_reference()
    from mp3stego.decoder import Frame as RF
    _RF = RF


def _walk(data, full):
    """the parser's loop; full: init_frame_params (PCM), else stop behind __set_main_data"""
    RF = _RF
    file_data = list(data)
    fr = RF.Frame()
    assert file_data[0] == 0xFF and file_data[1] >= 0xE0
    fr.init_header_params(file_data)                                   # MP3_Parser.py:41-42
    fr.set_frame_size()
    offset, out = 0, []
    err = ("", -1)
    while len(file_data) > offset + 4:
        buffer = file_data[offset:]
        assert buffer[0] == 0xFF and buffer[1] >= 0xE0
        fr.init_header_params(buffer)
        try:
            if full:
                fr.init_frame_params(buffer, file_data, offset)
                out.append(np.array(fr.pcm, dtype=np.float64))
            else:
                fr._Frame__buffer = buffer
                fr.set_frame_size()
                hdr = fr._Frame__header
                fr.side_info.set_side_info(buffer[6 if hdr.crc == 0 else 4:], hdr)
                fr._Frame__set_main_data(file_data, offset)
                smp = np.array(fr._Frame__samples)
                assert (smp == np.round(smp)).all() and np.abs(smp).max() <= H.VALUE_MAX
                out.append((smp.astype(np.int16), np.array(fr.side_info.scale_fac_l).astype(np.uint8), np.array(fr.side_info.scale_fac_s).astype(np.uint8)))
        except Exception as e:                                          # noqa: BLE001 -- what the reference raises is what is recorded
            err = (type(e).__name__, len(out))
            break
        offset += fr.frame_size
    return out, err


def _run(name):
    s = H.streams()[name]
    rows, err = _walk(s.data, False)
    pcm = None
    if s.pcm:
        frames, err2 = _walk(s.data, True)
        assert err2 == err
        pcm = H.frame_digests(np.concatenate(frames, axis=0)) if frames else np.zeros(0, dtype=np.uint64)
    return name, rows, err, pcm


def probe_books():
    """every big-value book and count1 book A of the reference against an all-zeros and an all-ones 32-bit window -> the (book, window) without a match"""
    from mp3stego.decoder import tables as T
    miss = []
    for t in (t for t in range(32) if t not in (0, 4, 14)):            # (those three are never searched)
        n = int(T.big_value_max[t])
        tab = T.big_value_table[t]
        for wi, window in enumerate((0, 0xFFFFFFFF)):
            hit = any(int(tab[2 * (n * r + c)]) >> (32 - int(tab[2 * (n * r + c) + 1])) == window >> (32 - int(tab[2 * (n * r + c) + 1]))
                      for r in range(n) for c in range(n))
            if n and not hit:
                miss.append((t, wi))
    for wi, window in enumerate((0, 0xFFFFFFFF)):
        if not any(int(T.quad_table_1.h_cod[e]) >> (32 - int(T.quad_table_1.h_len[e])) == window >> (32 - int(T.quad_table_1.h_len[e])) for e in range(16)):
            miss.append((32, wi))
    return miss


def main():
    t0 = time.time()
    S = H.streams()
    names = list(S)
    procs = max(1, min(int(os.environ.get("MP3S_GEN_JOBS", "8")), os.cpu_count() or 1))
    with concurrent.futures.ProcessPoolExecutor(procs, multiprocessing.get_context("spawn"), _init) as pool:
        res = {r[0]: r for r in pool.map(_run, names, chunksize=4)}
    _init()
    miss = probe_books()
    print("books without a match for a window (book, 0 = zeros | 1 = ones):", miss)
    assert sorted(miss) == sorted(H.PROBE_NOMATCH), "tests/huffman_edges.py PROBE_NOMATCH does not list what the probe finds"
    isv, sfl, sfs, pcm, pcm_of = [], [], [], [], []
    n_done = []
    for n in names:
        _, rows, err, p = res[n]
        n_done.append(len(rows))
        for a, b, c in rows:
            isv.append(a); sfl.append(b); sfs.append(c)
        if p is not None:
            pcm_of.append(n)
            pcm.append(p)
        print("%-44s %d frames%s" % (n, len(rows), "  raises %s at frame %d" % err if err[1] >= 0 else ""))
    out = {"names": np.array(names), "in_digest": np.array([H.input_digest(S[n].data) for n in names], dtype=np.uint64),
           "n_frames": np.array(n_done, dtype=np.int32),                    # frames the reference decoded (all of them unless it raises)
           "raises": np.array([res[n][2][0] for n in names]), "raises_at": np.array([res[n][2][1] for n in names], dtype=np.int32),
           "is": np.stack(isv), "scale_fac_l": np.stack(sfl), "scale_fac_s": np.stack(sfs),
           "pcm_names": np.array(pcm_of), "pcm_frames": np.array([len(p) for p in pcm], dtype=np.int32), "pcm_digest": np.concatenate(pcm),
           "probe_nomatch": np.array(miss, dtype=np.int32).reshape(-1, 2)}
    save_npz(OUT, out)
    size = os.path.getsize(OUT)
    assert size <= SIZE_LIMIT, size
    print("wrote", OUT, size, "bytes: %d streams, %d frames in %.0fs with %d processes" % (len(names), len(isv), time.time() - t0, procs))


if __name__ == "__main__":
    main()
