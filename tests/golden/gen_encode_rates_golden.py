#!/usr/bin/env python3
"""Golden for whole encodes away from 44.1 kHz / 128 and 320 kbit/s: the upstream reference's encoder on eight-frame streams at 48 kHz
and 32 kHz (32, 128, 320 kbit/s) and at 44.1 kHz with 32 and 64 kbit/s (padding changes from frame to frame there), every second one with
a short message, and its decoder on every MP3 it wrote; one long 44.1 kHz / 128 kbit/s stream whose message of more than 1024 bits ends
two frames before the stream does.  Runs the reference (build container only, refshim.py) through encode_instrumented and
decode_instrumented of gen_golden.py; the long case's frame count comes from the oracle's cursor, so the build must have been run.

    python tests/golden/gen_encode_rates_golden.py      ->  tests/golden/g13_encode_rates.npz

The PCM is tests/synth_pcm.py's with frames 3-4 set to zero and channel 0 of frame 6 at 32767 (case_pcm); the fixture keeps its seed and
sha256, tests/test_reference_rates.py makes it again."""
import concurrent.futures
import hashlib
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

from synth_pcm import synth_pcm  # noqa: E402

OUT = os.path.join(HERE, "g13_encode_rates.npz")
FRAMES, HEAD = 8, 2
TEXTS = ("rates", "48k", "pad?", "lo")
# (sampling rate, kbit/s): every second case carries "<n>#<text>"
CASES = [(48000, 32), (48000, 128), (48000, 320), (32000, 32), (32000, 128), (32000, 320), (44100, 32), (44100, 64)]
LONG = (44100, 128)
LONG_TEXT = "".join(chr(97 + (7 * i) % 26) if i % 9 else " " for i in range(140))          # 144 bytes framed: 1152 bits
LONG_SPARE = 2                                                                             # frames behind the one the message ends in


def case_name(rate, kbps):
    return "r%d_k%d" % (rate, kbps)


def case_seed(rate, kbps):
    return 0x5EED0000 + rate + kbps


def case_text(i):
    return TEXTS[i // 2] if i % 2 else None


def case_pcm(rate, kbps):
    pcm = synth_pcm(FRAMES, rate=rate, seed=case_seed(rate, kbps))
    pcm[3 * 1152:5 * 1152] = 0                                      # a silent stretch: empty units, inherited addresses
    pcm[6 * 1152:7 * 1152, 0] = 32767                               # a clipped burst: the quantiser's float path
    return pcm


def long_pcm(n):
    return synth_pcm(n, rate=LONG[0], seed=case_seed(*LONG))


def framed(text):
    """the bits the reference's facade hides for `text` (steganography.py:46-47)"""
    return np.frombuffer("".join(format(b, "08b") for b in ("%d#%s" % (len(text), text)).encode()).encode(), dtype=np.uint8) - ord("0")


def sha(b):
    return np.frombuffer(hashlib.sha256(bytes(b)).hexdigest().encode(), dtype=np.uint8)


def _run(job):
    """one case in a process of its own: -> {key: array}"""
    name, rate, kbps, text, n_long = job
    import gen_golden as G                                          # (imports the reference)
    import oracle_lib
    t0 = time.time()
    pcm = long_pcm(n_long) if n_long else case_pcm(rate, kbps)
    out = {"rate": np.int32(rate), "kbps": np.int32(kbps), "seed": np.int64(case_seed(rate, kbps)), "n_frames": np.int32(len(pcm) // 1152),
           "pcm_sha256": sha(np.ascontiguousarray(pcm, dtype="<i2").tobytes()), "text": np.array(text or "")}
    with tempfile.TemporaryDirectory() as td:
        wav, mp3p = os.path.join(td, "in.wav"), os.path.join(td, "out.mp3")
        with open(wav, "wb") as f:
            f.write(oracle_lib.wav_bytes(pcm, rate))
        hide = "".join(str(int(b)) for b in framed(text)) if text else ""
        assert not text or hide == G.str_to_binary_str("%d#%s" % (len(text), text))
        enc, mp3 = G.encode_instrumented(wav, mp3p, kbps, hide, keep_frames=HEAD)
        out["mp3"] = np.frombuffer(mp3, dtype=np.uint8)
        if n_long:
            keep = ("hide_off", "too_long")
        else:
            keep = ("gi", "table_select", "scfsi", "written", "hide_off", "padding", "too_long", "mdct_freq", "ix", "gi_fields")
            dec, _ = G.decode_instrumented(mp3p, os.path.join(td, "back.wav"), keep_pcm_frames=1)
            out["dec_bits"], out["dec_pcm_sha256"], out["dec_pcm_i16_sha256"] = dec["bits"], dec["pcm_sha256"], dec["pcm_i16_sha256"]
            if text:                                               # the same PCM without a message: what hide_message starts from
                plain = os.path.join(td, "plain.mp3")
                G.REncoder(wav, plain, bitrate=kbps, hide_str="").encode(quiet=True)
                out["plain_mp3"] = np.frombuffer(open(plain, "rb").read(), dtype=np.uint8)
        for k in keep:
            out[k] = enc[k]
    print("%-12s frames %3d  bytes %6d  cursor %4d  too_long %d  %.0fs" % (name, int(out["n_frames"]), len(mp3), int(enc["hide_off"][-1]),
                                                                         int(enc["too_long"]), time.time() - t0), flush=True)
    return {name + "__" + k: v for k, v in out.items()}


def long_frames():
    """the smallest stream in which LONG_TEXT ends, by the oracle's cursor, and LONG_SPARE frames more"""
    import oracle_lib
    bits = framed(LONG_TEXT)
    assert len(bits) > 1024
    o = oracle_lib.encode(long_pcm(160), LONG[0], LONG[1], bits)
    assert o["rc"] == 0 and o["hide_offset"] >= len(bits)
    fits = int(np.argmax(o["frames"]["hide_off"] >= len(bits))) + 1
    return fits + LONG_SPARE


def main():
    from gen_rate_units_golden import save_npz
    t0 = time.time()
    n_long = long_frames()
    jobs = [("long", LONG[0], LONG[1], LONG_TEXT, n_long)]          # the longest first
    jobs += [(case_name(r, k), r, k, case_text(i), 0) for i, (r, k) in enumerate(CASES)]
    workers = max(1, min(int(os.environ.get("MP3S_GEN_JOBS", "8")), os.cpu_count() or 1))
    with concurrent.futures.ProcessPoolExecutor(workers, multiprocessing.get_context("spawn")) as pool:
        parts = list(pool.map(_run, jobs))
    out = {"names": np.array([j[0] for j in jobs[1:]]), "long_frames": np.int32(n_long)}
    for p in parts[1:] + parts[:1]:
        out.update(p)
    save_npz(OUT, out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes in %.0fs" % (time.time() - t0))


if __name__ == "__main__":
    main()
