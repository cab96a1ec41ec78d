#!/usr/bin/env python3
"""Golden for streams whose headers change from frame to frame (tests/vbr_streams.py G10): per-frame VBR over all 14
bit-rate indices, 44.1 -> 48 -> 32 kHz switches, a last frame with a rate and bit rate of its own, reserved rate bits
inside a 48 kHz stream, main_data_begin 511 behind the smallest frames, and a stereo -> mono change (the reference
raises).  The reference parses each frame under its own header (decoder/MP3_Parser.py:66-79) and takes the WAV's rate
and the re-encode bit rate from the last frame (:91, :93-98, steganography.py:137-162).  Runs the upstream reference
(build container only, refshim.py).

    python tests/golden/gen_vbr_golden.py        ->  tests/golden/g10_vbr.npz
"""
import hashlib
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import vbr_streams  # noqa: E402
from refshim import load_reference  # noqa: E402

load_reference()
from mp3stego import Steganography  # noqa: E402
from mp3stego.decoder.decoder import Decoder as RDecoder  # noqa: E402

HEAD_FRAMES = 1


def sha(b):
    return np.frombuffer(hashlib.sha256(b).hexdigest().encode(), dtype=np.uint8)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as td:
        for name in vbr_streams.G10_NAMES:
            t0 = time.time()
            data = vbr_streams.g10_stream(name)
            mp3, wav = os.path.join(td, name + ".mp3"), os.path.join(td, name + ".wav")
            open(mp3, "wb").write(data)
            out[name + "__mp3"] = np.frombuffer(data, dtype=np.uint8)
            try:
                dec = RDecoder(mp3, wav)
                kbps = dec.decode(quiet=True)
            except Exception as e:                                  # noqa: BLE001
                out[name + "__error"] = np.array(type(e).__name__)
                print(name, "raises", type(e).__name__)
                continue
            parser = dec._Decoder__parser
            pcm = np.asarray(parser._MP3Parser__pcm_data, dtype=np.float64)
            wavb = open(wav, "rb").read()
            out[name + "__error"] = np.array("")
            out[name + "__n_frames"] = np.int64(pcm.shape[0] // 1152)
            out[name + "__kbps"] = np.int64(kbps)
            out[name + "__sampling_rate"] = np.int64(int.from_bytes(wavb[24:28], "little"))
            out[name + "__nch"] = np.int64(pcm.shape[1])
            out[name + "__bits"] = np.frombuffer(parser.output_bits.encode(), dtype=np.uint8) - ord("0")
            out[name + "__pcm_sha256"] = sha(np.ascontiguousarray(pcm).tobytes())
            out[name + "__pcm_head"] = pcm[: HEAD_FRAMES * 1152]
            out[name + "__pcm_i16_sha256"] = sha((pcm * 32767).astype(np.int16).tobytes())
            out[name + "__wav_sha256"] = sha(wavb)
            if name in vbr_streams.G10_HIDE:
                hid = os.path.join(td, name + "_hide.mp3")
                too_long = Steganography(quiet=True).hide_message(mp3, hid, vbr_streams.G10_HIDE[name])
                out[name + "__hide_mp3"] = np.frombuffer(open(hid, "rb").read(), dtype=np.uint8)
                out[name + "__hide_too_long"] = np.bool_(bool(too_long))
            print(name, "frames", int(out[name + "__n_frames"]), "kbps", kbps, "rate", int(out[name + "__sampling_rate"]),
                  "hide" if name in vbr_streams.G10_HIDE else "", f"{time.time() - t0:.1f}s", flush=True)
    np.savez_compressed(os.path.join(HERE, "g10_vbr.npz"), **out)


if __name__ == "__main__":
    main()
