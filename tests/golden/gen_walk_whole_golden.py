#!/usr/bin/env python3
"""Golden for the whole-file walk (mp3s_walk_stream): what the library itself answered for tests/golden/test.mp3, for the same
stream cut inside a frame, and for files the walk does not take, on the commit before the walk's four loops became one
(walk_whole).  This is the project's own output, pinned so that the shared loop cannot drift from the loops it replaced.

    python tests/golden/gen_walk_whole_golden.py      ->  tests/golden/g11_walk_whole.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "mp3-steganography-lib_amd"))


def cases():
    """name -> bytes; shared with tests/test_file_lists.py"""
    mp3 = open(os.path.join(HERE, "test.mp3"), "rb").read()
    k = mp3.index(b"\xff\xfb")                                      # the first frame: its main data begins 511 bytes in front of the file
    back = mp3[:k + 4] + b"\xff" + bytes([mp3[k + 5] | 0x80]) + mp3[k + 6:]
    return {"whole": mp3,
            "irregular": back,
            "cut": mp3[:len(mp3) * 2 // 3 + 7],                      # ends inside a frame
            "cut_side": mp3[:len(mp3) // 2 + 20 - (len(mp3) // 2) % 4],
            "garbage": b"not an mp3 file at all" * 10,
            "no_sync": b"\0" * 64,
            "one_byte": b"\xff",
            "empty": b""}


def walk(mlib, data):
    """-> {field: array}: the call's code, and everything mp3s_walk_stream says of a stream it calls regular"""
    try:
        w = mlib.walk_stream(data)
    except mlib.Mp3sError as e:
        return {"code": np.array(e.code)}
    out = {"code": np.array(0), "regular": np.array(int(w["regular"]))}
    if w["regular"]:
        for k in ("n_frames", "channels", "sampling_rate", "bit_rate", "dup_last_frame", "max_part2_3_length", "any_silent", "blob_len"):
            out[k] = np.array(int(w[k]))
        for k in ("refs", "stream", "tables"):
            out[k] = np.frombuffer(np.ascontiguousarray(w[k]).tobytes(), dtype=np.uint8)
    return out


def main():
    from mp3stego import _lib
    out = {}
    for name, data in cases().items():
        r = walk(_lib, data)
        print(name, len(data), {k: (int(v) if v.ndim == 0 else v.shape) for k, v in r.items()})
        for k, v in r.items():
            out[name + "__" + k] = v
    np.savez_compressed(os.path.join(HERE, "g11_walk_whole.npz"), **out)


if __name__ == "__main__":
    main()
