"""The oracle on streams whose headers change from frame to frame, pinned to the reference (tests/golden/g10_vbr.npz,
written by gen_vbr_golden.py from tests/vbr_streams.py G10): per-frame VBR over all 14 bit-rate indices, 44.1 -> 48 ->
32 kHz switches, a last frame with a rate and bit rate of its own, reserved rate bits in a 48 kHz stream, main_data_begin
511 behind the smallest frames, a stereo -> mono change.  The GPU tests on such streams (test_vbr_streams.py) compare
with the oracle; this is what makes that a comparison with the reference."""
import hashlib
import os

import numpy as np
import pytest

import vbr_streams as V


@pytest.fixture(scope="module")
def g10(golden_dir):
    return np.load(os.path.join(golden_dir, "g10_vbr.npz"))


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def _message_bits(message):
    """'<character count>#<message>' as UTF-8 bits, MSB first (steganography.py:44-47, :9-24)"""
    m = (str(len(message)) + "#" + message).encode("utf-8")
    return np.unpackbits(np.frombuffer(m, dtype=np.uint8))


def test_g10_streams_are_reproducible(g10):
    for n in V.G10_NAMES:
        assert V.g10_stream(n) == g10[n + "__mp3"].tobytes(), n


def test_g10_streams_change_headers():
    """what the fixture is for: the headers really change, the reservoir really reaches back 9 frames"""
    import oracle_lib as O
    vbr = O.decode(V.g10_stream("vbr_joint_44"))["frames"]
    assert len({(int(h[2]) >> 4) & 15 for h in vbr["hdr"]}) == 14
    assert {(int(h[3]) >> 4) & 3 for h in vbr["hdr"]} == {0, 1, 2, 3}
    assert len({int(f["sr_idx"]) for f in O.decode(V.g10_stream("rate_switch"))["frames"]}) == 3
    assert {(int(h[2]) >> 2) & 3 for h in O.decode(V.g10_stream("reserved_48"))["frames"]["hdr"]} == {1, 3}
    deep = O.decode(V.g10_stream("deep_reservoir_48"))["frames"]
    assert deep["main_data_begin"].max() == 511 and deep["frame_size"].min() == 96


@pytest.mark.parametrize("name", V.G10_NAMES)
def test_oracle_decodes_like_reference(orc, g10, name):
    data = g10[name + "__mp3"].tobytes()
    r = orc.decode(data)
    if str(g10[name + "__error"]):
        assert r["rc"] != 0, name                            # the reference raised
        return
    assert r["rc"] == 0, name
    assert r["n_frames"] == int(g10[name + "__n_frames"]) and r["channels"] == int(g10[name + "__nch"]), name
    assert r["sampling_rate"] == int(g10[name + "__sampling_rate"]), name          # the last frame's
    assert r["bit_rate"] // 1000 == int(g10[name + "__kbps"]), name                 # the last frame's
    assert np.array_equal(r["bits"], g10[name + "__bits"]), name
    head = g10[name + "__pcm_head"]
    assert r["pcm"][:len(head)].tobytes() == head.tobytes(), name
    assert _sha(r["pcm"].tobytes()) == bytes(g10[name + "__pcm_sha256"]).decode(), name
    i16 = orc.pcm_to_i16(r["pcm"])
    assert _sha(i16.tobytes()) == bytes(g10[name + "__pcm_i16_sha256"]).decode(), name
    assert _sha(orc.wav_bytes(i16, r["sampling_rate"])) == bytes(g10[name + "__wav_sha256"]).decode(), name


@pytest.mark.parametrize("name", sorted(V.G10_HIDE))
def test_oracle_hide_chain_like_reference(orc, g10, name):
    """decode -> int16 -> encode at the last frame's rate and bit rate, message hidden = the reference's hide_message"""
    r = orc.decode(g10[name + "__mp3"].tobytes())
    e = orc.encode(orc.pcm_to_i16(r["pcm"]), r["sampling_rate"], r["bit_rate"] // 1000, _message_bits(V.G10_HIDE[name]))
    assert e["rc"] == 0
    assert e["mp3"] == g10[name + "__hide_mp3"].tobytes(), name
    assert bool(e["too_long"]) == bool(g10[name + "__hide_too_long"]), name
    # ... which a re-encode at the first frame's rate / bit rate would not give
    first = r["frames"][0]
    f_rate, f_kbps = [44100, 48000, 32000][int(first["sr_idx"])], [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320][(int(first["hdr"][2]) >> 4) & 15]
    assert (f_rate, f_kbps) != (r["sampling_rate"], r["bit_rate"] // 1000)
