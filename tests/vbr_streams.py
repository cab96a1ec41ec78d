"""Streams whose headers change from frame to frame (VBR, sampling-rate switches, a last frame of its own, reserved rate
bits, a channel change), built with tests/frame_synth.py.  The reference parses every frame under its own header
(decoder/MP3_Parser.py:66-79) and takes the WAV's rate and the re-encode bit rate from the LAST frame (:91, :93-98).

G10 are the short streams pinned to the reference (tests/golden/g10_vbr.npz, gen_vbr_golden.py); the families are the
longer streams of the GPU tests (tests/test_vbr_streams.py), joined with frame_synth.concat so that the slow
synthesiser only writes a few hundred frames of each.
"""
import functools

from frame_synth import concat, make_stream

BLOCKS = (0, 1, 2, 3)
VBR14 = [1 + (5 * f) % 14 for f in range(64)]        # every bit-rate index 1..14, neighbours far apart


def _vbr(n, off=0):
    return [VBR14[(f + off) % 14] for f in range(n)]


# ---- G10: at most 24 frames each (the reference decodes ~4 frames/s and encodes ~1 frame/s)
G10 = {
    # per-frame VBR over all 14 bit-rate indices: reservoir, short / start / stop / mixed blocks, joint stereo with every mode_ext
    "vbr_joint_44": dict(seed=101, n_frames=22, sr_idx=0, bitrate_idx=_vbr(22), mode=1, mode_ext=[f % 4 for f in range(22)],
                         block_types=BLOCKS, allow_mixed=True),
    # 44.1 -> 48 -> 32 kHz inside one reservoir
    "rate_switch": dict(seed=102, n_frames=18, sr_idx=[0] * 6 + [1] * 6 + [2] * 6, bitrate_idx=_vbr(18, 3), mode=0,
                        block_types=BLOCKS),
    # the last frame has a rate and a bit rate of its own: the WAV and the re-encode take them
    "last_own": dict(seed=103, n_frames=14, sr_idx=[1] * 13 + [2], bitrate_idx=[11] * 13 + [5], mode=0, block_types=(0, 2)),
    # reserved rate bits in a 48 kHz stream (the frame keeps the rate and tables of the one before)
    "reserved_48": dict(seed=104, n_frames=12, sr_idx=[1] * 5 + [3] + [1] * 5 + [3], bitrate_idx=_vbr(12, 6), mode=1,
                        mode_ext=2, block_types=BLOCKS),
    # main_data_begin 511 behind the smallest frames (32 kbit/s at 48 kHz): the data starts 9 frames back
    "deep_reservoir_48": dict(seed=105, n_frames=20, sr_idx=1, bitrate_idx=[14] * 4 + [1] * 16, mode=0, fill=0.2, max_mdb=511),
}
G10_HIDE = {"vbr_joint_44": "vbr!", "last_own": "last"}   # streams whose hide_message bytes the reference wrote


def g10_stream(name):
    if name == "stereo_to_mono":                      # the reference raises (ragged pcm_data); the library refuses
        return concat(make_stream(106, 4, bitrate_idx=9), make_stream(107, 4, bitrate_idx=9, mode=3))
    return make_stream(**G10[name])


G10_NAMES = list(G10) + ["stereo_to_mono"]


# ---- families of the GPU tests
@functools.lru_cache(maxsize=None)
def family_a():
    """per-frame VBR at each sampling rate, in stereo, joint (mode_ext 0..3, the intensity bit included) and mono, all block types"""
    out = {}
    for sr, rate in enumerate(("44", "48", "32")):
        for mname, mode, ext in (("stereo", 0, 0), ("joint", 1, [0, 1, 2, 3] * 10), ("mono", 3, 0)):
            out[f"a_{rate}_{mname}"] = make_stream(200 + 10 * sr + mode, 36, sr_idx=sr, bitrate_idx=_vbr(36, sr), mode=mode,
                                                  mode_ext=ext, block_types=BLOCKS, allow_mixed=sr == 0)
    # CRC on some frames and not others (without reservoir: the reference reads earlier frames with the current frame's header length)
    out["a_44_crc_some"] = make_stream(231, 30, bitrate_idx=_vbr(30), crc=[f % 3 == 0 for f in range(30)], use_reservoir=False,
                                       block_types=(0, 2))
    out["a_48_deep_reservoir"] = make_stream(232, 40, sr_idx=1, bitrate_idx=[13] * 4 + [1] * 36, fill=0.2, max_mdb=511)
    return out


@functools.lru_cache(maxsize=None)
def _seg(seed, n, **kw):
    return make_stream(seed, n, **kw)


@functools.lru_cache(maxsize=None)
def family_b():
    """first frame at 32 kbit/s and the rest at 320, the reverse, and a reverse one longer than a decode chunk (16 384 frames)"""
    small, big = _seg(301, 60, bitrate_idx=1), _seg(302, 60, bitrate_idx=14)
    return {"b_32_then_320": concat(_seg(303, 1, bitrate_idx=1), *[big] * 50),                # 3 001 frames
            "b_320_then_32": concat(_seg(304, 1, bitrate_idx=14), *[small] * 50),
            "b_320_then_32_long": concat(_seg(304, 1, bitrate_idx=14), *[small] * 275)}     # 16 501 frames


@functools.lru_cache(maxsize=None)
def family_c():
    """rate switches at every offset modulo 32 frames (the stream kernel's waves take 2..8 frames, 4 waves a workgroup) and
    across the 16 384-frame decode chunk's halo"""
    segs = [_seg(311 + r, 33, sr_idx=r, bitrate_idx=9 + r, block_types=(0, 2)) for r in range(3)]
    switch = [make_stream(314, 96, sr_idx=[(f * f // 7 + f // 5) % 3 for f in range(96)], bitrate_idx=_vbr(96, 1), mode=1,
                          mode_ext=2, block_types=BLOCKS)]      # per-frame switches inside one reservoir
    base = _seg(315, 127, bitrate_idx=5)
    halo = concat(*[base] * 129, _seg(316, 1, sr_idx=1, bitrate_idx=5), _seg(317, 1, bitrate_idx=5),
                  _seg(318, 6, sr_idx=2, bitrate_idx=5))           # 48 kHz at frame 16 383, 44.1 at 16 384, 32 kHz from 16 385
    return {"c_offsets": concat(*[segs[k % 3] for k in range(33)]),           # switches at 33 k: residue k mod 32
            "c_per_frame": switch[0], "c_chunk_halo": halo}


@functools.lru_cache(maxsize=None)
def family_d():
    """the last frame's rate or bit rate differs from the rest"""
    return {"d_last_rate": make_stream(321, 40, sr_idx=[1] * 39 + [2], bitrate_idx=[9] * 39 + [7], block_types=(0, 2)),
            "d_last_bitrate": make_stream(322, 40, bitrate_idx=[11] * 39 + [6]),
            "d_last_rate_long": concat(*[_seg(323, 100, bitrate_idx=9)] * 40, _seg(324, 1, sr_idx=1, bitrate_idx=12))}


@functools.lru_cache(maxsize=None)
def family_e():
    """reserved rate bits inside 48 and 32 kHz streams (the frame keeps the rate of the one before), also as the last frame"""
    return {"e_reserved_48": make_stream(331, 40, sr_idx=[1] * 17 + [3] + [1] * 22, bitrate_idx=_vbr(40), mode=1, mode_ext=2,
                                         block_types=BLOCKS),
            "e_reserved_32": make_stream(332, 40, sr_idx=[2] * 9 + [3, 3] + [2] * 28 + [3], bitrate_idx=_vbr(40, 2), block_types=(0, 2))}


@functools.lru_cache(maxsize=None)
def family_f():
    """a channel change behind the first chunk (the library refuses it, MP3S_E_UNSUPPORTED; the oracle's rc != 0)"""
    st = _seg(341, 100, bitrate_idx=9)
    return {"f_to_mono_late": concat(*[st] * 50, _seg(342, 4, bitrate_idx=9, mode=3)),
            "f_to_stereo_late": concat(*[_seg(343, 100, bitrate_idx=9, mode=3)] * 30, _seg(344, 4, bitrate_idx=9))}


G_RESERVED = (5, 6, 14, 23, 31, 39)                   # frames of family_g that carry the reserved rate bits; 39 is the last
G_SR_IDX = {name: [3 if f in G_RESERVED else sr for f in range(40)] for name, sr in (("g_reserved_48_long", 1), ("g_reserved_44_long", 0))}


@functools.lru_cache(maxsize=None)
def family_g():
    """reserved rate bits inside long-block streams at 48 and at 44.1 kHz: every reserved frame has regions whose bounds are those of
    the rate it inherits (neither is the 32 kHz row that clamping the header's two bits to 2 would pick).  The streams of the list
    calls' tests only (tests/test_list_calls_foreign.py): not part of all_good()"""
    return {name: make_stream(351 + k, 40, sr_idx=sr, bitrate_idx=_vbr(40, 4 + k), block_types=(0,))
            for k, (name, sr) in enumerate(G_SR_IDX.items())}


def all_good():
    """every family of streams the library decodes"""
    out = {}
    for fam in (family_a, family_b, family_c, family_d, family_e):
        out.update(fam())
    return out
