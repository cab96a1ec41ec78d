"""What mirrors include/mp3s.h on the Python side (libmp3s_hip.so, built in-tree by ../Makefile): the constants and error codes, every
record as a ctypes.Structure and / or a numpy dtype (RECORDS names them by the header's names), ONE prototype table in the header's
order (PROTOTYPES) and lib(), which loads the library and applies the table.  tests/test_abi.py holds the table and the records against
the header itself.  What calls the library is mp3stego/_lib.py.

There is no CPU fallback: if the shared library is missing, or no MI355X is visible, the first call that needs the transforms raises.
"""
import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmp3s_hip.so")

MP3S_PCM_I16, MP3S_PCM_F32, MP3S_PCM_F64 = 0, 1, 2
E_NO_DEVICE, E_HIP, E_ARG, E_MALFORMED, E_UNSUPPORTED, E_STEP_RANGE, E_NOMEM, E_EXIT, E_BUSY, E_TABLES = -1, -2, -3, -4, -5, -6, -7, -8, -9, -10
RF_ACTIVE, RF_USED_ADDR_IN, RF_STEP_RANGE, RF_LOG_GUARD, RF_LISTED = 1, 2, 4, 8, 16


class Mp3sError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mp3s error {code}: {msg}")
        self.code = code
        self.text = msg      # for E_EXIT: the exact string the reference passes to sys.exit()


class GranuleSI(C.Structure):
    _fields_ = [("global_gain", C.c_uint8), ("scalefac_scale", C.c_uint8), ("block_type", C.c_uint8),
                ("mixed_block_flag", C.c_uint8), ("preflag", C.c_uint8), ("sub_block_gain", C.c_uint8 * 3),
                ("scale_fac_l", C.c_uint8 * 22), ("scale_fac_s", C.c_uint8 * 39), ("pad", C.c_uint8 * 3)]


GRANULE_SI_DTYPE = np.dtype([("global_gain", "u1"), ("scalefac_scale", "u1"), ("block_type", "u1"),
                             ("mixed_block_flag", "u1"), ("preflag", "u1"), ("sub_block_gain", "u1", (3,)),
                             ("scale_fac_l", "u1", (22,)), ("scale_fac_s", "u1", (3, 13)), ("pad", "u1", (3,))])
FRAME_HDR_DTYPE = np.dtype([("sr_idx", "u1"), ("nch", "u1"), ("ms_stereo", "u1"), ("flags", "u1"),
                            ("stream_first", "<u4")])
RATE_FRAME_DTYPE = np.dtype([("max_bits", "<i4"), ("sr_idx", "<i4"), ("hide_end", "<i4"), ("stream", "<i4")])
UNIT_SIDE_DTYPE = np.dtype([("part2_3_length", "<u2"), ("big_values", "<u2"), ("global_gain", "u1"),
                            ("scalefac_compress", "u1"), ("window_switching", "u1"), ("block_type", "u1"),
                            ("mixed_block_flag", "u1"), ("table_select", "u1", (3,)), ("region0_count", "u1"),
                            ("region1_count", "u1"), ("preflag", "u1"), ("scalefac_scale", "u1"),
                            ("count1table_select", "u1"), ("sub_block_gain", "u1", (3,))])
FRAME_SIDE_DTYPE = np.dtype([("md_off", "<u4"), ("md_len", "<u4"), ("nch", "u1"), ("sr_idx", "u1"), ("ms_stereo", "u1"),
                             ("flags", "u1"), ("scfsi", "u1", (2, 4)), ("unit", UNIT_SIDE_DTYPE, (2, 2)),
                             ("reserved", "<u4")])
assert UNIT_SIDE_DTYPE.itemsize == 20 and FRAME_SIDE_DTYPE.itemsize == 104
GR_OUT_DTYPE = np.dtype([("part2_3_length", "<i4"), ("big_values", "<i4"), ("count1", "<i4"),
                         ("quantizer_step", "<i4"), ("region0_count", "<i4"), ("region1_count", "<i4"),
                         ("count1table_select", "<i4"), ("table_select", "<i4", (3,)), ("address", "<i4", (3,)),
                         ("n_tables", "<i4"), ("flags", "<i4"), ("reserved0", "<i4"), ("xrmax", "<i4"),
                         ("reserved", "<i4")])
assert GRANULE_SI_DTYPE.itemsize == 72 and FRAME_HDR_DTYPE.itemsize == 8 and GR_OUT_DTYPE.itemsize == 72
CHAIN_SEG_DTYPE = np.dtype([("first_frame", "<i4"), ("n_frames", "<i4"), ("hide_base", "<i4"), ("hide_begin", "<i4"),
                            ("hide_end", "<i4"), ("reserved", "<i4"), ("chain_in", "<i4", (4, 4))])
CHAIN_SEG_OUT_DTYPE = np.dtype([("cursor", "<i8"), ("chain", "<i4", (4, 4)), ("carry_used", "<i4"), ("reserved", "<i4")])
assert CHAIN_SEG_DTYPE.itemsize == 88 and CHAIN_SEG_OUT_DTYPE.itemsize == 80


class HostShare(C.Structure):
    _fields_ = [("pinned_pooled_bytes", C.c_uint64), ("pinned_pool_cap_bytes", C.c_uint64), ("local_world_size", C.c_int32),
                ("cpus_allowed", C.c_int32), ("gpu_node_cpus", C.c_int32), ("reserved", C.c_int32)]


class Parsed(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("nch", C.c_int32), ("sampling_rate", C.c_int32), ("bit_rate", C.c_int32),
                ("n_bits", C.c_int32), ("dup_last_frame", C.c_int32), ("is_", C.c_void_p), ("si", C.c_void_p),
                ("hdr", C.c_void_p), ("bits", C.c_void_p), ("table_select", C.c_void_p), ("frame_size", C.c_void_p)]


class Scanned(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("nch", C.c_int32), ("sampling_rate", C.c_int32), ("bit_rate", C.c_int32),
                ("n_bits", C.c_int32), ("dup_last_frame", C.c_int32), ("gpu_ok", C.c_int32), ("max_part2_3_length", C.c_int32),
                ("side", C.c_void_p),
                ("hdr", C.c_void_p), ("blob", C.c_void_p), ("blob_len", C.c_size_t), ("bits", C.c_void_p),
                ("frame_size", C.c_void_p)]


FRAME_REF_DTYPE = np.dtype([("file_off", "<u4"), ("md_off", "<u4"), ("md_len", "<u2"), ("frame_size", "<u2"), ("stream", "<u2"), ("flags", "<u2")])
STREAM_REF_DTYPE = np.dtype([("base", "<u4"), ("end", "<u4"), ("first_frame", "<u4"), ("n_frames", "<u4"), ("prev_size", "<u2", (9,)),
                             ("reserved", "<u2", (3,))])
assert FRAME_REF_DTYPE.itemsize == 16 and STREAM_REF_DTYPE.itemsize == 40
PS_INHERITS, PS_MISMATCH = 1, 2


class StreamRef(C.Structure):
    _fields_ = [("base", C.c_uint32), ("end", C.c_uint32), ("first_frame", C.c_uint32), ("n_frames", C.c_uint32),
                ("prev_size", C.c_uint16 * 9), ("reserved", C.c_uint16 * 3)]


class Walked(C.Structure):
    _fields_ = [("regular", C.c_int32), ("n_frames", C.c_int32), ("nch", C.c_int32), ("sampling_rate", C.c_int32), ("bit_rate", C.c_int32),
                ("dup_last_frame", C.c_int32), ("max_part2_3_length", C.c_int32), ("any_silent", C.c_int32), ("blob_len", C.c_size_t),
                ("refs", C.c_void_p), ("stream", StreamRef), ("tables", C.c_void_p)]


class Decoded(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("nch", C.c_int32), ("sampling_rate", C.c_int32), ("bit_rate", C.c_int32),
                ("n_bits", C.c_int32), ("n_rows", C.c_int64), ("pcm", C.c_void_p), ("bits", C.c_void_p)]


class Encoded(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("too_long", C.c_int32), ("hide_offset", C.c_int64), ("mp3", C.c_void_p),
                ("mp3_len", C.c_size_t), ("gr", C.c_void_p), ("scfsi", C.c_void_p), ("rate_passes", C.c_int32)]


class Carry(C.Structure):
    """what crosses a block boundary in the encoder: message cursor + per (ch*2+gr) address1..3 / quantizerStepSize"""
    _fields_ = [("cursor", C.c_int64), ("chain", (C.c_int32 * 4) * 4)]

    def to_array(self):
        return np.array([self.cursor] + [self.chain[k][j] for k in range(4) for j in range(4)], dtype=np.int64)

    @classmethod
    def from_array(cls, a):
        c = cls()
        c.cursor = int(a[0])
        for k in range(4):
            for j in range(4):
                c.chain[k][j] = int(a[1 + 4 * k + j])
        return c


class WavInfo(C.Structure):
    _fields_ = [("channels", C.c_int32), ("samplerate", C.c_int32), ("bits_per_sample", C.c_int32), ("bitrate", C.c_int32),
                ("num_of_samples", C.c_int64), ("data_offset", C.c_int64), ("n_values", C.c_int64)]


class WavImport(C.Structure):
    _fields_ = [("format", C.c_int32), ("channels", C.c_int32), ("samplerate", C.c_int32), ("bits_per_sample", C.c_int32),
                ("block_align", C.c_int32), ("bitrate", C.c_int32), ("data_offset", C.c_int64), ("n_samples", C.c_int64), ("n_frames", C.c_int64)]


WAV_U8, WAV_S16, WAV_S24, WAV_S32, WAV_F32 = 1, 2, 3, 4, 5


class WavResample(C.Structure):
    _fields_ = [("in_", WavImport), ("out_rate", C.c_int32), ("L", C.c_int32), ("M", C.c_int32), ("taps", C.c_int32), ("half", C.c_int32),
                ("n_out", C.c_int64), ("n_frames", C.c_int64)]


class File(C.Structure):
    _fields_ = [("data", C.c_void_p), ("len", C.c_size_t), ("kbps", C.c_int32), ("sampling_rate", C.c_int32),
                ("channels", C.c_int32), ("n_frames", C.c_int32), ("too_long", C.c_int32), ("n_bits", C.c_int32),
                ("hide_offset", C.c_int64), ("bits", C.c_void_p)]


class Capacity(C.Structure):
    """mp3s_capacity: what mp3s_capacity_files / mp3s_capacity_wavs answer per file"""
    _fields_ = [("bits", C.c_int64), ("hide_offset", C.c_int64), ("text_bytes", C.c_int64), ("too_long", C.c_int32), ("n_frames", C.c_int32),
                ("kbps", C.c_int32), ("sampling_rate", C.c_int32), ("channels", C.c_int32), ("active_units", C.c_int32),
                ("fallback", C.c_int32), ("reserved", C.c_int32), ("profile", C.c_void_p)]


CAPACITY_SEG_DTYPE = np.dtype([("bits", "<i8"), ("active_units", "<i4"), ("reserved", "<i4")])


class TableAudit(C.Structure):
    """mp3s_table_audit: what mp3s_table_audit_files answers per file and k_table_audit_streams writes per stream"""
    _fields_ = [("regions", C.c_int64), ("natural", C.c_int64), ("forced", C.c_int64), ("forced_ones", C.c_int64), ("foreign", C.c_int64),
                ("empty", C.c_int64), ("excess_bits", C.c_int64), ("first_forced", C.c_int64), ("last_forced", C.c_int64),
                ("n_frames", C.c_int32), ("channels", C.c_int32), ("sampling_rate", C.c_int32), ("kbps", C.c_int32),
                ("window_units", C.c_int32), ("reserved", C.c_int32), ("profile", C.c_void_p)]


TABLE_AUDIT_DTYPE = np.dtype([("regions", "<i8"), ("natural", "<i8"), ("forced", "<i8"), ("forced_ones", "<i8"), ("foreign", "<i8"), ("empty", "<i8"),
                              ("excess_bits", "<i8"), ("first_forced", "<i8"), ("last_forced", "<i8"), ("n_frames", "<i4"), ("channels", "<i4"),
                              ("sampling_rate", "<i4"), ("kbps", "<i4"), ("window_units", "<i4"), ("reserved", "<i4"), ("profile", "<u8")])
TABLE_AUDIT_UNIT_DTYPE = np.dtype([("cls", "u1", (3,)), ("forced_bits", "u1"), ("nat", "u1", (3,)), ("window", "u1"), ("excess", "<i2", (3,)),
                                   ("reserved", "<u2")])
TABLE_AUDIT_SEG_DTYPE = np.dtype([("first_frame", "<i4"), ("n_frames", "<i4")])
assert TABLE_AUDIT_DTYPE.itemsize == 104 and TABLE_AUDIT_UNIT_DTYPE.itemsize == 16 and TABLE_AUDIT_SEG_DTYPE.itemsize == 8
TA_NONE, TA_NATURAL, TA_FORCED, TA_FOREIGN, TA_EMPTY = 0, 1, 2, 3, 4     # MP3S_TA_*
TABLE_AUDIT_FIELDS = ("regions", "natural", "forced", "forced_ones", "foreign", "empty", "excess_bits", "first_forced", "last_forced",
                      "n_frames", "channels", "sampling_rate", "kbps", "window_units")


class PcmDistortion(C.Structure):
    """mp3s_pcm_distortion: what mp3s_pcm_distortion_files answers per pair"""
    _fields_ = [("err2", C.c_uint64), ("sig2", C.c_uint64), ("n_samples", C.c_int64), ("n_diff", C.c_int64), ("first_diff", C.c_int64),
                ("rows_a", C.c_int64), ("rows_b", C.c_int64), ("max_abs", C.c_uint32), ("channels", C.c_int32), ("sampling_rate", C.c_int32),
                ("n_frames", C.c_int32), ("snr_db", C.c_double), ("psnr_db", C.c_double), ("profile", C.c_void_p)]


class PcmPair(C.Structure):
    _fields_ = [("a_first", C.c_uint32), ("b_first", C.c_uint32), ("n_frames", C.c_uint32), ("out_first", C.c_uint32)]


class PcmFrameDiff(C.Structure):
    _fields_ = [("err2", C.c_uint64), ("sig2", C.c_uint64), ("max_abs", C.c_uint32), ("n_diff", C.c_uint32), ("first_diff", C.c_uint32),
                ("reserved", C.c_uint32)]


class PcmPairDiff(C.Structure):
    _fields_ = [("err2", C.c_uint64), ("sig2", C.c_uint64), ("n_diff", C.c_uint64), ("first_diff", C.c_int64), ("max_abs", C.c_uint32),
                ("reserved", C.c_uint32)]


PCM_PAIR_DTYPE = np.dtype([("a_first", "<u4"), ("b_first", "<u4"), ("n_frames", "<u4"), ("out_first", "<u4")])
PCM_FRAME_DIFF_DTYPE = np.dtype([("err2", "<u8"), ("sig2", "<u8"), ("max_abs", "<u4"), ("n_diff", "<u4"), ("first_diff", "<u4"), ("reserved", "<u4")])
PCM_PAIR_DIFF_DTYPE = np.dtype([("err2", "<u8"), ("sig2", "<u8"), ("n_diff", "<u8"), ("first_diff", "<i8"), ("max_abs", "<u4"), ("reserved", "<u4")])
NO_DIFF = 0xFFFFFFFF         # mp3s_pcm_frame_diff.first_diff of a frame without a differing sample


class PcmRunPair(C.Structure):
    """mp3s_pcm_run_pair: rows of the PCM buffer"""
    _fields_ = [("a_first", C.c_uint32), ("a_rows", C.c_uint32), ("b_first", C.c_uint32), ("b_rows", C.c_uint32), ("out_first", C.c_uint32),
                ("reserved", C.c_uint32)]


class PcmLag(C.Structure):
    """mp3s_pcm_lag: the lag record of a pair"""
    _fields_ = [("lag", C.c_int32), ("n_best", C.c_uint32), ("err2_best", C.c_uint64), ("err2_at_0", C.c_uint64), ("search_first", C.c_uint32),
                ("search_rows", C.c_uint32), ("n_rows", C.c_uint32), ("n_chunks", C.c_uint32)]


class PcmAlignment(C.Structure):
    """mp3s_pcm_alignment: what mp3s_pcm_alignment_files answers per pair"""
    _fields_ = [("at_lag", PcmDistortion), ("lag", PcmLag), ("scores", C.c_void_p)]


PCM_RUN_PAIR_DTYPE = np.dtype([("a_first", "<u4"), ("a_rows", "<u4"), ("b_first", "<u4"), ("b_rows", "<u4"), ("out_first", "<u4"), ("reserved", "<u4")])
PCM_LAG_DTYPE = np.dtype([("lag", "<i4"), ("n_best", "<u4"), ("err2_best", "<u8"), ("err2_at_0", "<u8"), ("search_first", "<u4"), ("search_rows", "<u4"),
                          ("n_rows", "<u4"), ("n_chunks", "<u4")])
PCM_MAX_LAG = 4608           # MP3S_PCM_MAX_LAG


class PcmBatchItem(C.Structure):
    _fields_ = [("src_row", C.c_int64), ("n_rows", C.c_int64), ("first_row", C.c_int64), ("slot", C.c_int32), ("reserved", C.c_int32)]


class PcmUnbatchItem(C.Structure):
    _fields_ = [("dst_frame", C.c_int64), ("n_rows", C.c_int64), ("slot", C.c_int32), ("reserved", C.c_int32)]


class PcmBatchInfo(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("nch", C.c_int32), ("sampling_rate", C.c_int32), ("bit_rate", C.c_int32),
                ("n_rows", C.c_int64), ("first_row", C.c_int64), ("valid_rows", C.c_int64)]


class PcmResampleRatio(C.Structure):
    _fields_ = [("L", C.c_int32), ("M", C.c_int32), ("taps", C.c_int32), ("half", C.c_int32)]


class PcmResampleItem(C.Structure):
    _fields_ = [("src_row", C.c_int64), ("n_rows", C.c_int64), ("first_row", C.c_int64), ("slot", C.c_int32), ("L", C.c_int32), ("M", C.c_int32),
                ("reserved", C.c_int32)]


class PcmBatchInfoAt(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("nch", C.c_int32), ("sampling_rate", C.c_int32), ("bit_rate", C.c_int32),
                ("n_rows", C.c_int64), ("first_row", C.c_int64), ("valid_rows", C.c_int64), ("in_rows", C.c_int64),
                ("out_rate", C.c_int32), ("L", C.c_int32), ("M", C.c_int32), ("reserved", C.c_int32)]


PCM_RESAMPLE_ITEM_DTYPE = np.dtype([("src_row", "<i8"), ("n_rows", "<i8"), ("first_row", "<i8"), ("slot", "<i4"), ("L", "<i4"), ("M", "<i4"), ("reserved", "<i4")])
PCM_BATCH_INFO_AT_DTYPE = np.dtype([("n_frames", "<i4"), ("nch", "<i4"), ("sampling_rate", "<i4"), ("bit_rate", "<i4"), ("n_rows", "<i8"), ("first_row", "<i8"),
                                    ("valid_rows", "<i8"), ("in_rows", "<i8"), ("out_rate", "<i4"), ("L", "<i4"), ("M", "<i4"), ("reserved", "<i4")])
PCM_BATCH_ITEM_DTYPE = np.dtype([("src_row", "<i8"), ("n_rows", "<i8"), ("first_row", "<i8"), ("slot", "<i4"), ("reserved", "<i4")])
PCM_UNBATCH_ITEM_DTYPE = np.dtype([("dst_frame", "<i8"), ("n_rows", "<i8"), ("slot", "<i4"), ("reserved", "<i4")])
PCM_BATCH_INFO_DTYPE = np.dtype([("n_frames", "<i4"), ("nch", "<i4"), ("sampling_rate", "<i4"), ("bit_rate", "<i4"),
                                 ("n_rows", "<i8"), ("first_row", "<i8"), ("valid_rows", "<i8")])
BATCH_I16, BATCH_F32 = 0, 1  # MP3S_BATCH_*: int16, float32 = int16 / 32768
BATCH_FORMATS = {"i16": BATCH_I16, "f32": BATCH_F32, BATCH_I16: BATCH_I16, BATCH_F32: BATCH_F32}
BATCH_DTYPES = {BATCH_I16: np.dtype(np.int16), BATCH_F32: np.dtype(np.float32)}


class QmdctChannel(C.Structure):
    """mp3s_qmdct_channel: the features of one channel of a stream (include/mp3s.h, vi-g)"""
    _fields_ = [("hist", C.c_int64 * 16), ("intra", (C.c_int64 * 9) * 9), ("inter", (C.c_int64 * 9) * 9), ("max_abs", C.c_int64), ("bandwidth", C.c_int64)]


class QmdctFeatures(C.Structure):
    """mp3s_qmdct_features: what mp3s_qmdct_features_files answers per file and k_qmdct_features writes per stream"""
    _fields_ = [("ch", QmdctChannel * 2), ("n_frames", C.c_int32), ("channels", C.c_int32), ("sampling_rate", C.c_int32), ("kbps", C.c_int32),
                ("n_lines", C.c_int32), ("reserved", C.c_int32)]


class QmdctBatchItem(C.Structure):
    _fields_ = [("src_frame", C.c_int64), ("n_frames", C.c_int64), ("first_granule", C.c_int64), ("slot", C.c_int32), ("reserved", C.c_int32)]


class QmdctBatchInfo(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("nch", C.c_int32), ("sampling_rate", C.c_int32), ("bit_rate", C.c_int32),
                ("n_granules", C.c_int64), ("first_granule", C.c_int64), ("valid_granules", C.c_int64)]


QMDCT_T, QMDCT_SLICE = 4, 64          # MP3S_QMDCT_T, MP3S_QMDCT_SLICE
QMDCT_CHANNEL_DTYPE = np.dtype([("hist", "<i8", (16,)), ("intra", "<i8", (9, 9)), ("inter", "<i8", (9, 9)), ("max_abs", "<i8"), ("bandwidth", "<i8")])
QMDCT_FEATURES_DTYPE = np.dtype([("ch", QMDCT_CHANNEL_DTYPE, (2,)), ("n_frames", "<i4"), ("channels", "<i4"), ("sampling_rate", "<i4"), ("kbps", "<i4"),
                                 ("n_lines", "<i4"), ("reserved", "<i4")])
QMDCT_BATCH_ITEM_DTYPE = np.dtype([("src_frame", "<i8"), ("n_frames", "<i8"), ("first_granule", "<i8"), ("slot", "<i4"), ("reserved", "<i4")])
QMDCT_BATCH_INFO_DTYPE = np.dtype([("n_frames", "<i4"), ("nch", "<i4"), ("sampling_rate", "<i4"), ("bit_rate", "<i4"),
                                   ("n_granules", "<i8"), ("first_granule", "<i8"), ("valid_granules", "<i8")])
assert QMDCT_CHANNEL_DTYPE.itemsize == 1440 and QMDCT_FEATURES_DTYPE.itemsize == 2904
assert QMDCT_BATCH_ITEM_DTYPE.itemsize == 32 and QMDCT_BATCH_INFO_DTYPE.itemsize == 40


class IndexInfo(C.Structure):
    _fields_ = [("n_frames", C.c_int64), ("nch", C.c_int32), ("sampling_rate", C.c_int32), ("bit_rate", C.c_int32),
                ("dup_last_frame", C.c_int32), ("gpu_ok", C.c_int32), ("reserved", C.c_int32)]


SELECT_SPAN_DTYPE = np.dtype([("first_entry", "<i4"), ("reach", "<i4")])
SELECT_VARIANTS = 10
NO_CURSOR = 0x3fffffff


class PipeStats(C.Structure):
    _fields_ = [("submitted", C.c_int64), ("collected", C.c_int64), ("fast", C.c_int64), ("slow", C.c_int64),
                ("scan_ms", C.c_double), ("issue_ms", C.c_double), ("last_device_span_ms", C.c_double), ("scan_cpu_ms", C.c_double),
                ("resolved", C.c_int64), ("rehearsal_ms", C.c_double), ("rehearsals", C.c_int64), ("lanes", C.c_int64), ("queue_shared", C.c_int64)]


class Block(C.Structure):
    _fields_ = [("total_frames", C.c_int64), ("first_frame", C.c_int64), ("n_frames", C.c_int64), ("is_last", C.c_int32),
                ("carry_used", C.c_int32), ("carry_out", Carry), ("file", File)]


REVEAL_TILE = 256            # MP3S_REVEAL_TILE: frames a workgroup of k_reveal takes at a time
RV_BAD_REF = 1

# the device's constant tables (csrc, not the header: mp3s_debug_tables hands out a copy and its size)
DEV_TABLES_DTYPE = np.dtype([
    ("synth_matrix", "<f8", (64, 32)), ("synth_window", "<f8", (512,)), ("synth_window_t", "<f8", (32, 16)), ("imdct_cos36", "<f8", (36, 18)),
    ("imdct_cos12", "<f8", (12, 6)), ("sine_block", "<f8", (4, 36)), ("alias_cs", "<f8", (8,)), ("alias_ca", "<f8", (8,)),
    ("pow43", "<f8", (8207,)), ("pow2q", "<f8", (312,)), ("pow2h", "<f8", (40,)), ("sqrt2", "<f8"),
    ("synth_fast", "<f8", (344,)), ("synth_eps_a", "<f8"), ("synth_eps_x", "<f8"), ("synth_eps_g", "<f8"), ("imdct_kappa", "<f8"), ("synth_window_f", "<f8", (32, 16)), ("synth_window_fs", "<f8", (32, 16)), ("synth_xbound", "<f8"), ("synth_reserved", "<f8"), ("synth_stream", "<f8", (2, 8, 112)), ("stream_cx", "<f8", (32, 16)), ("stream_taps", "<f8", (2, 32, 16)), ("imdct_rot", "<f8", (1, 18)), ("imdct_pq", "<f8", (10, 18)),
    ("rq_map", "u1", (3, 3, 32, 20)), ("reorder_src", "<i2", (3, 576)), ("pre_tab", "u1", (24,)),
    ("enwindow", "<i4", (512,)), ("fl", "<i4", (32, 64)), ("cos_l", "<i4", (18, 36)), ("mdct_cs", "<i4", (8,)),
    ("mdct_ca", "<i4", (8,)), ("steptab", "<f8", (128,)), ("steptabi", "<i4", (128,)), ("_pad_int2idx", "u1", (8,)), ("int2idx", "<u2", (10000,)),   # (int2idx is alignas(16))
    ("sfb_long", "<i4", (3, 23)), ("en_base", "<i4", (32,)), ("en_step", "<i4", (32,)), ("subdv", "<i4", (23, 2)), ("subdiv_lut", "<u4", (3, 289)), ("hlen13", "u1", (256,)), ("hlen15", "u1", (256,)),
    ("hlen16", "u1", (256,)), ("hlen24", "u1", (256,)), ("hlen_c1a", "u1", (16,)), ("linbits", "u1", (32,)),
    ("linmax", "<i4", (32,)), ("transform", "u1", (32, 2)), ("dec_max", "u1", (32,)),
    ("huf_tinfo", "<u4", (32,)), ("_pad_huf_tab", "u1", (8,)), ("huf_tab", "<u2", (10256 + 1200 + 2560,)),   # (huf_tab is alignas(16))
    ("hcod", "<u4", (4, 256)), ("hcod_c1a", "u1", (16,)), ("rl_hl", "<u4", (256, 2)), ("rl_c1w", "<u4", (16,)), ("rl_t1", "<u4", (128,)), ("rl_t2", "<u4", (128,)), ("rl_t8", "<u4", (128,))], align=True)   # (the struct is 16-byte aligned)

# the header's record (typedef struct { ... } mp3s_<name>;) -> its mirrors here; tests/test_abi.py compiles the header and compares sizes
RECORDS = {
    "granule_si": (GranuleSI, GRANULE_SI_DTYPE), "frame_hdr": (FRAME_HDR_DTYPE,), "rate_frame": (RATE_FRAME_DTYPE,), "gr_out": (GR_OUT_DTYPE,),
    "host_share": (HostShare,), "chain_seg": (CHAIN_SEG_DTYPE,), "chain_seg_out": (CHAIN_SEG_OUT_DTYPE,), "select_span": (SELECT_SPAN_DTYPE,),
    "unit_side": (UNIT_SIDE_DTYPE,), "frame_side": (FRAME_SIDE_DTYPE,), "frame_ref": (FRAME_REF_DTYPE,), "stream_ref": (StreamRef, STREAM_REF_DTYPE),
    "walked": (Walked,), "scanned": (Scanned,), "parsed": (Parsed,), "decoded": (Decoded,), "index_info": (IndexInfo,), "encoded": (Encoded,),
    "carry": (Carry,), "wav_info": (WavInfo,), "wav_import": (WavImport,), "wav_resample": (WavResample,), "file": (File,), "block": (Block,),
    "capacity_seg": (CAPACITY_SEG_DTYPE,), "capacity": (Capacity,), "pcm_pair": (PcmPair, PCM_PAIR_DTYPE),
    "pcm_frame_diff": (PcmFrameDiff, PCM_FRAME_DIFF_DTYPE), "pcm_pair_diff": (PcmPairDiff, PCM_PAIR_DIFF_DTYPE), "pcm_distortion": (PcmDistortion,),
    "pcm_run_pair": (PcmRunPair, PCM_RUN_PAIR_DTYPE), "pcm_lag": (PcmLag, PCM_LAG_DTYPE), "pcm_alignment": (PcmAlignment,),
    "table_audit_unit": (TABLE_AUDIT_UNIT_DTYPE,), "table_audit_seg": (TABLE_AUDIT_SEG_DTYPE,), "table_audit": (TableAudit, TABLE_AUDIT_DTYPE),
    "pcm_batch_item": (PcmBatchItem, PCM_BATCH_ITEM_DTYPE), "pcm_unbatch_item": (PcmUnbatchItem, PCM_UNBATCH_ITEM_DTYPE),
    "pcm_batch_info": (PcmBatchInfo, PCM_BATCH_INFO_DTYPE), "pcm_resample_ratio": (PcmResampleRatio,),
    "pcm_resample_item": (PcmResampleItem, PCM_RESAMPLE_ITEM_DTYPE), "pcm_batch_info_at": (PcmBatchInfoAt, PCM_BATCH_INFO_AT_DTYPE),
    "qmdct_channel": (QmdctChannel, QMDCT_CHANNEL_DTYPE), "qmdct_features": (QmdctFeatures, QMDCT_FEATURES_DTYPE),
    "qmdct_batch_item": (QmdctBatchItem, QMDCT_BATCH_ITEM_DTYPE), "qmdct_batch_info": (QmdctBatchInfo, QMDCT_BATCH_INFO_DTYPE),
    "pipe_stats": (PipeStats,)}

VOID = object()              # a restype of PROTOTYPES: the function returns nothing


def _prototypes():
    """every function include/mp3s.h declares, in its order: name -> (restype, or None for int; argtypes)"""
    P, vp, i32, i64, sz, u32, f64 = C.POINTER, C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_uint32, C.c_double
    pvp, psz, pi32, pi64, pf64 = P(vp), P(sz), P(C.c_int32), P(i64), P(f64)
    return {
        "mp3s_ctx_create": (None, [i32, pvp]),
        "mp3s_device_count": (None, [pi32]),
        "mp3s_ctx_destroy": (VOID, [vp]),
        "mp3s_last_error": (C.c_char_p, []),
        "mp3s_version": (C.c_char_p, []),
        "mp3s_device_name": (None, [vp, C.c_char_p, sz]),
        "mp3s_device_pci": (None, [vp, C.c_char_p, sz]),
        "mp3s_sync": (None, [vp]),
        "mp3s_ctx_wait": (None, [vp, vp]),
        "mp3s_ctx_wait_last": (None, [vp, vp]),
        "mp3s_ctx_run_stats": (None, [vp, vp]),
        "mp3s_ctx_host_share": (None, [vp, vp]),
        "mp3s_ctx_set_option": (None, [vp, i32, i64]),
        "mp3s_ctx_get_option": (None, [vp, i32, pi64]),
        "mp3s_debug_tables": (vp, [psz]),
        "mp3s_debug_scfsi_energies": (None, [vp, i32, vp]),
        "mp3s_debug_guard_margin": (None, [vp, vp, vp, i64]),
        "mp3s_debug_parse_scanned_frame": (None, [vp, vp, vp, vp]),
        "mp3s_debug_walk_rate": (None, [vp, sz, f64, pf64, pi64]),
        "mp3s_dev_alloc": (None, [vp, sz, pvp]),
        "mp3s_dev_free": (None, [vp, vp]),
        "mp3s_dev_upload": (None, [vp, vp, vp, sz]),
        "mp3s_dev_download": (None, [vp, vp, vp, sz]),
        "mp3s_dev_memset": (None, [vp, vp, i32, sz]),
        "mp3s_dev_copy": (None, [vp, vp, vp, sz]),
        "mp3s_timer_start": (None, [vp]),
        "mp3s_timer_stop": (None, [vp, P(C.c_float)]),
        "mp3s_synth_mode": (None, [vp, f64, pi64]),
        "mp3s_bench_copy": (None, [vp, sz, i32, pf64]),
        "mp3s_profile_enable": (None, [vp, i32]),
        "mp3s_profile_select": (None, [vp, C.c_uint]),
        "mp3s_profile_collect": (None, [vp, vp, vp, i32]),
        "mp3s_decode_transform_dev": (None, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        "mp3s_decode_transform": (None, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
        "mp3s_encode_transform_dev": (None, [vp, vp, vp, i32, vp]),
        "mp3s_encode_transform": (None, [vp, vp, vp, i32, vp]),
        "mp3s_rate_loop_dev": (None, [vp, vp, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp]),
        "mp3s_chain_resolve_dev": (None, [vp, vp, vp, i32, vp, i32, vp, vp, vp, vp]),
        "mp3s_chain_redo_dev": (None, [vp, vp, vp, i32, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp]),
        "mp3s_select_patterns": (VOID, [vp]),
        "mp3s_select_plan": (None, [vp, i32, vp, vp, vp, i32]),
        "mp3s_rate_select_dev": (None, [vp, vp, vp, i32, vp, i32, vp, vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
        "mp3s_rate_variants_dev": (None, [vp, vp, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
        "mp3s_select_dev": (None, [vp, vp, vp, vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
        "mp3s_huffman_decode_dev": (None, [vp, vp, vp, i32, i32, i32, vp, vp, vp]),
        "mp3s_walk_stream": (None, [vp, sz, pvp, P(Walked)]),
        "mp3s_parse_frames_dev": (None, [vp, vp, u32, vp, vp, i32, u32, vp, vp, vp, vp, vp]),
        "mp3s_stego_bits": (None, [vp, i64, i32, vp, pvp, pvp, psz]),
        "mp3s_reveal_bits_dev": (None, [vp, vp, u32, vp, vp, i32, vp, vp, vp, vp]),
        "mp3s_pack_frames_dev": (None, [vp, vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
        "mp3s_scan_stream": (None, [vp, sz, pvp, P(Scanned)]),
        "mp3s_buf_free": (VOID, [vp]),
        "mp3s_parse_stream": (None, [vp, sz, pvp, P(Parsed)]),
        "mp3s_format_stream": (None, [i32, i32, i32, vp, vp, vp, pvp, pvp, psz]),
        "mp3s_rate_frames": (None, [i32, i32, i32, i32, vp, vp]),
        "mp3s_decode_stream": (None, [vp, vp, sz, i32, pvp, P(Decoded)]),
        "mp3s_decode_streams": (None, [vp, pvp, psz, i32, i32, pvp, P(Decoded), vp]),
        "mp3s_decode_block": (None, [vp, vp, sz, i64, i64, i32, pvp, P(Decoded)]),
        "mp3s_index_stream": (None, [vp, sz, pvp, P(IndexInfo)]),
        "mp3s_index_free": (VOID, [vp]),
        "mp3s_scan_range": (None, [vp, sz, vp, i64, i64, pvp, P(Scanned)]),
        "mp3s_decode_block_indexed": (None, [vp, vp, sz, vp, i64, i64, i32, pvp, P(Decoded)]),
        "mp3s_encode_pcm": (None, [vp, vp, i64, i32, i32, i32, vp, i32, pvp, P(Encoded)]),
        "mp3s_encode_block": (None, [vp, vp, i64, i32, i64, i32, i32, i32, vp, i32, P(Carry), P(Carry), pi32, pvp, P(Encoded)]),
        "mp3s_wav_parse": (None, [vp, sz, i32, P(WavInfo)]),
        "mp3s_wav_import_info": (None, [vp, sz, i32, P(WavImport)]),
        "mp3s_wav_resample_info": (None, [vp, sz, i32, i32, P(WavResample)]),
        "mp3s_wav_resample_taps": (None, [i32, i32, vp, i32, pi32]),
        "mp3s_wav_header": (None, [i64, i32, i32, vp]),
        "mp3s_message_frame": (None, [vp, sz, pvp, pvp, psz]),
        "mp3s_message_reveal": (None, [vp, sz, pvp, pvp, psz]),
        "mp3s_decode_file": (None, [vp, vp, sz, pvp, P(File)]),
        "mp3s_decode_file_fd": (None, [vp, vp, sz, i32, pvp, P(File)]),
        "mp3s_encode_file": (None, [vp, vp, sz, i32, vp, i32, pvp, P(File)]),
        "mp3s_hide_message": (None, [vp, vp, sz, vp, sz, pvp, P(File)]),
        "mp3s_clear_file": (None, [vp, vp, sz, pvp, P(File)]),
        "mp3s_hide_message_fd": (None, [vp, vp, sz, vp, sz, i32, P(File)]),
        "mp3s_clear_file_fd": (None, [vp, vp, sz, i32, P(File)]),
        "mp3s_hide_messages": (None, [vp, vp, vp, i32, vp, vp, pvp, vp, vp]),
        "mp3s_encode_files": (None, [vp, vp, vp, i32, vp, vp, vp, pvp, vp, vp]),
        "mp3s_debug_wav_gather": (None, [vp, vp, vp, i32, vp, i64, pi64]),
        "mp3s_reencode_block": (None, [vp, vp, sz, vp, sz, i32, i32, P(Carry), pvp, P(Block)]),
        "mp3s_reencode_block_indexed": (None, [vp, vp, sz, vp, vp, sz, i32, i32, P(Carry), pvp, P(Block)]),
        "mp3s_hide_message_chunked": (None, [vp, vp, sz, vp, sz, i64, pvp, P(File)]),
        "mp3s_reveal_message": (None, [vp, sz, pvp, P(File)]),
        "mp3s_reveal_messages": (None, [vp, vp, vp, i32, pvp, vp, vp]),
        "mp3s_debug_reveal_messages": (None, [vp, vp, vp, i32, i32, pvp, vp, vp]),
        "mp3s_capacity_dev": (None, [vp, vp, vp, i32, vp, vp]),
        "mp3s_capacity_files": (None, [vp, vp, vp, i32, vp, vp, i32, pvp, vp, vp]),
        "mp3s_capacity_wavs": (None, [vp, vp, vp, i32, vp, vp, vp, i32, pvp, vp, vp]),
        "mp3s_capacity_text_bytes": (i64, [i64]),
        "mp3s_pcm_diff_dev": (None, [vp, vp, i32, vp, vp, i32, vp, vp]),
        "mp3s_pcm_distortion_files": (None, [vp, vp, vp, vp, vp, i32, i32, pvp, vp, vp]),
        "mp3s_pcm_align_dev": (None, [vp, vp, i32, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]),
        "mp3s_pcm_alignment_files": (None, [vp, vp, vp, vp, vp, i32, i32, i32, vp, i32, pvp, vp, vp]),
        "mp3s_table_audit_dev": (None, [vp, vp, vp, i32, i32, vp, i32, vp, vp, vp]),
        "mp3s_table_audit_files": (None, [vp, vp, vp, i32, i32, pvp, vp, vp]),
        "mp3s_pcm_batch_dev": (None, [vp, vp, i32, vp, vp, i32, i32, i32, i64, vp]),
        "mp3s_pcm_unbatch_dev": (None, [vp, vp, i32, i32, i64, vp, vp, i32, vp]),
        "mp3s_pcm_batch_decode_files": (None, [vp, vp, vp, i32, vp, i64, i32, i32, vp, sz, vp, vp]),
        "mp3s_pcm_batch_encode": (None, [vp, vp, i32, i32, i32, i64, vp, i32, i32, vp, vp, pvp, vp, vp]),
        "mp3s_pcm_resample_plan": (None, [i32, i32, vp]),
        "mp3s_pcm_batch_resample_dev": (None, [vp, vp, i32, vp, i32, i32, i32, i64, vp]),
        "mp3s_pcm_batch_decode_files_at": (None, [vp, vp, vp, i32, i32, vp, i64, i32, i32, vp, sz, vp, vp]),
        "mp3s_pcm_batch_encode_at": (None, [vp, vp, i32, i32, i32, i64, vp, i32, i32, i32, vp, vp, pvp, vp, vp]),
        "mp3s_qmdct_features_dev": (None, [vp, vp, i32, i32, vp, vp, i32, i32, vp]),
        "mp3s_qmdct_features_files": (None, [vp, vp, vp, i32, i32, vp, vp]),
        "mp3s_qmdct_batch_dev": (None, [vp, vp, i32, vp, vp, i32, i32, i64, vp]),
        "mp3s_qmdct_batch_decode_files": (None, [vp, vp, vp, i32, vp, i64, i32, vp, sz, vp, vp]),
        "mp3s_pipe_create": (None, [vp, i32, sz, i32, pvp]),
        "mp3s_pipe_destroy": (VOID, [vp]),
        "mp3s_pipe_submit": (None, [vp, vp, vp, i32, vp, vp, pi64]),
        "mp3s_pipe_submit_decode": (None, [vp, vp, vp, i32, pi64]),
        "mp3s_pipe_submit_encode": (None, [vp, vp, vp, i32, vp, vp, vp, pi64]),
        "mp3s_pipe_collect": (None, [vp, pi64, pvp, vp, vp, i32, pi32]),
        "mp3s_pipe_submit_block": (None, [vp, vp, sz, vp, sz, i32, i32, P(Carry), pi64]),
        "mp3s_pipe_collect_block": (None, [vp, pi64, pvp, P(Block)]),
        "mp3s_pipe_next_is_block": (None, [vp]),
        "mp3s_pipe_get_stats": (None, [vp, P(PipeStats)])}


PROTOTYPES = _prototypes()
SYMBOLS = list(PROTOTYPES)   # tests/test_abi.py checks the library exports all of them

_lib = None
_lock = threading.Lock()


def lib():
    """Load libmp3s_hip.so (raises if it has not been built: no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it with `make -C mp3-steganography-lib_amd` "
                              "(or `python __graft_entry__.py`); the HIP extension has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            if restype is not None:
                fn.restype = None if restype is VOID else restype
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise Mp3sError(rc, lib().mp3s_last_error().decode("utf-8", "replace"))
