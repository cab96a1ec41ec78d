// Host-visible launchers of the device translation unit (mp3s_device.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mp3s.h"

namespace mp3s {

// waves per channel in a synthesis tile (tile = TW*64 - 15 output slots).  2: 31 KB of LDS per workgroup, five groups =
// five waves per SIMD on a CU; the kernel waits for scalar-cache misses (the 16 KB matrix is streamed once per tile), so
// the fifth wave buys more (0.217 -> 0.207 ms) than the larger halo share (15/128 instead of 15/256) costs
#ifndef MP3S_DEC_SYNTH_TW
#define MP3S_DEC_SYNTH_TW 2
#endif
constexpr int DEC_SYNTH_TW = MP3S_DEC_SYNTH_TW;
constexpr int DEC_SYNTH_FAST_TW = 2;   // the fast int16 variant (k_dec_synth_fast)

// optional per-kernel HIP-event timing: when non-null, every kernel launch is bracketed by two events
// recorded on the launch stream; mp3s_profile_collect() turns the pairs into per-kernel totals.
enum KernelId { K_DEC_IMDCT = 0, K_DEC_SYNTH, K_ENC_ANALYSIS, K_ENC_MDCT, K_RATE_LOOP, K_DEC_HUFFMAN, K_ENC_PACK, K_CHAIN, K_WAV_RESAMPLE, K_COUNT };
struct Profiler {
    static constexpr int MAX_PAIRS = 8192;
    hipEvent_t ev[2 * MAX_PAIRS];
    int kid[MAX_PAIRS];
    int n_pairs = 0, n_created = 0;
    long dropped = 0;                         // launches that asked for an event pair and got none (MAX_PAIRS reached, event creation failed): mp3s_profile_collect refuses a table that misses them
    bool enabled = false;
    unsigned mask = ~0u;                      // bit k: kernel k gets an event pair
    double total_ms[K_COUNT] = {0};
    long count[K_COUNT] = {0};
    int take(int k);                          // a fresh event pair for kernel k: its index, or -1 (not enabled, not in the mask, none left)
    int begin(hipStream_t s, int k);          // returns pair index or -1
    void end(hipStream_t s, int pair);
    // the pair as the START and STOP event of one dispatch (hipExtLaunchKernelGGL): the kernel's own time stamps, no record packets around it
    bool attach(int k, hipEvent_t *start, hipEvent_t *stop);
};

int dev_upload_tables(hipStream_t stream);

// mp3s_debug_guard_margin: where the fused int16 decode leaves its fast values and guard widths (device arrays of `cap` doubles; a launch's
// sample i goes to element base + i)
struct GuardProbe { double *x, *eps; int64_t base, cap; };
// scratch: time-domain subband samples, float64 [nch][36 n][32], + what the fast int16 path keeps beside them
size_t dec_scratch_bytes(int n_frames, int nch);
// how a batch is decoded: the context's part (decode_how, mp3s_internal.h) and the caller's (done, the probe's base)
struct DecodeHow {
    int sf_base;              // hdr[].stream_first counts from this frame of the batch; d_is / d_si / d_hdr start there
    double eps_scale;         // int16 output: guard of the fast kernels (imdct_run<true>, k_dec_synth_fast); 0 = the exact kernels
    int32_t *d_sync;          // the context's self-clearing words (8): [2] counts the samples the guard sent through the exact order, [6..7] belong to the fix-up list; null: the exact kernels
    bool fast_imdct, float_fast, fused;   // MP3S_OPT_FAST_IMDCT: the mirrored, fused IMDCT under the fast synthesis; MP3S_OPT_FLOAT_FAST: float32 output through the fast sums,
                              // unguarded (within 1e-5, not bit-identical); MP3S_OPT_FUSED_DECODE: the fast paths as one kernel (k_decode_stream.hpp)
    hipEvent_t done;          // (may be null) recorded behind the transforms: as the last dispatch's own completion signal on the fused int16 path (no record packet), by a record otherwise
    const GuardProbe *probe;  // the fused int16 path also writes its fast values and guard widths there (null, or x == null: no probe)
};
int launch_decode(hipStream_t stream, const int16_t *d_is, const mp3s_granule_si *d_si, const mp3s_frame_hdr *d_hdr,
                  int n_frames, int nch, int n_halo, int out_format, void *d_pcm, void *d_scratch, Profiler *prof, const DecodeHow &how);

// scratch: subband samples int32 [2][32][36 n]
size_t enc_scratch_bytes(int n_frames);
int launch_encode(hipStream_t stream, const int16_t *d_pcm, const mp3s_frame_hdr *d_hdr, int n_frames, int32_t *d_mdct,
                  void *d_scratch, Profiler *prof, bool fused = false /* MP3S_OPT_FUSED_ENCODE: one kernel, no scratch (d_scratch may be null) */,
                  bool analysis_shared = true /* MP3S_OPT_ANALYSIS_SHARED */);

// entries behind the launch's own units: unit d_unit[e] once more with cursor d_cursor[e] and no inherited state, results
// to element e of d_ix / d_out / d_en (the message variants the device chooses from, launch_select)
struct RateVariantArgs {
    const int32_t *d_unit, *d_cursor;
    int n;
    int16_t *d_ix; mp3s_gr_out *d_out; int32_t *d_en;
    uint8_t *d_tables;   // n bytes: the entries' table counts (kept behind the GrInfo records: variant_out_bytes)
};
// the GrInfo array of n variant entries is followed by their table counts, one byte each
inline size_t variant_out_bytes(int n) { return (size_t)n * sizeof(mp3s_gr_out) + (((size_t)n + 15) & ~(size_t)15); }
// state: int32 [units][4] = address1, address2, address3, quantizerStepSize inherited from the previous frame
int launch_rate(hipStream_t stream, const int32_t *d_mdct, const mp3s_rate_frame *d_frames, int n_frames,
                const uint8_t *d_hide, int n_hide, const int32_t *d_cursor, const int32_t *d_state,
                const int32_t *d_list, int n_list, int16_t *d_ix, mp3s_gr_out *d_out, int32_t *d_en, Profiler *prof,
                int out_base = 0 /* unit whose results land on element 0 of d_ix / d_out / d_en */,
                int compact = 0 /* 1: d_cursor / d_state / d_out are indexed by the position in d_list; 2: d_ix / d_en too */,
                const RateVariantArgs *variants = nullptr,
                hipEvent_t done = nullptr /* the dispatch's own completion signal: no record packet behind it (MP3S_OPT_RATE_SIGNALS) */);

// the serial chains of the rate loop (k_chain.hpp): two small launches; d_agg: chain_agg_bytes(n_frames) of scratch.
// With `redo` (the rate loop's other operands) the units the check finds wrong -- they read inherited addresses that were
// not what the chain holds, or ran on another cursor -- are listed on the device, run again on what the check found
// (k_rate_redo, results in place, d_cursor updated for them: it is written then) and everything is checked once more:
// five launches, the verdict is the second check's.
struct ChainRedoArgs { const int32_t *d_mdct; const uint8_t *d_hide; int n_hide; int16_t *d_ix; int32_t *d_en; };
size_t chain_agg_bytes(int n_frames);
int launch_chain(hipStream_t stream, mp3s_gr_out *d_gr, const mp3s_rate_frame *d_frames, int n_frames, const mp3s_chain_seg *d_segs,
                 const int32_t *d_cursor, const int32_t *d_state, void *d_agg, int32_t *d_verdict, mp3s_chain_seg_out *d_seg_out,
                 Profiler *prof, const ChainRedoArgs *redo = nullptr);

// the message cursor decided on the device (k_chain_select): one workgroup per stream, after a launch_rate with variants
int launch_select(hipStream_t stream, const mp3s_chain_seg *d_segs, const mp3s_select_span *d_spans, int n_segs, int max_reach,
                  const uint8_t *d_hide, const RateVariantArgs &v, int16_t *d_ix, int32_t *d_en, mp3s_gr_out *d_out, int32_t *d_cursor,
                  void *d_pairs /* n_segs * max_reach * 8 bytes of scratch */, Profiler *prof);

// side-info parse + main-data gather on the device (k_parse.hpp) from the file image and the host's frame walk (FrameRef /
// StreamRef of mp3s_host.h, 16 / 40 bytes): side records, frame headers and the blob as the host scan would have written
// them.  image_base / md_base: what d_image[0] and d_blob[0] are in the offsets the references hold (a chunk of a long
// file brings its own piece of both).  d_tsel optional (decode jobs: the stego bits are put together from it on the host);
// d_status: one word the caller has zeroed, PARSE_* bits are OR-ed in.
using FrameRef = mp3s_frame_ref;
using StreamRef = mp3s_stream_ref;
constexpr int kParseInherits = 1, kParseMismatch = 2;
int launch_parse(hipStream_t stream, const uint8_t *d_image, uint32_t image_base, const FrameRef *d_refs, const StreamRef *d_streams, int n_frames,
                 uint32_t md_base, mp3s_frame_side *d_side, mp3s_frame_hdr *d_hdr, uint8_t *d_blob, uint64_t *d_tsel, int32_t *d_status);

// the stego bits of a batch of walked streams (k_reveal.hpp): per stream its bits packed eight to a byte, MSB first, from byte
// d_out_off[s] (a multiple of 4) of d_packed -- room for reveal_packed_bytes(n_frames) there --, their count and a status word
// (0, or kRevealBadRef: a frame reference of the stream names another stream or a place outside it; its bits are not to be used)
constexpr int kRevealTile = MP3S_REVEAL_TILE; // frames a workgroup takes at a time
constexpr int kRevealBadRef = MP3S_RV_BAD_REF;
constexpr int kRevealMaxStreams = 65535;     // of one launch
inline size_t reveal_packed_bytes(uint64_t n_frames) { return (size_t)((n_frames * 12 + 31) / 32 * 4); }   // whole dwords are written
int launch_reveal(hipStream_t stream, const uint8_t *d_image, uint32_t image_base, const FrameRef *d_refs, const StreamRef *d_streams, int n_streams,
                  const uint32_t *d_out_off, uint8_t *d_packed, int32_t *d_n_bits, int32_t *d_status);

// message capacity of the streams of an encode batch (k_capacity.hpp) from the records the chain check has made final: per stream its
// record, and with d_profile (optional, [frames of the batch]) per frame the running sum of the stream's bits up to and including it
int launch_capacity(hipStream_t stream, const mp3s_gr_out *d_gr, const mp3s_chain_seg *d_segs, int n_segs, mp3s_capacity_seg *d_out, uint32_t *d_profile);

// the table audit of a batch of Huffman-decoded streams (k_table_audit.hpp; the rule: include/mp3s.h, vi-e): a record per unit into
// d_units [n_frames][4] (16-byte aligned), then per stream of d_segs its record and, with d_profile (optional, [n_frames]), a word per frame
int launch_table_audit(hipStream_t stream, const int16_t *d_is, const mp3s_frame_side *d_side, int n_frames, int nch, const mp3s_table_audit_seg *d_segs,
                       int n_segs, mp3s_table_audit_unit *d_units, mp3s_table_audit *d_out, uint32_t *d_profile);

// the exact difference of pairs of frame runs of one int16 PCM buffer [frame][1152][nch] (k_pcmdiff.hpp): pass 1 writes a record per
// compared frame (pair p's at d_frames[out_first ..]), pass 2 a record per pair.  Pass 1 takes kPcmDiffWaves frames to a workgroup and
// finds them in d_tiles, which the host makes from the pairs' frame counts (pcm_diff_tiles; n_tiles = the grid): a pair of 0 frames has
// no tile and gets its (zero) record from pass 2.  d_pcm must be 16-byte aligned.
constexpr int kPcmDiffWaves = 4;
struct PcmTile { uint32_t pair, first; };   // 8 bytes: frames [first, first + kPcmDiffWaves) of pair `pair`, cut at its n_frames
// appends the tiles of pairs[0 .. n_pairs) to `tiles` (anything with push_back); false: more tiles than a grid takes
template <class Tiles>
bool pcm_diff_tiles(const mp3s_pcm_pair *pairs, int n_pairs, Tiles &tiles)
{
    uint64_t n = tiles.size();
    for (int p = 0; p < n_pairs; p++) n += ((uint64_t)pairs[p].n_frames + kPcmDiffWaves - 1) / kPcmDiffWaves;
    if (n > 0x7fffffffu) return false;
    for (int p = 0; p < n_pairs; p++)
        for (uint64_t f = 0; f < pairs[p].n_frames; f += kPcmDiffWaves) tiles.push_back(PcmTile{(uint32_t)p, (uint32_t)f});
    return true;
}
int launch_pcm_diff(hipStream_t stream, const int16_t *d_pcm, int nch, const mp3s_pcm_pair *d_pairs, int n_pairs, const PcmTile *d_tiles, int n_tiles,
                    mp3s_pcm_frame_diff *d_frames, mp3s_pcm_pair_diff *d_out);

// the lag that aligns pairs of row runs of one int16 PCM buffer [row][nch] and their exact difference at it (k_pcmalign.hpp): pass 1
// (k_pcm_lag_scores, only without d_given: d_scores[n_pairs][2 max_lag + 1]), pass 2 (k_pcm_lag_pick: d_lags, and d_geo for what
// follows), pass 3 (k_pcm_diff_lagged: a record per chunk of 1152 rows of the overlap) and k_pcm_diff_pairs over d_geo.  d_tiles is
// pcm_diff_tiles of pcm_align_bound_pairs: pass 3's grid stands on the bound ceil(min(a_rows, b_rows) / 1152) chunks a pair, which
// holds for every lag.  d_pcm must be 16-byte aligned.
constexpr int kPcmMaxLag = MP3S_PCM_MAX_LAG;
int launch_pcm_align(hipStream_t stream, const int16_t *d_pcm, int nch, const mp3s_pcm_run_pair *d_runs, int n_pairs, int max_lag, int search_rows,
                     const int32_t *d_given, const PcmTile *d_tiles, int n_tiles, uint64_t *d_scores, mp3s_pcm_lag *d_lags, mp3s_pcm_pair *d_geo,
                     mp3s_pcm_frame_diff *d_frames, mp3s_pcm_pair_diff *d_out);
// appends per run pair the mp3s_pcm_pair whose n_frames is that bound (the other fields 0): what pcm_diff_tiles takes
template <class Pairs>
void pcm_align_bound_pairs(const mp3s_pcm_run_pair *runs, int n_pairs, Pairs &pairs)
{
    for (int p = 0; p < n_pairs; p++) {
        const uint32_t rows = runs[p].a_rows < runs[p].b_rows ? runs[p].a_rows : runs[p].b_rows;
        pairs.push_back(mp3s_pcm_pair{0, 0, (uint32_t)(((uint64_t)rows + 1151) / 1152), 0});
    }
}

// PCM batches in the caller's device memory (k_pcmbatch.hpp; the rules: include/mp3s.h, vi-f).  Both kernels take kPcmBatchThreads lanes
// to a workgroup and find their item and their tile inside it in d_tiles, which the host makes (n_tiles = the grid).
//   k_pcm_batch:   a lane owns 8 elements of a plane, counted from the 16-byte boundary in front of the plane's first element: an item
//                  has up to ceil((T + 7) / 8) such groups a plane, whatever its n_rows is (the padding is written too)
//   k_pcm_unbatch: a lane owns 4 rows of an item's ceil(n_rows / 1152) frames
constexpr int kPcmBatchThreads = 256;
struct PcmBatchTile { uint32_t item, first; };   // 8 bytes: lanes [first * kPcmBatchThreads, + kPcmBatchThreads) of item `item`
// appends the tiles of n_items items of a batch of T elements a plane (anything with push_back); false: more tiles than a grid takes
template <class Tiles>
bool pcm_batch_tiles(int n_items, int64_t T, Tiles &tiles)
{
    if (n_items <= 0 || T <= 0 || T > ((int64_t)1 << 40)) return false;
    const uint64_t groups = ((uint64_t)T + 6) / 8 + 1, per = (groups + kPcmBatchThreads - 1) / kPcmBatchThreads;
    if ((uint64_t)tiles.size() + per * (uint64_t)n_items > 0x7fffffffu) return false;
    for (int i = 0; i < n_items; i++)
        for (uint64_t f = 0; f < per; f++) tiles.push_back(PcmBatchTile{(uint32_t)i, (uint32_t)f});
    return true;
}
// ... of the items of an unbatch launch, from their row counts (each >= 1)
template <class Tiles>
bool pcm_unbatch_tiles(const mp3s_pcm_unbatch_item *items, int n_items, Tiles &tiles)
{
    uint64_t n = tiles.size();
    for (int i = 0; i < n_items; i++) {
        if (items[i].n_rows < 1 || items[i].n_rows > ((int64_t)1 << 40)) return false;
        n += (((uint64_t)items[i].n_rows + 1151) / 1152 * 288 + kPcmBatchThreads - 1) / kPcmBatchThreads;
    }
    if (n > 0x7fffffffu) return false;
    for (int i = 0; i < n_items; i++) {
        const uint64_t per = (((uint64_t)items[i].n_rows + 1151) / 1152 * 288 + kPcmBatchThreads - 1) / kPcmBatchThreads;
        for (uint64_t f = 0; f < per; f++) tiles.push_back(PcmBatchTile{(uint32_t)i, (uint32_t)f});
    }
    return true;
}
// what a launch needs of its items beside the tiles: true when every record is one the kernels may follow
inline bool pcm_batch_items_ok(const mp3s_pcm_batch_item *items, int n_items)
{
    for (int i = 0; i < n_items; i++)
        if (items[i].src_row < 0 || items[i].n_rows < 0 || items[i].first_row < 0 || items[i].slot < 0 || items[i].src_row > INT64_MAX / 4 - items[i].first_row) return false;
    return true;
}
inline bool pcm_unbatch_items_ok(const mp3s_pcm_unbatch_item *items, int n_items, int64_t T)
{
    for (int i = 0; i < n_items; i++)
        if (items[i].dst_frame < 0 || items[i].dst_frame > 0x7fffffff || items[i].n_rows < 1 || items[i].n_rows > T || items[i].slot < 0) return false;
    return true;
}
// d_pcm: int16 rows of nch samples, aligned to a row; d_out: [slots][out_channels][T] int16 or float32, aligned to an element
int launch_pcm_batch(hipStream_t stream, const int16_t *d_pcm, int nch, const mp3s_pcm_batch_item *d_items, const PcmBatchTile *d_tiles, int n_tiles,
                     int out_channels, int out_format, int64_t T, void *d_out);
// d_in: [slots][in_channels][T], aligned to an element; d_pcm: [frames][1152][2] int16, 16-byte aligned
int launch_pcm_unbatch(hipStream_t stream, const void *d_in, int in_channels, int in_format, int64_t T, const mp3s_pcm_unbatch_item *d_items,
                       const PcmBatchTile *d_tiles, int n_tiles, int16_t *d_pcm);

// QMDCT on the device (k_qmdct.hpp; the rules: include/mp3s.h, vi-g).
//   k_qmdct_features: one workgroup per (entry of d_tiles, channel): slice `slice` (kQmdctSlice granule rows) of stream `seg` of d_segs.
//                     A stream of 0 frames has one entry too: its slice 0 writes the record's tail.  The launcher clears d_out [n_segs]
//                     on the stream in front of the kernel, which adds into it.
//   k_qmdct_batch:    a lane owns one 16-byte piece of a slot's out_channels * Gt rows of 72 pieces; item and tile from d_tiles
//                     (PcmBatchTile: lanes [first * kPcmBatchThreads, + kPcmBatchThreads) of item `item`).
constexpr int kQmdctSlice = MP3S_QMDCT_SLICE;
constexpr int64_t kQmdctMaxRows = (int64_t)1 << 24;   // Gt of a batch
struct QmdctTile { uint32_t seg, slice; };   // 8 bytes
// appends the entries of segs[0 .. n_segs) (anything with push_back); false: more than a grid takes
template <class Tiles>
bool qmdct_feature_tiles(const mp3s_table_audit_seg *segs, int n_segs, Tiles &tiles)
{
    uint64_t n = tiles.size();
    for (int s = 0; s < n_segs; s++) n += segs[s].n_frames <= 0 ? 1 : ((uint64_t)2 * (uint64_t)segs[s].n_frames + kQmdctSlice - 1) / kQmdctSlice;
    if (n > 0x7fffffffu) return false;
    for (int s = 0; s < n_segs; s++) {
        const uint64_t per = segs[s].n_frames <= 0 ? 1 : ((uint64_t)2 * (uint64_t)segs[s].n_frames + kQmdctSlice - 1) / kQmdctSlice;
        for (uint64_t k = 0; k < per; k++) tiles.push_back(QmdctTile{(uint32_t)s, (uint32_t)k});
    }
    return true;
}
// ... of n_items items of a batch of Gt rows a plane
template <class Tiles>
bool qmdct_batch_tiles(int n_items, int out_channels, int64_t Gt, Tiles &tiles)
{
    if (n_items <= 0 || out_channels < 1 || out_channels > 2 || Gt <= 0 || Gt > kQmdctMaxRows) return false;
    const uint64_t per = ((uint64_t)out_channels * (uint64_t)Gt * 72 + kPcmBatchThreads - 1) / kPcmBatchThreads;
    if ((uint64_t)tiles.size() + per * (uint64_t)n_items > 0x7fffffffu) return false;
    for (int i = 0; i < n_items; i++)
        for (uint64_t f = 0; f < per; f++) tiles.push_back(PcmBatchTile{(uint32_t)i, (uint32_t)f});
    return true;
}
inline bool qmdct_batch_items_ok(const mp3s_qmdct_batch_item *items, int n_items)
{
    for (int i = 0; i < n_items; i++)
        if (items[i].src_frame < 0 || items[i].n_frames < 0 || items[i].first_granule < 0 || items[i].slot < 0 || items[i].src_frame > 0x7fffffff ||
            items[i].n_frames > 0x7fffffff || items[i].first_granule > ((int64_t)1 << 40))
            return false;
    return true;
}
// d_is: 4-byte aligned; d_out: [n_segs], 8-byte aligned
int launch_qmdct_features(hipStream_t stream, const int16_t *d_is, int nch, const mp3s_table_audit_seg *d_segs, int n_segs, const QmdctTile *d_tiles,
                          int n_tiles, int n_lines, mp3s_qmdct_features *d_out);
// d_is and d_out: 16-byte aligned; d_out [slots][out_channels][Gt][576] int16
int launch_qmdct_batch(hipStream_t stream, const int16_t *d_is, int nch, const mp3s_qmdct_batch_item *d_items, const PcmBatchTile *d_tiles, int n_tiles,
                       int out_channels, int64_t Gt, int16_t *d_out);

// WAV bytes -> int16 PCM frames of an encode batch (k_wav.hpp): per stream the byte offset of its first sample in the image (any
// alignment), its first frame in the batch and its frames.  d_image needs kWavSlack readable bytes behind the last sample taken.
struct WavRun { uint64_t src; uint32_t first_frame, n_frames; };   // 16 bytes
// ... and of k_wav_import: a stream of any sample format (MP3S_WAV_*) and one or two channels; n_samples per channel are taken, the rest
// of its n_frames frames is zero
struct WavImportRun { uint64_t src, n_samples; uint32_t first_frame, n_frames, format, channels; };   // 32 bytes
constexpr size_t kWavSlack = 64;   // k_wav_gather reads up to 31 bytes behind the last sample taken, k_wav_import up to 40 (k_wav.hpp)
// ... and of k_wav_resample (k_resample.hpp, MP3S_OPT_WAV_RESAMPLE): a stream whose n_in rows k_wav_import has laid as [L | R] dwords from dword
// src_row of a scratch buffer; n_out rows are computed into its n_frames frames of the batch, the rest of them is zero.  taps: the packed
// table of the ratio on the device (pack_resample_taps), span: the input rows a tile of kResTile output rows stages (resample_span)
struct WavResampleRun { const uint32_t *taps; uint64_t src_row, n_in, n_out; uint32_t first_frame, n_frames, L, M, T, span, mono, taps_lds; };   // 64 bytes
constexpr int kResTile = 1024;          // output rows of a tile: four per lane, one 16-byte store
constexpr uint32_t kResTapsLds = 2048;  // tap pairs (dwords) of a table that is staged in LDS; a larger one is read through the cache
inline uint32_t resample_span(uint32_t L, uint32_t M, uint32_t T) { return (uint32_t)(((uint64_t)(kResTile - 1) * M + L - 1) / L) + T; }
int launch_wav_resample(hipStream_t stream, const uint32_t *d_rows, const WavResampleRun *d_runs, int n_runs, int max_frames /* of one run */,
                        size_t lds_bytes /* the largest (span + staged tap pairs) * 4 of the runs */, int16_t *d_pcm, Profiler *prof);
// ... and of k_pcm_batch_resample (k_pcmresample.hpp; the rules: include/mp3s.h, mp3s_pcm_batch_resample_dev): k_pcm_batch with that FIR in
// front.  An item's n_in rows (nch int16 each) from row src_row of the decode's PCM become n_out rows at L / M, of which the window from
// first_row on goes into the item's slot.  T = 0 (L = M = 1): a copy, taps unused.  span: the input rows a tile stages.  One workgroup per
// PcmBatchTile; a tile owns kPcmResGroups groups of 8 elements of each output plane (lanes [0, 128) store plane 0, the others plane 1)
// and computes the kPcmResRows window rows they can lie in.
struct PcmResampleRun { const uint32_t *taps; int64_t src_row, n_in, n_out, first_row; uint32_t L, M, T, span, taps_lds, mono; int32_t slot; uint32_t pad; };   // 72 bytes
constexpr int kPcmResGroups = 128, kPcmResRows = 8 * kPcmResGroups + 8;
inline uint32_t pcm_resample_span(uint32_t L, uint32_t M, uint32_t T) { return T ? (uint32_t)(((uint64_t)(kPcmResRows - 1) * M + L - 1) / L) + T : (uint32_t)kPcmResRows; }
// dynamic LDS of a launch that holds this run: the computed rows, the staged span and the staged tap pairs
inline size_t pcm_resample_lds(const PcmResampleRun &r) { return ((size_t)kPcmResRows + r.span + (r.taps_lds ? (size_t)r.L * (r.T / 2) : 0)) * 4; }
// appends the tiles of n_items items of a batch of T elements a plane; false: more tiles than a grid takes
template <class Tiles>
bool pcm_resample_tiles(int n_items, int64_t T, Tiles &tiles)
{
    if (n_items <= 0 || T <= 0 || T > ((int64_t)1 << 40)) return false;
    const uint64_t groups = ((uint64_t)T + 6) / 8 + 1, per = (groups + kPcmResGroups - 1) / kPcmResGroups;
    if ((uint64_t)tiles.size() + per * (uint64_t)n_items > 0x7fffffffu) return false;
    for (int i = 0; i < n_items; i++)
        for (uint64_t f = 0; f < per; f++) tiles.push_back(PcmBatchTile{(uint32_t)i, (uint32_t)f});
    return true;
}
// lds_bytes: the largest pcm_resample_lds of the runs
int launch_pcm_batch_resample(hipStream_t stream, const int16_t *d_pcm, int nch, const PcmResampleRun *d_runs, const PcmBatchTile *d_tiles, int n_tiles,
                              size_t lds_bytes, int out_channels, int out_format, int64_t T, void *d_out);
int launch_wav_import(hipStream_t stream, const uint8_t *d_image, const WavImportRun *d_runs, int n_runs, int max_frames /* of one run */, int16_t *d_pcm);
int launch_wav_gather(hipStream_t stream, const uint8_t *d_image, const WavRun *d_runs, int n_runs, int max_frames /* of one run */, int16_t *d_pcm);

// a frame the host decoded (the last frame of a stream: E14) on its way into the Huffman outputs: k_place_frames copies is / si to frame `frame`
struct PlaceEntry { int32_t frame; int32_t pad[3]; int16_t is[2304]; mp3s_granule_si si[4]; };
static_assert(sizeof(PlaceEntry) == 4912 && offsetof(PlaceEntry, is) == 16 && offsetof(PlaceEntry, si) == 16 + 4608, "k_place_frames copies dwords from byte 16 on");
// the ONE way an entry is written on the host: its head, then decode(is, si) -> true: the entry is to be used
template <class Decode>
static inline bool fill_place_entry(PlaceEntry &e, int32_t frame, Decode &&decode) { e.frame = frame; e.pad[0] = e.pad[1] = e.pad[2] = 0; return decode(e.is, e.si); }
int launch_place_frames(hipStream_t stream, const uint8_t *d_entries, int n_entries, int16_t *d_is, mp3s_granule_si *d_si);
int launch_copy(hipStream_t stream, const void *d_src, void *d_dst, size_t bytes);
// one wave that occupies its hardware queue for about `microseconds`; a kernel that does nothing
int launch_spin(hipStream_t stream, int microseconds);
int launch_noop(hipStream_t stream);

// bit-level stages on the device
int launch_huffman(hipStream_t stream, const uint8_t *d_blob, const mp3s_frame_side *d_side, int n_frames, int nch, int max_bits,
                   int16_t *d_is, mp3s_granule_si *d_si, int32_t *d_status, int32_t *d_sync /* one zeroed 64-bit word owned by the context (k_sync.hpp) */,
                   Profiler *prof,
                   bool per_frame = false /* d_status holds 1 + n_frames words: [0] = all, [1 + f] = frame f */,
                   int lanes_opt = 0 /* MP3S_OPT_HUF_LANES: 0 = from the launch's size */);
// the tables every entry of a compact == 2 launch took, one byte each
int launch_gather_tables(hipStream_t stream, const mp3s_gr_out *d_outv, int n, uint8_t *d_tables);
// pairs: int32 [n][2] = (entry, unit): entry's ix / energies / GrInfo (compact == 2 arrays) -> the unit's place
int launch_scatter(hipStream_t stream, const int32_t *d_pairs, int n_pairs, const int16_t *d_ixv, const int32_t *d_env,
                   const mp3s_gr_out *d_outv, int16_t *d_ix, int32_t *d_en, mp3s_gr_out *d_out);
int launch_pack(hipStream_t stream, const int16_t *d_ix, const mp3s_gr_out *d_gr, const int32_t *d_en, int n_frames, int sri,
                int bri, int whole_slots, const uint32_t *d_frame_off, const uint8_t *d_padding, uint8_t *d_mp3,
                int32_t *d_scfsi, int32_t *d_status, int32_t *d_sync /* one zeroed 64-bit word owned by the context (k_sync.hpp) */, Profiler *prof,
                int f_begin = 0, int f_end = -1 /* frames [f_begin, f_end) only (f_end < 0: to the end); with d_sync == null only:
                                                   the arrival counter hands out ONE launch's bits */);

}  // namespace mp3s
