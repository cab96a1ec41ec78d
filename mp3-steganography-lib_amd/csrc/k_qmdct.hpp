// QMDCT on the device (gfx950): Markov / histogram features of Huffman-decoded streams, and the spectra themselves as a batch in the
// caller's memory.  Included by mp3s_device.hip only, behind k_wave.hpp.  The definitions are include/mp3s.h, section (vi-g).
//
//   k_qmdct_features : one workgroup per (stream, slice of QM_SLICE granule rows, channel) -- the (stream, slice) from a table the host
//                      made (QmdctTile), the channel from blockIdx.y --, so one file of 10 000 frames is 626 workgroups and not two.
//                      The slice's rows are dealt to the four waves in runs of QM_SLICE / 4 consecutive rows; a wave walks its run
//                      with a window of three rows in registers (g, g + 1, g + 2: the inter terms whose first row is g), so a row is
//                      fetched once per wave that needs it and the two rows behind a run come from the cache the next wave filled.
//                        * A row is 288 dwords (two lines each); lane l holds dwords l, l + 64, ... l + 256 (the last for l < 32):
//                          five coalesced dword loads a row.  The right-hand neighbours k + 1, k + 2 of the current row come from a
//                          second, OVERLAPPING load of dword d + 1 (same cache lines, no cross-lane step and no wave-edge case); it
//                          is issued one row ahead together with the window's next row, under the counting of the row in front.
//                        * Most lines of real spectra are zero: hist[0], intra[T][T] and inter[T][T] take the bulk of the increments.
//                          Those three are counted in LANE-PRIVATE registers (a compare and an add with carry) and reduced once per wave
//                          (wave_add3); only the other bins go through LDS atomics, into counters the wave has to itself
//                          (QM_BINS dwords a wave).  A 32-bit counter cannot wrap inside a slice (static_assert below).
//                        * After a barrier thread b adds the four waves' counts of bin b and sends a non-zero sum to the record with ONE
//                          64-bit integer atomic (max_abs / bandwidth: an atomic maximum).  The launcher clears the records on the
//                          stream in front; slice 0 of channel 0 writes the record's tail.  Integer sums: any order, the same bytes.
//                      No scratch, no spill.
//   k_qmdct_batch    : a streaming copy with a change of layout, the shape of k_pcm_batch: a lane owns one 16-byte piece (8 lines) of
//                      one output row, a row is 72 pieces, a slot C * Gt rows; item and tile from the host's table (PcmBatchTile).
//                      Rows behind `valid` and plane 1 of a mono item are written as zero.  One writer per element, nothing to clear.
#pragma once

namespace mp3s {

constexpr int QM_T = MP3S_QMDCT_T, QM_B = 2 * QM_T + 1;
constexpr int QM_SLICE = kQmdctSlice, QM_WAVES = 4, QM_RUN = QM_SLICE / QM_WAVES;
constexpr int QM_ND = 5;                                   // dwords of a row per lane
constexpr int QM_HIST = 0, QM_INTRA = 16, QM_INTER = QM_INTRA + QM_B * QM_B, QM_MAX = QM_INTER + QM_B * QM_B, QM_BW = QM_MAX + 1;
constexpr int QM_BINS = QM_BW + 1;                         // int64 words of an mp3s_qmdct_channel
constexpr int QM_MID = QM_T * QM_B + QM_T;                 // (T, T): both differences zero
static_assert(QM_BINS * 8 == sizeof(mp3s_qmdct_channel) && sizeof(mp3s_qmdct_features) == 2 * QM_BINS * 8 + 24, "the record is 180 words a channel");
static_assert(QM_SLICE % QM_WAVES == 0 && (uint64_t)QM_SLICE * 576 < ((uint64_t)1 << 32), "a 32-bit counter holds a slice");
static_assert(QM_BINS <= QM_WAVES * 64, "one thread per bin");

__device__ __forceinline__ int qm_abs_lo(uint32_t w) { const int x = (int)(w << 16) >> 16; return x < 0 ? -x : x; }
__device__ __forceinline__ int qm_abs_hi(uint32_t w) { const int x = (int)w >> 16; return x < 0 ? -x : x; }
__device__ __forceinline__ int qm_clamp(int d) { return min(max(d, -QM_T), QM_T) + QM_T; }

__global__ __launch_bounds__(QM_WAVES * 64) void k_qmdct_features(
    const int16_t *__restrict__ is /* [n_frames][2 gr][2 ch][576] */, const mp3s_table_audit_seg *__restrict__ segs,
    const QmdctTile *__restrict__ tiles, int nch, int K, mp3s_qmdct_features *__restrict__ out)
{
    __shared__ uint32_t cnt[QM_WAVES][QM_BINS];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const QmdctTile tile = tiles[blockIdx.x];
    const int c = (int)blockIdx.y;
    const mp3s_table_audit_seg sg = segs[tile.seg];
    const int G = 2 * sg.n_frames;
    const int s0 = (int)tile.slice * QM_SLICE, s1 = min(s0 + QM_SLICE, G);
    mp3s_qmdct_features *rec = out + tile.seg;
    if (tile.slice == 0 && c == 0 && tid == 0) {
        rec->n_frames = sg.n_frames; rec->channels = nch; rec->sampling_rate = 0; rec->kbps = 0; rec->n_lines = K; rec->reserved = 0;
    }
    for (int b = lane; b < QM_BINS; b += 64) cnt[wave][b] = 0;   // (the wave's own counters: its LDS operations keep their order)
    const int r0 = s0 + wave * QM_RUN, r1 = min(r0 + QM_RUN, s1);
    // row g of the channel: frame g >> 1, granule g & 1
    auto row_of = [&](int g) { return reinterpret_cast<const uint32_t *>(is + ((size_t)(sg.first_frame + (g >> 1)) * 4 + (size_t)((g & 1) * 2 + c)) * 576); };
    auto load_w = [&](int g, uint32_t (&w)[QM_ND]) {
        const uint32_t *p = row_of(g);
#pragma unroll
        for (int j = 0; j < QM_ND; j++) { const int d = lane + 64 * j; w[j] = (g < G && d < 288) ? p[d] : 0u; }
    };
    auto load_n = [&](int g, uint32_t (&n)[QM_ND]) {
        const uint32_t *p = row_of(g);
#pragma unroll
        for (int j = 0; j < QM_ND; j++) { const int d = lane + 64 * j; n[j] = (g < G && d < 287) ? p[d + 1] : 0u; }
    };
    uint32_t zero_h = 0, zero_i = 0, zero_v = 0, mx = 0, bw = 0;
    if (r0 < r1) {
        uint32_t w0[QM_ND], n0[QM_ND], w1[QM_ND], w2[QM_ND], wn[QM_ND], nn[QM_ND];
        load_w(r0, w0); load_n(r0, n0); load_w(r0 + 1, w1); load_w(r0 + 2, w2);
        for (int g = r0; g < r1; g++) {
            const bool more = g + 1 < r1;                 // (uniform)
            if (more) { load_n(g + 1, nn); load_w(g + 3, wn); }
            const bool pair_v = g + 2 < G;                // the inter term whose first row is g exists
#pragma unroll
            for (int j = 0; j < QM_ND; j++) {
                if (128 * j >= K) continue;               // (uniform: no counted line in this dword of any lane)
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int k = 2 * (lane + 64 * j) + h;
                    const int a0 = h ? qm_abs_hi(w0[j]) : qm_abs_lo(w0[j]);
                    const int a1 = h ? qm_abs_lo(n0[j]) : qm_abs_hi(w0[j]);
                    const int a2 = h ? qm_abs_hi(n0[j]) : qm_abs_lo(n0[j]);
                    const int b1 = h ? qm_abs_hi(w1[j]) : qm_abs_lo(w1[j]);
                    const int b2 = h ? qm_abs_hi(w2[j]) : qm_abs_lo(w2[j]);
                    const bool in = k < K;                // (k < 576 follows: K <= 576, and lanes past the row hold k >= 576)
                    if (in) {
                        const int v = min(a0, 15);
                        if (v == 0) zero_h++;
                        else atomicAdd(&cnt[wave][QM_HIST + v], 1u);
                        mx = max(mx, (uint32_t)a0);
                        if (a0) bw = max(bw, (uint32_t)k + 1);
                    }
                    if (k + 2 < K) {
                        const int idx = qm_clamp(a0 - a1) * QM_B + qm_clamp(a1 - a2);
                        if (idx == QM_MID) zero_i++;
                        else atomicAdd(&cnt[wave][QM_INTRA + idx], 1u);
                    }
                    if (in && pair_v) {
                        const int idx = qm_clamp(a0 - b1) * QM_B + qm_clamp(b1 - b2);
                        if (idx == QM_MID) zero_v++;
                        else atomicAdd(&cnt[wave][QM_INTER + idx], 1u);
                    }
                }
            }
            if (more) {
#pragma unroll
                for (int j = 0; j < QM_ND; j++) { w0[j] = w1[j]; n0[j] = nn[j]; w1[j] = w2[j]; w2[j] = wn[j]; }
            }
        }
    }
    wave_add3(zero_h, zero_i, zero_v);
    mx = wave_max_u32(mx); bw = wave_max_u32(bw);
    if (lane == 0) {
        atomicAdd(&cnt[wave][QM_HIST], zero_h); atomicAdd(&cnt[wave][QM_INTRA + QM_MID], zero_i); atomicAdd(&cnt[wave][QM_INTER + QM_MID], zero_v);
        cnt[wave][QM_MAX] = mx; cnt[wave][QM_BW] = bw;
    }
    __syncthreads();
    if (tid < QM_BINS) {
        unsigned long long *dst = reinterpret_cast<unsigned long long *>(&rec->ch[c]) + tid;
        if (tid < QM_MAX) {
            uint32_t s = 0;
#pragma unroll
            for (int w = 0; w < QM_WAVES; w++) s += cnt[w][tid];   // (at most QM_SLICE * 576: no wrap)
            if (s) atomicAdd(dst, (unsigned long long)s);
        } else {
            uint32_t s = 0;
#pragma unroll
            for (int w = 0; w < QM_WAVES; w++) s = max(s, cnt[w][tid]);
            if (s) atomicMax(dst, (unsigned long long)s);
        }
    }
}

template <int NCH, int C>
__global__ __launch_bounds__(kPcmBatchThreads) void k_qmdct_batch(
    const int16_t *__restrict__ is, const mp3s_qmdct_batch_item *__restrict__ items, const PcmBatchTile *__restrict__ tiles, int64_t Gt,
    int16_t *__restrict__ out)
{
    const PcmBatchTile tile = tiles[blockIdx.x];
    const mp3s_qmdct_batch_item it = items[tile.item];
    const int64_t left = 2 * it.n_frames - it.first_granule, valid = left < 0 ? 0 : (left > Gt ? Gt : left);
    const int64_t q = (int64_t)tile.first * kPcmBatchThreads + (int64_t)threadIdx.x;   // the lane's piece of the slot
    if (q >= (int64_t)C * Gt * 72) return;
    const int64_t row = q / 72, g = row % Gt;
    const int piece = (int)(q - row * 72), c = (int)(row / Gt);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (c < NCH && g < valid) {
        const int64_t sg = it.first_granule + g;
        v = *reinterpret_cast<const uint4 *>(is + ((it.src_frame + (sg >> 1)) * 4 + ((sg & 1) * 2 + c)) * 576 + piece * 8);
    }
    *reinterpret_cast<uint4 *>(out + (((int64_t)it.slot * C + c) * Gt + g) * 576 + piece * 8) = v;
}

}  // namespace mp3s
