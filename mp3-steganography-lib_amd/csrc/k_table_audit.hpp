// Table audit of a batch of Huffman-decoded streams on the device (gfx950).  Included by mp3s_device.hip only, behind k_rate.hpp
// (lin_bits_of, family_of) and k_wave.hpp.  The rule is spelled out in include/mp3s.h, section vi-e; in short: the reference's encoder
// makes a NATURAL choice of a region's code book from the region's values alone and lets a message bit transform it
// (__new_choose_table, encoder/MP3_Encoder.py:1170-1264, IDX_TO_TRANSFORM_HUF :419-449); a decoder sees the values exactly, so the
// natural choice is computed again here and every region is NATURAL, FORCED by a bit, FOREIGN or EMPTY.
//
//   k_table_audit_units   : one workgroup per frame, one WAVE per unit (wave ch * 2 + gr), no barrier, no LDS.  A lane holds five
//                           CONSECUTIVE pairs of the granule's 288 (lanes 0..57, as k_rate.hpp's RL_NP), one dword load each: the
//                           region of a pair is two compares against the wave-uniform bounds.  Per unit
//                             * the three region maxima in one wave_max3;
//                             * per region the two candidate books (13 / 15 below 15; the first adequate of 15..23 and of 24..31 above:
//                               linmax from the linbits constants of lin_bits_of, no table) and the named one -- wave-uniform;
//                             * per pair ONE look-up of the packed length word the rate loop uses (DevTables::rl_hl: the lengths under
//                               the four length tables, the non-zero count and the escape count of the pair) serves all nine bit
//                               counts -- three books for three regions -- which go through three wave_add3.
//                               The word is read from the constant segment with a per-lane index, i.e. as an ordinary cached vector
//                               load of a 2 KB table: five loads a lane and unit.  The rate loop keeps the same words in LDS because
//                               it reads them thousands of times a unit; here a copy per workgroup would cost more than the reads
//                               (256 loads, 256 LDS stores and a barrier for 1 280 look-ups);
//                             * lane 0 classifies and writes the unit's 16-byte record.
//   k_table_audit_streams : one workgroup per stream, one frame per thread, the stream's frames in tiles of TA_TILE with the running
//                           totals carried in registers (the shape of k_capacity): a thread reads its frame's four unit records (64
//                           bytes, four dwordx4 loads), counts the classes, and one scan of the frame's region count gives every
//                           region its index -- wave_scan_u32 in the wave, wave totals through LDS (two rows in turn: one barrier a
//                           tile).  The class sums travel as 16-bit fields (a tile holds at most 3 072 of a class), the first / last
//                           forced index of the tile as two keys under wave_max_u32.
//                           Every word written has one writer: ordinary vector stores, no atomics, no scratch.
#pragma once

namespace mp3s {

constexpr int TA_TILE = 256;                // frames of a tile = threads of k_table_audit_streams' workgroup
constexpr int TA_NP = 5;                    // pairs per lane, consecutive

// the first book of lo .. hi whose linmax reaches v; hi when none does (a value no stream can hold)
__device__ __forceinline__ int ta_first_book(int lo, int hi, int v)
{
    int c = hi;
    for (int i = hi - 1; i >= lo; i--)
        if ((1 << lin_bits_of(i)) - 1 >= v) c = i;
    return c;
}

// bits of a pair under book t (count_bit, MP3_Encoder.py:234-261) from its packed word; t in {13, 15 .. 31}
__device__ __forceinline__ uint32_t ta_pair_bits(uint32_t h, int fam, int lb)
{
    return ((h >> (5 * fam)) & 31u) + ((h >> 20) & 3u) + (uint32_t)lb * ((h >> 22) & 3u);
}

__global__ __launch_bounds__(256) void k_table_audit_units(
    const int16_t *__restrict__ is /* [n_frames][2 gr][2 ch][576] */, const mp3s_frame_side *__restrict__ side, int nch,
    mp3s_table_audit_unit *__restrict__ units /* [n_frames][4], unit ch * 2 + gr */)
{
    const int lane = (int)threadIdx.x & 63;
    const int u = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), ch = u >> 1, gr = u & 1;
    const size_t f = blockIdx.x;
    mp3s_table_audit_unit rec;
    rec.cls[0] = rec.cls[1] = rec.cls[2] = MP3S_TA_NONE; rec.forced_bits = 0;
    rec.nat[0] = rec.nat[1] = rec.nat[2] = 0; rec.window = 0;
    rec.excess[0] = rec.excess[1] = rec.excess[2] = 0; rec.reserved = 0;
    mp3s_table_audit_unit *const dst = units + f * 4 + u;
    if (ch >= nch) {                                      // (wave-uniform)
        if (lane == 0) *dst = rec;
        return;
    }
    const mp3s_frame_side *fs = side + f;
    const mp3s_unit_side *us = &fs->unit[gr][ch];
    const int t[3] = {us->table_select[0], us->table_select[1], us->table_select[2]};
    if (us->window_switching) {
        rec.window = 1;
        rec.cls[0] = t[0] ? MP3S_TA_FOREIGN : MP3S_TA_NONE;
        rec.cls[1] = t[1] ? MP3S_TA_FOREIGN : MP3S_TA_NONE;
        if (lane == 0) *dst = rec;
        return;
    }
    const int sr = min((int)fs->sr_idx, 2);
    const int bv = min((int)us->big_values, 288);
    const int i0 = min((int)us->region0_count + 1, 22), i1 = min((int)us->region0_count + (int)us->region1_count + 2, 22);
    const int a3 = 2 * bv, e1 = c_tab.sfb_long[sr][i0], e2 = c_tab.sfb_long[sr][i1];
    const int a1 = min(e1, a3), a2 = min(e2, a3);         // (all even: a pair lies in one region)
    // The encoder chose a book for regions 0 and 1 from every line up to e1 and e2 (__subdivide does not cut them at 2 bv), and the
    // lines behind the big values do not reach a decoder as the encoder held them: such a region is not judged
    const bool unseen[3] = {e1 > a3, e2 > a3, false};
    // ---- the lane's pairs: |x| | |y| << 16, their region (3: behind the big values), their packed length word
    const uint32_t *row = reinterpret_cast<const uint32_t *>(is + (f * 4 + (size_t)(gr * 2 + ch)) * 576);
    uint32_t mx[3] = {0, 0, 0}, h[TA_NP];
    int reg[TA_NP];
#pragma unroll
    for (int m = 0; m < TA_NP; m++) {
        const int p = lane * TA_NP + m, line = 2 * p;
        const uint32_t w = p < 288 ? row[p] : 0u;
        const int xs = (int)(int16_t)(w & 0xffffu), ys = (int)(int16_t)(w >> 16);
        const uint32_t x = (uint32_t)(xs < 0 ? -xs : xs), y = (uint32_t)(ys < 0 ? -ys : ys);
        const int r = line >= a3 ? 3 : (line >= a1) + (line >= a2);
        reg[m] = r;
        const uint32_t big = max(x, y);
#pragma unroll
        for (int q = 0; q < 3; q++) mx[q] = max(mx[q], r == q ? big : 0u);
        h[m] = c_tab.rl_hl[min(x, 15u) * 16 + min(y, 15u)][0];
    }
    wave_max3(mx[0], mx[1], mx[2]);
    // ---- per region: the two candidates, then the bits under both and under the named book
    int cand[3][2], fam[3][3], lb[3][3];
    bool named_ok[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const int mq = (int)mx[q];
        cand[q][0] = mq < 15 ? 13 : ta_first_book(15, 23, mq - 15);
        cand[q][1] = mq < 15 ? 15 : ta_first_book(24, 31, mq - 15);
        named_ok[q] = t[q] == 13 || (t[q] >= 15 && t[q] <= 31);
        const int book[3] = {cand[q][0], cand[q][1], named_ok[q] ? t[q] : 13};
#pragma unroll
        for (int k = 0; k < 3; k++) { fam[q][k] = family_of(book[k]); lb[q][k] = lin_bits_of(book[k]); }
    }
    uint32_t s[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};   // [region][candidate 0, candidate 1, named]
#pragma unroll
    for (int m = 0; m < TA_NP; m++)
#pragma unroll
        for (int q = 0; q < 3; q++)
            if (reg[m] == q) {
#pragma unroll
                for (int k = 0; k < 3; k++) s[q][k] += ta_pair_bits(h[m], fam[q][k], lb[q][k]);
            }
#pragma unroll
    for (int q = 0; q < 3; q++) wave_add3(s[q][0], s[q][1], s[q][2]);
    // ---- the classes (everything is wave-uniform by now; lane 0 writes)
#pragma unroll
    for (int q = 0; q < 3; q++) {
        if (!t[q]) continue;
        if (unseen[q] || !mx[q]) { rec.cls[q] = MP3S_TA_EMPTY; continue; }
        const bool second = mx[q] < 15 ? s[q][1] <= s[q][0] : s[q][1] < s[q][0];
        const int nat = second ? cand[q][1] : cand[q][0];
        const uint32_t nat_bits = second ? s[q][1] : s[q][0];
        rec.nat[q] = (uint8_t)nat;
        if (t[q] == nat) rec.cls[q] = MP3S_TA_NATURAL;
        else if (named_ok[q] && (t[q] == c_tab.transform[nat][0] || t[q] == c_tab.transform[nat][1])) {
            rec.cls[q] = MP3S_TA_FORCED;
            if (t[q] != c_tab.transform[nat][0]) rec.forced_bits |= (uint8_t)(1u << q);
            rec.excess[q] = (int16_t)((int)s[q][2] - (int)nat_bits);
        } else rec.cls[q] = MP3S_TA_FOREIGN;
    }
    if (lane == 0) *dst = rec;
}

__global__ __launch_bounds__(TA_TILE) void k_table_audit_streams(
    const mp3s_table_audit_unit *__restrict__ units, const mp3s_table_audit_seg *__restrict__ segs, int nch,
    mp3s_table_audit *__restrict__ out, uint32_t *__restrict__ profile /* [frames of the batch] or null */)
{
    constexpr int WAVES = TA_TILE / 64;
    __shared__ uint32_t w_tot[2][WAVES][7];               // wave totals, the tiles take the two rows in turn
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const mp3s_table_audit_seg sg = segs[blockIdx.x];
    const int first = sg.first_frame, n = sg.n_frames;    // (the same for the whole workgroup: every thread meets every barrier)
    uint64_t run[5] = {0, 0, 0, 0, 0};                    // natural, forced, foreign, empty, forced ones in front of the tile
    int64_t run_excess = 0;
    uint64_t run_regions = 0;
    uint32_t run_window = 0;
    int64_t first_forced = -1, last_forced = -1;
    int row = 0;
    for (int t0 = 0; t0 < n; t0 += TA_TILE, row ^= 1) {
        const int f = t0 + tid;
        uint32_t cnt[5] = {0, 0, 0, 0, 0};                // per class of the frame (index MP3S_TA_*)
        uint32_t ones = 0, excess = 0, window = 0, f_first = 0xffffu, f_last = 0, pos = 0;
        if (f < n) {
            const uint4 *q = reinterpret_cast<const uint4 *>(units + (size_t)(first + f) * 4);
            uint4 r[4];
#pragma unroll
            for (int k = 0; k < 4; k++) r[k] = q[k];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if ((k >> 1) >= nch) continue;
                window += (r[k].y >> 24) & 1u;
                const uint32_t fb = r[k].x >> 24;
                const int32_t ex[3] = {(int16_t)(r[k].z & 0xffffu), (int16_t)(r[k].z >> 16), (int16_t)(r[k].w & 0xffffu)};   // (signed)
#pragma unroll
                for (int g = 0; g < 3; g++) {
                    const uint32_t cl = (r[k].x >> (8 * g)) & 0xffu;
                    if (cl == MP3S_TA_NONE || cl > MP3S_TA_EMPTY) continue;
                    cnt[cl]++;
                    if (cl == MP3S_TA_FORCED) {
                        ones += (fb >> g) & 1u; excess += (uint32_t)ex[g];   // (two's complement: the sums wrap back)
                        f_first = min(f_first, pos); f_last = pos + 1;
                    }
                    pos++;
                }
            }
        }
        // ---- the frame's first region index: an inclusive scan of the region counts
        uint32_t sc = wave_scan_u32(pos);
        uint32_t a = cnt[MP3S_TA_NATURAL] | (cnt[MP3S_TA_FORCED] << 16), b = cnt[MP3S_TA_FOREIGN] | (cnt[MP3S_TA_EMPTY] << 16), c = ones | (window << 16);
        wave_add3(a, b, c);
        const uint32_t ex_w = wave_add_u32(excess);
        const uint32_t base_w = sc - pos;                 // regions of the wave's frames in front of this one
        // keys of the wave's first / last forced region, relative to the wave's first region: 0 = none
        const uint32_t k_first = wave_max_u32(f_last ? 0xffffu - (base_w + f_first) : 0u);
        const uint32_t k_last = wave_max_u32(f_last ? base_w + f_last : 0u);
        if (lane == 63) {
            uint32_t *w = w_tot[row][wave];
            w[0] = sc; w[1] = a; w[2] = b; w[3] = c; w[4] = ex_w; w[5] = k_first; w[6] = k_last;
        }
        __syncthreads();
        uint32_t tile_regions = 0, ta = 0, tb = 0, tc = 0, tex = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            const uint32_t *t = w_tot[row][w];
            if (t[6]) {                                   // wave w has a forced region; tile_regions = the regions in front of the wave
                const int64_t at = (int64_t)(run_regions + tile_regions);
                if (first_forced < 0) first_forced = at + (int64_t)(0xffffu - t[5]);
                last_forced = at + (int64_t)t[6] - 1;
            }
            tile_regions += t[0]; ta += t[1]; tb += t[2]; tc += t[3]; tex += t[4];
        }
        if (profile && f < n)
            profile[(size_t)first + f] = cnt[MP3S_TA_NATURAL] | (cnt[MP3S_TA_FORCED] << 4) | (cnt[MP3S_TA_FOREIGN] << 8) | (cnt[MP3S_TA_EMPTY] << 12);
        run[0] += ta & 0xffffu; run[1] += ta >> 16; run[2] += tb & 0xffffu; run[3] += tb >> 16; run[4] += tc & 0xffffu; run_excess += (int32_t)tex;
        run_window += tc >> 16; run_regions += tile_regions;
    }
    if (tid == 0) {
        mp3s_table_audit r;
        r.regions = (int64_t)run_regions; r.natural = (int64_t)run[0]; r.forced = (int64_t)run[1]; r.forced_ones = (int64_t)run[4];
        r.foreign = (int64_t)run[2]; r.empty = (int64_t)run[3]; r.excess_bits = run_excess;
        r.first_forced = first_forced; r.last_forced = last_forced;
        r.n_frames = n; r.channels = nch; r.sampling_rate = 0; r.kbps = 0; r.window_units = (int32_t)run_window; r.reserved = 0;
        r.profile = nullptr;
        out[blockIdx.x] = r;
    }
}

}  // namespace mp3s
