// Bit packing on the device (gfx950).  Included by mp3s_device.hip only.
//
//   k_enc_pack : __resv_frame_end + __format_bitstream (reference encoder/MP3_Encoder.py:1097-1145, 1266-1547) for
//                every frame of the batch.  The reference writes bits serially through a 32-bit cache; here the
//                position of every code word is known up front: a frame is exactly 8*(slots+padding) bits (all
//                slack becomes stuffing, E6), a granule*channel starts after the part2_3_lengths before it, and inside
//                it the offset of a pair is the prefix sum of the code lengths.  One workgroup per frame, one
//                wavefront per granule*channel, lane = 5 consecutive pairs, bits OR-ed into an LDS image of the frame.
//                A pair stays the dword x | y << 16 it is loaded as: |x|, |y|, the clamp to 15, the escape and sign fields and
//                their widths are packed 16-bit instructions on both halves at once.  What a pair is compared with (the region
//                starts, big_values, the end of count1) is wave-uniform, so a lane takes its distance to each bound once, as a
//                mask of six bits per pair below it, and picks the regions' words for its five pairs with two v_bfi; a pair that
//                emits nothing is cleared as a dword and needs no further case.  A lane's words are pushed into a 64-bit register
//                from below, one shift each, and leave as whole dwords of the image.
#pragma once

namespace mp3s {

constexpr int PACK_DW = 372;          // LDS image of one frame: 1441 bytes max (320 kbps @ 32 kHz) + slack
constexpr int PACK_FAM = 260;         // a book family's 256 words + 4: small values of different families (what a wave mostly reads at once) in different banks
constexpr int PACK_PT_QUAD = 4 * PACK_FAM, PACK_PT_NONE = PACK_PT_QUAD + 32, PACK_PT = PACK_PT_NONE + 1;   // the code-word table of k_enc_pack
#define MP3S_PS_OVERFLOW 1            // Huffman bits exceed part2_3_length (cannot happen for rate-loop output)
#define MP3S_PS_BAD_TABLE 2           // a code book this encoder never selects

__device__ __forceinline__ void lds_put(uint32_t *fb, uint32_t pos, uint32_t val, int n)
{
    if (n <= 0) return;
    const uint32_t d = pos >> 5, o = pos & 31;
    const uint64_t w = (uint64_t)val << (64 - o - n);
    atomicOr(&fb[d], (uint32_t)(w >> 32));
    if ((uint32_t)w) atomicOr(&fb[d + 1], (uint32_t)w);
}

// (mask & a) | (~mask & b): v_bfi_b32
__device__ __forceinline__ uint32_t pack_bfi(uint32_t mask, uint32_t a, uint32_t b) { return (mask & a) | (~mask & b); }

typedef uint16_t pk_u16 __attribute__((ext_vector_type(2)));
typedef int16_t pk_i16 __attribute__((ext_vector_type(2)));
// min(x, 1), min(y, 1) of a packed pair (written as a minimum the compiler turns it into two compares, two selects and a permute)
__device__ __forceinline__ pk_u16 pack_pk_min1(pk_u16 a)
{
    pk_u16 r;
    asm("v_pk_min_u16 %0, %1, 1 op_sel_hi:[1,0]" : "=v"(r) : "v"(a));
    return r;
}

// wave sum of a small non-negative value over the lanes selected by `on`
__device__ __forceinline__ int pack_wave_sum(int v, bool on) { return (int)wave_add_u32(on ? (uint32_t)v : 0u); }

// Persistent workgroups: the code tables are staged in LDS once, then the group walks frames f, f + gridDim.x, ...
// Everything the four waves need about the frame (part2_3_length after stuffing, start offsets) is wave-uniform
// scalar work done redundantly by each wave; the header / side info bits are written by the wave they describe.
__global__ __launch_bounds__(256) void k_enc_pack(
    const int16_t *__restrict__ ix, const mp3s_gr_out *__restrict__ gr, const int32_t *__restrict__ en, int n_frames,
    int sri, int bri, int whole_slots, const uint32_t *__restrict__ frame_off, const uint8_t *__restrict__ padding,
    uint8_t *__restrict__ mp3, int32_t *__restrict__ scfsi_out, int32_t *__restrict__ status, int32_t *__restrict__ sync,
    int f_begin /* frames [f_begin, n_frames) of the batch: a one-file call packs its last chunk in two launches, the first half on its way
                   down while the second is packed */)
{
    __shared__ uint32_t fb3[3][PACK_DW];   // frame images, rotating: written / being copied out / being cleared
    // code words of every kind in ONE table, code | length << 24 (a code has at most 19 bits): [book family][min(x,15)][min(y,15)] for the four
    // families of big-value books (13, 15, 16.., 24..), then the quadruples of count1 table A and B, then an empty word -- a pair picks its INDEX
    // (big value / first pair of a quadruple / nothing) and reads once; code and length used to come from two to four reads and as many selects
    __shared__ uint32_t pt[PACK_PT];
    __shared__ int wg_err;                 // the group's error bits
    const int wave0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane0 = threadIdx.x & 63;
    for (int i = threadIdx.x; i < 1024; i += 256) {
        const uint32_t len = i < 256 ? c_tab.hlen13[i] : (i < 512 ? c_tab.hlen15[i - 256] : (i < 768 ? c_tab.hlen16[i - 512] : c_tab.hlen24[i - 768]));
        pt[(i >> 8) * PACK_FAM + (i & 255)] = (&c_tab.hcod[0][0])[i] | (len << 24);
    }
    if (threadIdx.x < 16) {
        pt[PACK_PT_QUAD + threadIdx.x] = (uint32_t)c_tab.hcod_c1a[threadIdx.x] | ((uint32_t)c_tab.hlen_c1a[threadIdx.x] << 24);
        pt[PACK_PT_QUAD + 16 + threadIdx.x] = (15u - threadIdx.x) | (4u << 24);      // table B: four bits, the complement
    }
    if (threadIdx.x == 0) pt[PACK_PT_NONE] = 0;
    for (int i = threadIdx.x; i < 3 * PACK_DW; i += 256) (&fb3[0][0])[i] = 0;
    if (threadIdx.x == 0) wg_err = 0;
    __syncthreads();
    int rot = 0;
    for (int f = f_begin + blockIdx.x; f < n_frames; f += gridDim.x) {
    // The wave number and a copy of the lane number used ONLY in comparisons are made opaque once per frame: what follows from them is
    // invariant over the frame loop, and kept across it every lane predicate (lane < 22, lane == 0 ...) is a mask in two scalar
    // registers and every wave-derived scalar one more -- 71 scalar spills, read back lane by lane (v_readlane) in front of each use, a
    // fifth of the kernel's vector instructions.  A predicate recomputed is one comparison, a scalar recomputed is scalar arithmetic;
    // the lane number's ARITHMETIC (addresses, pair numbers) stays invariant and hoisted (made opaque too, round 4's first try, it cost
    // more than the spills).
    const int lane = lane0, tid = (int)threadIdx.x;
    int lane_p = lane0, wave = wave0;
    asm volatile("" : "+v"(lane_p), "+s"(wave));
    // One barrier per frame.  This frame's image is fb3[rot]; the image of the frame before last -- every thread
    // finished copying it out before the previous barrier -- is cleared now and is ready after this frame's barrier.
    uint32_t *fb = fb3[rot];
    {
        uint32_t *cl = fb3[rot == 2 ? 0 : rot + 1];
        for (int i = tid; i < PACK_DW; i += 256) cl[i] = 0;
    }
    const int pad = padding[f];
    // ---- __resv_frame_end (:1097-1145): all slack of the frame becomes stuffing; emission order e = gr*2 + ch
    int p23v[4];
    {
        const int bits_per_frame = 8 * (whole_slots + pad);
        const int mean_bits = (bits_per_frame - 288) / 2;
        int sum = 0;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            p23v[e] = __builtin_amdgcn_readfirstlane(gr[((long)f * 2 + (e & 1)) * 2 + (e >> 1)].part2_3_length);
            sum += p23v[e];
        }
        int stuffing = 2 * mean_bits - sum + ((mean_bits & 1) ? 1 : 0);
        if (stuffing < 0) stuffing = 0;
        if (stuffing) {
            if (p23v[0] + stuffing < 4095) p23v[0] += stuffing;
            else
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int extra = 4095 - p23v[e], now = extra < stuffing ? extra : stuffing;
                    p23v[e] += now; stuffing -= now;
                }
        }
    }
    const int e = wave, grn = e >> 1, ch = e & 1;
    const long u = ((long)f * 2 + ch) * 2 + grn;
    const mp3s_gr_out &g = gr[u];
    const int p23 = __builtin_amdgcn_readfirstlane(e == 0 ? p23v[0] : (e == 1 ? p23v[1] : (e == 2 ? p23v[2] : p23v[3])));   // this unit's, stuffing included
    if (wave < 2) {
        // ---- scfsi of channel `wave` (:861-892) from the band energies of its two granules: lane s holds band s
        const long u0 = ((long)f * 2 + wave) * 2, u1 = u0 + 1;
        int a = 0, tot21 = 0;
        if (lane_p < 22) {
            a = en[u0 * 22 + lane] - en[u1 * 22 + lane];
            a = a < 0 ? -a : a;
        }
        tot21 = __builtin_amdgcn_readlane(a, 21);
        // the five sums over lanes (all 21 bands; bands 0-5, 6-10, 11-15, 16-20) from ONE inclusive scan of the rows' 16 lanes + the row in
        // front: five wave reductions before
        int sc = lane_p < 21 ? a : 0;
        sc += __builtin_amdgcn_update_dpp(0, sc, 0x111, 0xf, 0xf, false);   // row_shr:1
        sc += __builtin_amdgcn_update_dpp(0, sc, 0x112, 0xf, 0xf, false);   // row_shr:2
        sc += __builtin_amdgcn_update_dpp(0, sc, 0x114, 0xf, 0xf, false);   // row_shr:4
        sc += __builtin_amdgcn_update_dpp(0, sc, 0x118, 0xf, 0xf, false);   // row_shr:8  (lane l: sum of its row's lanes up to l)
        const int row0 = __builtin_amdgcn_readlane(sc, 15);                 // bands 0..15
        const int p5 = __builtin_amdgcn_readlane(sc, 5), p10 = __builtin_amdgcn_readlane(sc, 10), q20 = __builtin_amdgcn_readlane(sc, 20);   // (q20: bands 16..20)
        const int tp = row0 + q20;
        int cond = 2 + (gr[u0].xrmax != 0) + (gr[u1].xrmax != 0);
        if (tot21 < 10) cond++;
        if (tp < 100) cond++;
        const int band_sum[4] = {p5, p10 - p5, row0 - p10, q20};
        uint32_t scbits = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int s0 = band_sum[b];
            const int v = (cond == 6 && s0 < 10) ? 1 : 0;
            scbits = (scbits << 1) | (uint32_t)v;
            if (lane_p == 0) scfsi_out[((long)f * 2 + wave) * 4 + b] = v;
        }
        if (lane_p == 0) {
            lds_put(fb, 44 + 4 * wave, scbits, 4);
            if (wave == 0) {
                // ---- frame header (:1281-1300): sync 11, version 2, layer 2, no CRC 1, bitrate 4, rate 2, padding 1, ext 1,
                //      mode 2, mode ext 2, copyright 1, original 1, emphasis 2;  main_data_begin 9 + private 3 stay zero
                const uint32_t h = (0x7ffu << 21) | (3u << 19) | (1u << 17) | (1u << 16) | ((uint32_t)bri << 12) |
                                   ((uint32_t)(sri % 3) << 10) | ((uint32_t)pad << 9) | (1u << 2);
                fb[0] = h;     // nothing else writes the first dword
            }
        }
    }
    {
        // ---- side info of this wave's granule*channel (:1305-1337), 59 bits at 52 + 59 e.  Its four fields are wave-uniform: the wave joins
        //      them to one string in scalar registers and cuts it into the three image dwords it can touch; lanes 0 .. 2 OR one each (four lanes
        //      used to pick a field, a width and a place by selects and put it with a 64-bit shift and two ORs)
        const uint32_t f0 = ((uint32_t)p23 << 9) | (uint32_t)g.big_values;                                            // 21 bits
        const uint32_t f1 = (((uint32_t)(g.quantizer_step + 210) & 0xff) << 5);                                           // 13: global_gain 8, scalefac_compress 4, window_switching 1
        const uint32_t f2 = ((uint32_t)g.table_select[0] << 10) | ((uint32_t)g.table_select[1] << 5) | (uint32_t)g.table_select[2];   // 15
        const uint32_t f3 = ((uint32_t)g.region0_count << 6) | ((uint32_t)g.region1_count << 3) | (uint32_t)g.count1table_select;     // 10: + preflag, scalefac_scale = 0
        const uint64_t top = ((((uint64_t)f0 << 38) | ((uint64_t)f1 << 25) | ((uint64_t)f2 << 10) | f3)) << 5;   // the string's first bit in bit 63
        const uint32_t at = 52 + 59 * (uint32_t)e, o = at & 31u;
        const uint64_t d01 = top >> o;
        const uint32_t d2 = (uint32_t)(((uint64_t)(uint32_t)top << 32) >> o);
        const uint32_t v = lane_p == 0 ? (uint32_t)(d01 >> 32) : (lane_p == 1 ? (uint32_t)d01 : d2);
        if (lane_p < 3) atomicOr(&fb[(at >> 5) + (uint32_t)lane], v);
    }

    // ---- main data of this wave's granule*channel (:1394-1446)
    const int ts0 = g.table_select[0], ts1 = g.table_select[1], ts2 = g.table_select[2], c1sel = g.count1table_select;
    uint32_t ustart = 288;
#pragma unroll
    for (int k = 0; k < 3; k++) ustart += k < e ? (uint32_t)p23v[k] : 0u;
    const int bvr = g.big_values, bv = bvr < 288 ? bvr : 288, c1 = g.count1;
    const int32_t *sfb = c_tab.sfb_long[sri];
    const int r1s = sfb[g.region0_count + 1], r2s = sfb[g.region0_count + 1 + g.region1_count + 1];
    // The lane's five pairs, two dwords x | y << 16 at a time: the addresses of lanes 57 (its last two pairs) to 63 lie behind the unit and
    // are pulled back into it; what such a lane reads there is no pair of its own and is cleared with the pairs behind count1 below.
    uint32_t w[5];
    {
        const char *xb0 = reinterpret_cast<const char *>(ix + u * 576);
        const int oa = lane * 20 < 1140 ? lane * 20 : 1140, ob = lane * 20 + 12 < 1144 ? lane * 20 + 12 : 1144;
        const uint32_t *xa = reinterpret_cast<const uint32_t *>(xb0 + oa), *xc = reinterpret_cast<const uint32_t *>(xb0 + ob);
        w[0] = xa[0]; w[1] = xa[1]; w[2] = xa[2]; w[3] = xc[0]; w[4] = xc[1];
    }
    // What differs between the regions is wave-uniform: six bits per region -- Huffman-length family (books 13, 15, 16.., 24..) |
    // linbits << 2 -- and "book in use".  Every bound a pair is compared with (region 1, region 2, big_values, the end of count1) is
    // wave-uniform too and the lane's pairs are consecutive, so the lane takes its DISTANCE to each bound once, as a mask of six bits
    // per pair below it (0 .. 5 pairs: a v_med3 and a shift), and picks the six bits of all five pairs with two v_bfi of the regions' words
    // repeated five times; "in use" likewise.  Per pair that leaves field extractions at compile-time positions where there were a
    // compare and a select per pair and bound.
    bool any_bad = false;
    uint32_t Wr[3], Ur[3];
    {
        const int tsr[3] = {ts0, ts1, ts2};
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const int ti = tsr[r];
            // family 0 for book 13, 1 for 15, 2 for every other book below 24, 3 from 24 on: two bits per book, read from a constant
            const uint32_t fam = (uint32_t)(0xffffaaaa62aaaaaaull >> (2 * (ti & 31))) & 3u;
            Wr[r] = (fam | ((uint32_t)lin_bits_of(ti) << 2)) * 0x01041041u;
            Ur[r] = ti ? 0x3fffffffu : 0u;
            // a book this encoder never selects, in a region that holds pairs
            const int lo = r == 0 ? 0 : (r == 1 ? r1s : r2s), hi = r == 0 ? r1s : (r == 1 ? r2s : 576);
            any_bad |= ti != 0 && ti != 13 && ti != 15 && ti < 16 && lo < 2 * bvr && lo < hi;
        }
    }
    const int l30 = lane * 30;
    auto below = [&](int bound) -> uint32_t {      // six bits for each of the lane's pairs in front of pair `bound`
        const int s = min(max(6 * bound - l30, 0), 30);
        return (1u << s) - 1u;
    };
    const int cend = bv + 2 * c1 < 288 ? bv + 2 * c1 : 288;
    const uint32_t M1 = below((r1s + 1) >> 1), M2 = below((r2s + 1) >> 1), MB = below(bv), ME = below(cend);
    const uint32_t P = pack_bfi(M1, Wr[0], pack_bfi(M2, Wr[1], Wr[2]));
    const uint32_t MU = pack_bfi(M1, Ur[0], pack_bfi(M2, Ur[1], Ur[2]));
    const uint32_t INS = pack_bfi(MB, MU, ME);      // pairs that emit anything: big values of a book in use, count1 pairs
    // a count1 quadruple starts at every second pair from big_values on: the lane's even or its odd pairs
    const uint32_t odd = 0u - (uint32_t)((lane ^ bv) & 1);
    const uint32_t quad_base = (uint32_t)(PACK_PT_QUAD + (c1sel ? 16 : 0));
    const int nb5 = bv - lane * 5;                   // pairs of the lane that are big values (compared with 0 .. 4)
#pragma unroll
    for (int k = 0; k < 5; k++) w[k] &= (uint32_t)__builtin_amdgcn_sbfe((int)INS, 6 * k, 1);
    // the low bits of the pairs' two values (two's complement: the low bit of |v| is the low bit of v), and of the pair behind the lane's
    // (the first pair of the lane above): a count1 quadruple is this pair + the next one
    uint32_t lowb[6];
#pragma unroll
    for (int k = 0; k < 5; k++) lowb[k] = w[k] & 0x00010001u;
    lowb[5] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lowb[0], 0x130, 0xf, 0xf, false);           // wave_shl:1
    uint32_t code0[5], code1[5]; int n0[5], n1[5];
    int tot = 0;
    // Both halves of a pair at once (packed 16-bit): |x|, |y| <= 8191 + 15.  The escape and sign bits (MP3_Encoder.py:1452-1500; books 13
    // and 15 have no linbits, so their value 15 emits none) are [x - 15 in lb bits][sign of x][y - 15 in lb bits][sign of y]; a value of 0
    // has no sign bit, one below 15 no escape bits: x - 15 saturates to 0, the width lb - 16 (15 - min(x, 15)) to 0.  The pair's own code
    // word -- its book's, or the quadruple's with the first pair of a quad (E13; :1502-1547), or none -- is one read of `pt`.
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const uint32_t lb = __builtin_amdgcn_ubfe(P, 6 * k + 2, 4), fam = __builtin_amdgcn_ubfe(P, 6 * k, 2);
        const pk_u16 c15 = {15, 15};
        const pk_u16 a = __builtin_bit_cast(pk_u16, __builtin_elementwise_abs(__builtin_bit_cast(pk_i16, w[k])));
        const pk_u16 cl = __builtin_elementwise_min(a, c15);
        const pk_u16 nz = pack_pk_min1(a);
        const pk_u16 lbs = {(uint16_t)lb, (uint16_t)lb};
        const pk_u16 wid = __builtin_elementwise_sub_sat(lbs, (c15 - cl) * (pk_u16){16, 16}) + nz;       // bits of x's and of y's field
        const pk_u16 fld = __builtin_elementwise_sub_sat(a, c15) * (pk_u16){2, 2} + (__builtin_bit_cast(pk_u16, w[k]) >> (pk_u16){15, 15});
        const uint32_t wu = __builtin_bit_cast(uint32_t, wid), fu = __builtin_bit_cast(uint32_t, fld);
        code1[k] = ((fu & 0xffffu) << (wu >> 16)) | (fu >> 16);
        n1[k] = (int)((wu & 0xffffu) + (wu >> 16));
        const uint32_t big = __builtin_amdgcn_udot2(cl, (pk_u16){16, 1}, fam * (uint32_t)PACK_FAM, false);
        const uint32_t q = __builtin_amdgcn_udot2(__builtin_bit_cast(pk_u16, lowb[k + 1]), (pk_u16){4, 8},
                                                  __builtin_amdgcn_udot2(__builtin_bit_cast(pk_u16, lowb[k]), (pk_u16){1, 2}, quad_base, false), false);
        const uint32_t qn = pack_bfi((k & 1) ? ~odd : odd, (uint32_t)PACK_PT_NONE, q);
        const uint32_t word = pt[k < nb5 ? big : qn] & (uint32_t)__builtin_amdgcn_sbfe((int)INS, 6 * k, 1);
        code0[k] = word & 0xffffffu;
        n0[k] = (int)(word >> 24);
        tot += n0[k] + n1[k];
    }
    // exclusive prefix of the lanes' bit counts
    const int incl = (int)wave_scan_u32((uint32_t)tot);
    const int huff_bits = __builtin_amdgcn_readlane(incl, 63);
    // The lane's code words are consecutive in the stream: they are gathered at the low end of a 64-bit register, each pushed in from
    // below with ONE 64-bit shift, and leave as dwords of the frame image.  A word has at most 28 bits and fewer than 32 are pending, so
    // the register never loses a bit that has not left; what has left stays above the pending bits and is never read again.  After every
    // word one OR goes to the image, without a branch: the dword the word completed (a funnel shift takes it from the register), or
    // zero where the word did not reach a boundary; position and count move on by arithmetic.
    if (tot) {   // (the lanes behind the last value hold nothing and all stand on ONE dword: 64 ORs of zero into one address, eleven times)
        uint32_t pos = ustart + (uint32_t)(incl - tot);                         // the lane's place in the frame, in bits: pos & 31 bits are pending
        uint32_t d = pos >> 5;                                                  // (bits of another lane in front of the lane's first: zero here)
        uint64_t acc = 0;
        auto append = [&](uint32_t v, int n) {
            acc = (acc << (uint32_t)n) | v;
            pos += (uint32_t)n;
            const uint32_t full = __builtin_amdgcn_alignbit((uint32_t)(acc >> 32), (uint32_t)acc, pos);   // (the shift is pos & 31: those stay pending)
            const uint32_t dn = pos >> 5;                                       // d or d + 1
            atomicOr(&fb[d], dn != d ? full : 0u);
            d = dn;
        };
#pragma unroll
        for (int k = 0; k < 5; k++) { append(code0[k], n0[k]); append(code1[k], n1[k]); }
        atomicOr(&fb[d], __builtin_amdgcn_alignbit((uint32_t)acc, 0u, pos));     // what the last word left behind a dword boundary
    }
    // stuffing with ones up to part2_3_length (:1433-1446)
    if (huff_bits > p23 || any_bad) { if (lane_p == 0) atomicOr(&wg_err, any_bad ? MP3S_PS_BAD_TABLE : MP3S_PS_OVERFLOW); }   // (LDS)
    else {
        // the ones are bits [s0, s1) of the image: a lane takes a DWORD of it and ORs the ones that fall into that dword, one OR and no 64-bit
        // shift (a lane used to take 32 bits from wherever the codes ended: two dwords each)
        const uint32_t s0 = ustart + (uint32_t)huff_bits, s1 = ustart + (uint32_t)p23;
        for (uint32_t j = (s0 >> 5) + (uint32_t)lane; 32u * j < s1; j += 64u) {
            const uint32_t a = s0 > 32u * j ? s0 - 32u * j : 0u;                        // 0 .. 31: the first one of the dword, counted from its top
            const uint32_t b = s1 - 32u * j < 32u ? s1 - 32u * j : 32u;                 // 1 .. 32: behind the last one
            atomicOr(&fb[j], (0xffffffffu >> a) & ~(0x7fffffffu >> (b - 1u)));
        }
    }
    __syncthreads();
    // ---- LDS image -> global bytes: unaligned head / tail as bytes, the aligned interior as dwords
    const int nbytes = whole_slots + pad;
    const uint32_t off = frame_off[f];
    auto byte_at = [&](int k) -> uint32_t { return (fb[k >> 2] >> (24 - 8 * (k & 3))) & 0xffu; };
    const int head = (int)((4u - (off & 3u)) & 3u) < nbytes ? (int)((4u - (off & 3u)) & 3u) : nbytes;
    const int n_dw = (nbytes - head) >> 2, tail0 = head + 4 * n_dw;
    if (tid < head) mp3[off + tid] = (uint8_t)byte_at(tid);
    uint32_t *outw = reinterpret_cast<uint32_t *>(mp3 + off + head);
    {
        // bytes head + 4j .. + 3 of the image (big-endian in its dwords) as one little-endian dword: a funnel shift over two image
        // dwords and a byte swap (byte by byte it was two dozen instructions per dword)
        const int hq = head >> 2, hs = 8 * (head & 3);               // (wave-uniform)
        for (int j = tid; j < n_dw; j += 256) {
            const uint32_t hi = fb[hq + j], lo = fb[hq + j + 1];     // (PACK_DW leaves slack behind the last byte)
            const uint32_t be = hs ? __builtin_amdgcn_alignbit(hi, lo, 32 - hs) : hi;
            outw[j] = __builtin_bswap32(be);
        }
    }
    if (tid < nbytes - tail0) mp3[off + tail0 + tid] = (uint8_t)byte_at(tail0 + tid);
    rot = rot == 2 ? 0 : rot + 1;
    }   // frames
    // The caller's status word is written once, by the workgroup that finishes last, from the context's 64-bit word {finished
    // groups | error bits} (k_sync.hpp: one atomic per group, no fill kernel in front of every launch).
    // sync == null: the caller has zeroed *status itself (the overlapped stages, where the word travels with the job's inputs): two
    // thousand arrivals on one counter are 0.1 ms of serialised atomics when the groups finish together, as they do on a short batch.
    __syncthreads();
    if (threadIdx.x != 0) return;
    const int g = wg_err;
    if (!sync) {
        if (g) atomicOr(status, g);
        return;
    }
    unsigned all;
    if (arrive_with_bits(sync, (unsigned)g, gridDim.x, &all)) *status = (int32_t)all;
}

}  // namespace mp3s
