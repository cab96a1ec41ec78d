// Stego bits of a batch of streams on the device (gfx950).  Included by mp3s_device.hip only.
//
//   k_reveal : what the reference's reveal reads of an MP3 file -- the table indices of every granule, in the order channel,
//              granule, region, index 0 skipped, an index in H0 a `0` and any other a `1` (decoder/Frame.py:676-685,
//              decoder/util.py:67-81; stego_bits_from_tsel on the host) -- from the file images as they are and the host's frame
//              walk (FrameRef / StreamRef, as k_dec_parse takes them).  No main data is touched: per frame the CRC bit and the
//              mode of the header and three bytes of each granule's side info (both layouts of a granule take 59 bits: the
//              window-switching flag and the 15 bits behind it hold every index, k_parse.hpp:58-78).
//              One workgroup per stream, one frame per thread, the stream's frames in tiles of REVEAL_TILE:
//                * region 2 of a window-switching granule is not in the side info: it contributes the index the last granule of
//                  the same (channel, granule) class without window switching left behind (0 at the stream's start).
//                  "last defined value" = an inclusive max-scan on (thread + 1) << 5 | index, 0 for a granule that defines
//                  nothing: two classes to a dword (16-bit fields, v_pk_max_u16), wave scan by __shfl_up, wave totals through
//                  LDS, the value in front of the tile carried in registers (it restarts with the workgroup = at every stream);
//                * the frame's <= 12 bits and their count; an exclusive prefix sum of the counts the same way;
//                * every thread ORs its bits into the tile's bit buffer in LDS (MSB first: <= 2 dwords per thread), the completed
//                  dwords go out with ordinary vector stores, the partial last dword is carried into the next tile and written,
//                  zero-padded, behind the last one.
//              Bytes past the stream's end read as zero, as in k_dec_parse.  No global atomics, no scratch.
#pragma once

namespace mp3s {

constexpr int REVEAL_TILE = 256;            // frames of a tile = threads of the workgroup
constexpr int REVEAL_BAD_REF = 1;           // status: a frame reference names another stream or lies outside [base, end) (nothing was read there)
constexpr int REVEAL_BUF = REVEAL_TILE * 12 / 32 + 2;   // dwords of the tile's bit buffer: the carried dword's bits + 12 per frame

typedef unsigned short reveal_u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t reveal_max2(uint32_t a, uint32_t b)   // two 16-bit maxima
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(reveal_u16x2, a), __builtin_bit_cast(reveal_u16x2, b)));
}

__global__ __launch_bounds__(REVEAL_TILE) void k_reveal(
    const uint8_t *__restrict__ image, uint32_t image_base /* image[0] is byte `image_base` of what file_off / base / end count in */,
    const ParseFrameRef *__restrict__ refs, const ParseStreamRef *__restrict__ streams, const uint32_t *__restrict__ out_off /* per stream, multiple of 4 */,
    uint32_t h0_mask /* bit t: table index t is in H0 */, uint8_t *__restrict__ packed, int32_t *__restrict__ n_bits, int32_t *__restrict__ status)
{
    constexpr int WAVES = REVEAL_TILE / 64;
    __shared__ uint32_t buf[REVEAL_BUF];                  // the tile's bits, big-endian dwords; buf[0] starts with the carried bits
    __shared__ uint32_t w_max[2][WAVES], w_sum[WAVES];    // wave totals of the two scans
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t s = blockIdx.x;
    const ParseStreamRef *st = streams + s;
    const uint32_t s_base = st->base, s_end = st->end, s_first = st->first_frame, s_n = st->n_frames;
    const uint8_t *img = image - image_base;              // indexed by the offsets the records hold
    uint32_t *out = reinterpret_cast<uint32_t *>(packed + out_off[s]);
    if (tid < REVEAL_BUF) buf[tid] = 0;
    uint32_t run_a = 0, run_b = 0;                        // the index each class was left with in front of the tile: (ch0 gr0 | ch0 gr1 << 16), (ch1 gr0 | ch1 gr1 << 16)
    uint32_t carried = 0, out_dw = 0, total_bits = 0;     // bits in buf[0] from the tile before; dwords written; bits of the stream so far
    bool bad = false;
    ParseFrameRef ref = {0, 0, 0, 0, 0, 0};
    if ((uint32_t)tid < s_n) ref = refs[s_first + tid];
    for (uint32_t t0 = 0; t0 < s_n; t0 += REVEAL_TILE) {
        const bool have = t0 + (uint32_t)tid < s_n;
        const ParseFrameRef cur = ref;
        if (t0 + REVEAL_TILE + (uint32_t)tid < s_n) ref = refs[s_first + t0 + REVEAL_TILE + tid];   // the next tile's, under this one's work
        // ---- the frame's header bits and, per granule*channel, the window-switching flag with the 15 bits behind it
        uint32_t x[4] = {0, 0, 0, 0};                     // class c = ch * 2 + gr (the order the bits walk them)
        uint32_t nch = 2;
        if (have) {
            const uint32_t off = cur.file_off;
            const bool ok = cur.stream == (uint16_t)s && off >= s_base && off < s_end;
            bad |= !ok;
            const uint32_t avail = ok ? s_end - off : 0u;  // bytes of the stream from the frame's header on: the rest reads as zero
            auto byte_at = [&](uint32_t k) -> uint32_t { return k < avail ? (uint32_t)img[(size_t)off + k] : 0u; };
            const uint32_t b1 = byte_at(1), b3 = byte_at(3);
            const uint32_t sstart = (b1 & 1u) == 0 ? 6u : 4u;
            nch = (b3 >> 6) == 3 ? 1u : 2u;
            const uint32_t units = 9 + (nch == 2 ? 3 : 5) + 4 * nch;   // main_data_begin, private bits, scfsi
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const uint32_t ch = (uint32_t)c >> 1, gr = (uint32_t)c & 1u;
                if (ch < nch) {
                    const uint32_t pos = units + 59 * (gr * nch + ch) + 33;   // window_switching
                    const uint32_t b = sstart + (pos >> 3);
                    const uint32_t w = (byte_at(b) << 16) | (byte_at(b + 1) << 8) | byte_at(b + 2);
                    x[c] = (w >> (8 - (pos & 7))) & 0xffffu;
                }
            }
        }
        // ---- region 2: the index each class holds behind this frame
        uint32_t key[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const bool defines = have && (uint32_t)(c >> 1) < nch && !(x[c] & 0x8000u);
            key[c] = defines ? ((uint32_t)(tid + 1) << 5) | (x[c] & 31u) : 0u;
        }
        uint32_t ka = key[0] | (key[1] << 16), kb = key[2] | (key[3] << 16);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t ua = __shfl_up(ka, d, 64), ub = __shfl_up(kb, d, 64);
            if (lane >= d) { ka = reveal_max2(ka, ua); kb = reveal_max2(kb, ub); }
        }
        if (lane == 63) { w_max[0][wave] = ka; w_max[1][wave] = kb; }
        __syncthreads();
        uint32_t all_a = 0, all_b = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            const uint32_t ta = w_max[0][w], tb = w_max[1][w];
            if (w < wave) { ka = reveal_max2(ka, ta); kb = reveal_max2(kb, tb); }
            all_a = reveal_max2(all_a, ta); all_b = reveal_max2(all_b, tb);
        }
        // (a field of 0: nothing in the tile up to here defines the class -- what stood in front of the tile holds)
        auto resolve = [](uint32_t k, uint32_t run) -> uint32_t {
            const uint32_t lo = (k & 0xffffu) ? k & 31u : run & 31u, hi = (k >> 16) ? (k >> 16) & 31u : (run >> 16) & 31u;
            return lo | (hi << 16);
        };
        const uint32_t ra = resolve(ka, run_a), rb = resolve(kb, run_b);
        run_a = resolve(all_a, run_a); run_b = resolve(all_b, run_b);
        const uint32_t t2[4] = {ra & 31u, ra >> 16, rb & 31u, rb >> 16};
        // ---- the frame's bits, first one on top
        uint32_t v = 0, cnt = 0;
        if (have) {
#pragma unroll
            for (int c = 0; c < 4; c++) {
                if ((uint32_t)(c >> 1) >= nch) continue;
                const bool ws = (x[c] & 0x8000u) != 0;
                const uint32_t t[3] = {ws ? (x[c] >> 7) & 31u : (x[c] >> 10) & 31u, ws ? (x[c] >> 2) & 31u : (x[c] >> 5) & 31u, t2[c]};
#pragma unroll
                for (int r = 0; r < 3; r++)
                    if (t[r]) { v = (v << 1) | (((h0_mask >> t[r]) & 1u) ^ 1u); cnt++; }
            }
        }
        // ---- where they go: exclusive prefix sum of the counts
        uint32_t sum = cnt;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t u = __shfl_up(sum, d, 64);
            if (lane >= d) sum += u;
        }
        if (lane == 63) w_sum[wave] = sum;
        __syncthreads();                                   // (also: buf is zeroed / holds the carried dword)
        uint32_t tile_bits = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            const uint32_t tw = w_sum[w];
            if (w < wave) sum += tw;
            tile_bits += tw;
        }
        if (cnt) {
            const uint32_t at = carried + sum - cnt;       // bit position in the tile's buffer
            const uint64_t w64 = (uint64_t)v << (64 - cnt - (at & 31u));
            atomicOr(&buf[at >> 5], (uint32_t)(w64 >> 32));
            if ((uint32_t)w64) atomicOr(&buf[(at >> 5) + 1], (uint32_t)w64);
        }
        __syncthreads();
        const uint32_t filled = carried + tile_bits, full = filled >> 5;
        const uint32_t mine = (uint32_t)tid < full ? buf[tid] : 0u, rest = buf[full];   // (full <= REVEAL_BUF - 2)
        __syncthreads();
        if ((uint32_t)tid < full) out[out_dw + tid] = __builtin_bswap32(mine);          // MSB first inside every byte, bytes in order
        if (tid < REVEAL_BUF) buf[tid] = tid == 0 ? rest : 0u;                          // (the next tile ORs behind two barriers)
        out_dw += full; carried = filled & 31u; total_bits += tile_bits;
    }
    if (tid == 0) {
        if (carried) out[out_dw] = __builtin_bswap32(buf[0]);   // the last bytes, zero-padded (thread 0 wrote buf[0] itself)
        n_bits[s] = (int32_t)total_bits;
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    if (tid == 0) status[s] = any_bad ? REVEAL_BAD_REF : 0;
}

}  // namespace mp3s
