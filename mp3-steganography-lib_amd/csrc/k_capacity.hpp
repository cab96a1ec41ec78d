// Message capacity of a batch of streams on the device (gfx950).  Included by mp3s_device.hip only.
//
//   k_capacity : what the message cursor of the reference advances by over a stream (__hide_str_offset, encoder/MP3_Encoder.py:808-809,
//                1154-1168): the non-zero table indices of every unit whose xrmax != 0 -- n_tables of the records with MP3S_RF_ACTIVE,
//                the sum k_chain.hpp takes for hiding streams -- from the records as the chain check left them.  Nothing else of the
//                encode is read.  One workgroup per stream (mp3s_chain_seg: first_frame, n_frames), one frame per thread, the stream's
//                frames in tiles of CAP_TILE:
//                  * a thread reads n_tables and flags of its frame's four records: two neighbouring dwords 52 bytes into each 72-byte
//                    record, which the compiler takes as one global_load_dwordx2 (dword-aligned, as global loads may be) -- four
//                    independent loads issued together, 8 of the 72 bytes.  A wave's lanes lie 288 bytes apart and a record is shorter
//                    than a cache line, so every line of the tile is fetched once: the kernel reads the record array once, 288 bytes a
//                    frame, which is what a staged, coalesced copy of the tile into LDS would read as well -- with 72 KB of LDS and a
//                    barrier more.  (Wider loads have nothing to take here: the records' other fields are not wanted.)
//                  * the frame's bits (0 .. 12) and its active units (0 .. 4) travel as one dword, bits | units << 16 (a tile's sums are
//                    at most 3 072 and 1 024): ONE inclusive scan -- wave_scan_u32 (k_wave.hpp) inside the wave, the wave totals
//                    through LDS (two buffers, taken in turn: one barrier a tile) -- gives the running sum of the profile and the tile's
//                    totals; the totals in front of the tile are carried in registers and restart with the workgroup = at every stream.
//                Every word written has one writer: ordinary vector stores, no atomics, no scratch.
#pragma once

namespace mp3s {

constexpr int CAP_TILE = 256;               // frames of a tile = threads of the workgroup

__global__ __launch_bounds__(CAP_TILE) void k_capacity(
    const mp3s_gr_out *__restrict__ gr, const mp3s_chain_seg *__restrict__ segs, mp3s_capacity_seg *__restrict__ out,
    uint32_t *__restrict__ profile /* [frames of the batch] or null */)
{
    constexpr int WAVES = CAP_TILE / 64;
    __shared__ uint32_t w_sum[2][WAVES];                  // wave totals of the scan, the tiles take the two rows in turn
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const mp3s_chain_seg *sg = segs + blockIdx.x;
    const int first = sg->first_frame, n = sg->n_frames;  // (the same for the whole workgroup: every thread meets every barrier)
    uint64_t run_bits = 0;                                // the stream's totals in front of the tile
    uint32_t run_units = 0;
    int row = 0;
    for (int t0 = 0; t0 < n; t0 += CAP_TILE, row ^= 1) {
        const int f = t0 + tid;
        uint32_t v = 0;
        if (f < n) {
            const mp3s_gr_out *g = gr + (size_t)(first + f) * 4;
            int32_t tables[4], flags[4];
#pragma unroll
            for (int k = 0; k < 4; k++) { tables[k] = g[k].n_tables; flags[k] = g[k].flags; }
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (flags[k] & MP3S_RF_ACTIVE) v += (uint32_t)tables[k] + 0x10000u;
        }
        v = wave_scan_u32(v);
        if (lane == 63) w_sum[row][wave] = v;
        __syncthreads();
        uint32_t tile = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            const uint32_t tw = w_sum[row][w];
            if (w < wave) v += tw;
            tile += tw;
        }
        if (profile && f < n) profile[(size_t)first + f] = (uint32_t)run_bits + (v & 0xffffu);
        run_bits += tile & 0xffffu; run_units += tile >> 16;
    }
    if (tid == 0) {
        mp3s_capacity_seg r;
        r.bits = (int64_t)run_bits; r.active_units = (int32_t)run_units; r.reserved = 0;
        out[blockIdx.x] = r;
    }
}

}  // namespace mp3s
