// The decoder's interleaved int16 frames -> a planar [B][C][T] batch at ANOTHER sampling rate (gfx950): k_pcm_batch (k_pcmbatch.hpp)
// with the polyphase FIR of k_wav_resample (k_resample.hpp) in front.  Included by mp3s_device.hip only, behind those two.  The rules:
// include/mp3s.h, section (vi-f), mp3s_pcm_batch_resample_dev.
//
// One launch for all items of a channel count, one workgroup per entry of a table the host made (PcmBatchTile: item and tile inside
// it), and every item carries its own ratio in its record (PcmResampleRun): a 48 kHz and a 44.1 kHz file share the launch, and an item
// with L = M = 1 (T = 0 in the record) is a plain copy.
//
// A tile is cut in elements of the OUTPUT plane: tile f of an item owns the groups [kPcmResGroups f, kPcmResGroups (f + 1)) of each
// plane, group g being the 8 elements t in [8 g - off, 8 g - off + 8) with off = the plane's first element counted from the 16-byte
// boundary in front of it (k_pcm_batch's groups).  Whatever the planes' off are, these lie in the kPcmResRows = 8 kPcmResGroups + 8
// window rows from t = 8 kPcmResGroups f - 8 on, and the workgroup
//   1. stages the input rows under them into LDS as [L | R] dwords, zeros outside [0, n_in), so the inner loop has no bounds test: the
//      window's row t is output row n = first_row + t of the stream, which sits at input row floor(n M / L) (64 bits on the tile's
//      first row, 32 bits inside the tile).  A stereo row is one aligned dword of the source; of a mono stream the aligned dwords are
//      loaded, two rows each, and split here (no short loads from global memory; the dword that holds the stream's first or last row
//      may hold a neighbour's sample beside it, which is not used);
//   2. computes every window row once with wav_resample_row -- the taps from LDS when the table has at most kResTapsLds dwords, through
//      the vector cache otherwise -- into LDS as [l | r] int16 pairs; rows outside [0, valid) are zeros;
//   3. stores the planes from there with pcm_batch_store8: lanes [0, 128) plane 0, lanes [128, 256) plane 1.  A stereo stream into one
//      plane is mixed HERE, behind the resampler: (l + r) >> 1 or (l + r) / 65536 of the resampled, clamped int16 values.
// Every element of the item's slot has exactly one writer, padding included; nothing outside it is touched.  No tile loop, no scratch,
// no per-lane array that is indexed at run time.
#pragma once

namespace mp3s {

// the window row's resampled [l | r] pair (MONO: the sample in both halves)
template <bool MONO, typename TP>
__device__ __forceinline__ uint32_t pcm_resample_at(const PcmResampleRun &r, const uint32_t *__restrict__ xs, TP taps, uint32_t e /* (n M) - (input row of xs[H - 1]) L */)
{
    const uint32_t j = e / r.L, p = e - j * r.L, n_pairs = r.T >> 1;
    return wav_resample_row<MONO>(xs + j, taps + (size_t)p * n_pairs, n_pairs);
}

template <int NCH, int C, bool F32>
__global__ __launch_bounds__(PCMBATCH_THREADS) void k_pcm_batch_resample(
    const int16_t *__restrict__ pcm, const PcmResampleRun *__restrict__ runs, const PcmBatchTile *__restrict__ tiles, int64_t T, uint8_t *__restrict__ out)
{
    constexpr int ESZ = F32 ? 4 : 2;
    static_assert(PCMBATCH_THREADS == 2 * kPcmResGroups, "lanes [0, 128) store plane 0, lanes [128, 256) plane 1");
    extern __shared__ uint32_t pres_lds[];
    const PcmBatchTile tile = tiles[blockIdx.x];
    const PcmResampleRun r = runs[tile.item];
    uint32_t *ys = pres_lds, *xs = pres_lds + kPcmResRows, *ts = xs + r.span;
    const resample_gtaps gt = (resample_gtaps)(uintptr_t)r.taps;
    const int64_t left = (int64_t)r.n_out - r.first_row, valid = left < 0 ? 0 : (left > T ? T : left);
    const int64_t t_base = (int64_t)tile.first * (8 * kPcmResGroups) - 8;      // the window row of ys[0]
    const int64_t t_lo = t_base < 0 ? 0 : t_base;                               // the first row that is computed
    const uint32_t lo = (uint32_t)(t_lo - t_base);                              // 0 or 8
    if (t_lo < valid) {                                                         // (uniform: a tile of padding alone stages nothing)
        if (r.taps_lds)
            for (uint32_t i = threadIdx.x; i < r.L * (r.T >> 1); i += PCMBATCH_THREADS) ts[i] = gt[i];
        const uint64_t a = (uint64_t)(r.first_row + t_lo) * r.M, q0 = a / r.L;  // input row of the first computed row (a < 2^41 x 10240)
        const uint32_t r0 = (uint32_t)(a - q0 * r.L);
        const int64_t base = (int64_t)q0 - (r.T ? (int64_t)(r.T >> 1) - 1 : 0); // input row of xs[0]
        if constexpr (NCH == 2) {
            const uint32_t *__restrict__ src = reinterpret_cast<const uint32_t *>(pcm) + r.src_row;
            for (uint32_t j = threadIdx.x; j < r.span; j += PCMBATCH_THREADS) {
                const int64_t i = base + (int64_t)j;
                xs[j] = i >= 0 && i < (int64_t)r.n_in ? src[i] : 0u;
            }
        } else {
            // row i lies at int16 index src_row + i; h = 1 when row `base` is the upper half of its dword
            const uintptr_t first = (uintptr_t)pcm + (uintptr_t)(2 * (r.src_row + base));
            const uint32_t h = (uint32_t)(first >> 1) & 1u;
            const uint32_t *__restrict__ src = reinterpret_cast<const uint32_t *>(first - 2 * h);   // rows base - h, base - h + 1
            for (uint32_t d = threadIdx.x; 2 * d < r.span + h; d += PCMBATCH_THREADS) {
                const int64_t j0 = (int64_t)(2 * d) - h, i0 = base + j0;                             // span index and input row of the low half
                const bool in0 = i0 >= 0 && i0 < (int64_t)r.n_in, in1 = i0 + 1 >= 0 && i0 + 1 < (int64_t)r.n_in;
                const uint32_t w = in0 || in1 ? src[d] : 0u;
                if (j0 >= 0) xs[j0] = in0 ? (w & 0xffffu) * 0x10001u : 0u;
                if (j0 + 1 < (int64_t)r.span) xs[j0 + 1] = in1 ? (w >> 16) * 0x10001u : 0u;
            }
        }
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < (uint32_t)kPcmResRows; j += PCMBATCH_THREADS) {
            uint32_t y = 0u;
            if (j >= lo && t_base + (int64_t)j < valid) {
                const uint32_t e = r0 + (j - lo) * r.M;                         // < 1280 + 1031 x 10240: the host refuses M / L > 8 (T > 256)
                if (!r.T) y = xs[j - lo];                                       // (uniform branches: copy; taps in LDS; taps in global memory)
                else if (r.taps_lds) y = pcm_resample_at<NCH == 1>(r, xs, (const uint32_t *)ts, e);
                else y = pcm_resample_at<NCH == 1>(r, xs, gt, e);
            }
            ys[j] = y;
        }
    } else {
        for (uint32_t j = threadIdx.x; j < (uint32_t)kPcmResRows; j += PCMBATCH_THREADS) ys[j] = 0u;
    }
    __syncthreads();
    const int c = C == 2 ? (int)(threadIdx.x >> 7) : 0;
    if (C == 1 && threadIdx.x >= (unsigned)kPcmResGroups) return;
    uint8_t *plane = out + ((int64_t)r.slot * C + c) * T * ESZ;
    const int64_t off = (int64_t)(((uintptr_t)plane & 15u) / ESZ);
    const uint32_t gl = threadIdx.x & (kPcmResGroups - 1);
    const int64_t t0 = 8 * ((int64_t)tile.first * kPcmResGroups + gl) - off;
    if (t0 >= T) return;
    const uint32_t *y = ys + (8 * gl + 8 - (uint32_t)off);                      // ys[t0 - t_base]
    int32_t v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t w = y[k];
        const int32_t l = (int32_t)(w << 16) >> 16, rr = (int32_t)w >> 16;
        if constexpr (NCH == 2 && C == 1) v[k] = F32 ? l + rr : (l + rr) >> 1;   // int16: floor; float32: (l + r) / 65536
        else v[k] = c == 0 ? l : rr;
    }
    pcm_batch_store8<F32>(plane, t0, T, v, NCH == 2 && C == 1 ? 1.0f / 65536.0f : 1.0f / 32768.0f);
}

}  // namespace mp3s
