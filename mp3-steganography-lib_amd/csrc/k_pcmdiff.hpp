// What hiding changed: the exact difference of two int16 PCM streams on the device (gfx950).  Included by mp3s_device.hip only.
//
// A re-encode delays the audio by the codec's delay, so a cover file and its stego file are NOT sample-aligned and their raw difference
// means nothing.  The meaningful pair is the clear re-encode (mp3s_clear_file) against the hide re-encode (mp3s_hide_message) of the
// same input: the same delay, frames and bitrate, only the swapped Huffman tables differ.  The kernels compare any two frame runs of one
// PCM buffer at lag 0; which runs make sense is the caller's business (mp3s_pcm_distortion_files compares what it is given, the Python
// convenience hide_distortions builds exactly that pair).
//
// The PCM is [frame][1152][nch] int16, interleaved, as decode_group(..., d_keep) leaves it: a stereo frame is 4 608 bytes, a mono frame
// 2 304, both multiples of 16, so every frame of a 16-byte aligned buffer starts on such a multiple.  Everything is exact integer
// arithmetic, bit for bit what numpy computes in int64, and does not depend on the order of anything.
//
//   k_pcm_diff_frames : pass 1, one WAVE per compared frame, PCMDIFF_WAVES frames to a workgroup.  The workgroup finds its pair and its
//                first frame in a table the host made from the pairs' frame counts (PcmTile, 8 bytes a workgroup: the grid is
//                the sum of ceil(n_frames / PCMDIFF_WAVES) whatever the mix of long and short pairs is -- one pair of 10 000 frames and
//                250 pairs of 40 frames both spread over the whole device).  A lane takes 16 bytes = 8 samples of A and of B per step
//                (global_load_dwordx4, consecutive lanes on consecutive 16 bytes: 1 KiB per wave instruction); the wave covers a stereo
//                frame in 4.5 steps and a mono frame in 2.25, the last step masked.  All loads of a frame (5 + 5 or 3 + 3) are issued
//                before the first use.  Traffic: a frame of A and of B is read once, 9 216 bytes (4 608 mono) in, 32 bytes out.
//                Per sample d = a - b:  |d| <= 65 535, d*d <= 65 535^2 < 2^32 (as an UNSIGNED product; it does not fit in int32),
//                a*a <= 2^30.  A lane sums its at most 40 samples (5 steps of 8) in 64 bits: < 40 * 2^32 < 2^38, which is what
//                wave_add64 (k_wave.hpp) takes.  max |d|, the count of d != 0 (<= 2 304) and the first differing index take 32 bits; the
//                index travels as its complement under a MAXIMUM, so that "none" (0xFFFFFFFF) is the 0 a lane without a source
//                contributes.  The reduction is DPP, no LDS; lane 63 holds the totals, they are read from there and lane 0 writes the
//                one 32-byte record (PcmDiffAcc: k_pcm_diff_lagged of k_pcmalign.hpp sums and writes its chunks with it too).
//   k_pcm_diff_pairs  : pass 2, one workgroup per pair over the pair's frame records in tiles of PCMDIFF_TILE, one record (two
//                16-byte loads, lanes 32 bytes apart: every line of the tile once) per thread; per-thread sums in 64 bits, ONE reduction at
//                the end -- shuffles inside the wave, the four wave totals through LDS.  Thread 0 writes the pair's 40-byte record.
// Two passes because a frame's record has one writer (its wave) and a pair's record has one writer (its workgroup), whatever the number
// of frames: ordinary vector stores, no atomics, no scratch, nothing to zero beforehand, and the per-frame profile is there for the
// asking.  (One pass with atomics would need zeroed records and 64-bit atomic adds from every wave of a pair into one line.)
#pragma once

namespace mp3s {

constexpr int PCMDIFF_WAVES = kPcmDiffWaves;   // frames of a workgroup of pass 1 = its waves
constexpr int PCMDIFF_TILE = 256;              // frame records of a tile of pass 2 = threads of its workgroup

// What a lane has seen of its frame (chunk), and the wave's record of it.  A lane may add up to 40 samples (wave_add64's bound).
// PCMDIFF_ADD(acc, x, y, index): sample x of A against sample y of B, `index` its place in the frame.  A macro, not a member: as an
// inlined call the compiler folds the chain of not_first maxima from its other end and the two kernels' instructions change
// (docs/LOG.md); written out in the kernel they are the ones measured.
#define PCMDIFF_ADD(acc, x, y, index)                                                                                                  \
    {                                                                                                                                  \
        const int32_t x_ = (x), y_ = (y);                                                                                              \
        const int32_t d_ = x_ - y_;                                                                                                    \
        const uint32_t ad_ = (uint32_t)(d_ < 0 ? -d_ : d_);                                                                            \
        (acc).err2 += ad_ * ad_;                          /* unsigned: 65 535^2 < 2^32 */                                              \
        (acc).sig2 += (uint32_t)(x_ * x_);                                                                                             \
        (acc).max_abs = max((acc).max_abs, ad_);                                                                                       \
        (acc).n_diff += d_ != 0;                                                                                                       \
        (acc).not_first = max((acc).not_first, d_ != 0 ? ~(uint32_t)(index) : 0u);   /* the smallest index has the largest complement */ \
    }
struct PcmDiffAcc {
    uint64_t err2 = 0, sig2 = 0;
    uint32_t max_abs = 0, n_diff = 0, not_first = 0;      // not_first = ~(first differing index), 0: none
    // the whole wave: the lanes' values to lane 63, from there into one record, written by lane 0
    __device__ __forceinline__ void reduce_and_store(int lane, mp3s_pcm_frame_diff *dst) const
    {
        const uint64_t w_err2 = wave_add64(err2), w_sig2 = wave_add64(sig2);
        const uint32_t w_max = wave_scan_max_u32(max_abs), w_n = wave_scan_u32(n_diff), w_nf = wave_scan_max_u32(not_first);
        mp3s_pcm_frame_diff r;
        r.err2 = (uint64_t)lane63((uint32_t)w_err2) | (uint64_t)lane63((uint32_t)(w_err2 >> 32)) << 32;
        r.sig2 = (uint64_t)lane63((uint32_t)w_sig2) | (uint64_t)lane63((uint32_t)(w_sig2 >> 32)) << 32;
        r.max_abs = lane63(w_max); r.n_diff = lane63(w_n); r.first_diff = ~lane63(w_nf); r.reserved = 0;
        if (lane == 0) *dst = r;
    }
};

template <int NCH>
__global__ __launch_bounds__(PCMDIFF_WAVES * 64) void k_pcm_diff_frames(
    const int16_t *__restrict__ pcm, const mp3s_pcm_pair *__restrict__ pairs, const PcmTile *__restrict__ tiles,
    mp3s_pcm_frame_diff *__restrict__ frames)
{
    constexpr int VEC = 1152 * NCH / 8;                   // 16-byte pieces of a frame: 288 / 144
    constexpr int STEPS = (VEC + 63) / 64;                // 5 / 3, the last one covers VEC % 64 = 32 / 16 lanes
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const PcmTile tile = tiles[blockIdx.x];
    const mp3s_pcm_pair pr = pairs[tile.pair];
    const uint32_t f = tile.first + (uint32_t)wave;       // (the same for the whole wave)
    if (f >= pr.n_frames) return;
    const uint4 *A = reinterpret_cast<const uint4 *>(pcm + ((size_t)pr.a_first + f) * (1152 * NCH));
    const uint4 *B = reinterpret_cast<const uint4 *>(pcm + ((size_t)pr.b_first + f) * (1152 * NCH));
    uint4 a[STEPS], b[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; s++) {
        const int i = s * 64 + lane;
        const bool in = (s + 1) * 64 <= VEC || i < VEC;
        a[s] = in ? A[i] : make_uint4(0, 0, 0, 0);
        b[s] = in ? B[i] : make_uint4(0, 0, 0, 0);      // (zeros against zeros: no difference, nothing to the sums)
    }
    PcmDiffAcc acc;
#pragma unroll
    for (int s = 0; s < STEPS; s++) {                     // in the order of the loads: the first step's sums run under the later loads
        const uint32_t wa[4] = {a[s].x, a[s].y, a[s].z, a[s].w}, wb[4] = {b[s].x, b[s].y, b[s].z, b[s].w};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int32_t x = (k & 1) ? (int32_t)wa[k >> 1] >> 16 : (int32_t)(wa[k >> 1] << 16) >> 16;
            const int32_t y = (k & 1) ? (int32_t)wb[k >> 1] >> 16 : (int32_t)(wb[k >> 1] << 16) >> 16;
            PCMDIFF_ADD(acc, x, y, (s * 64 + lane) * 8 + k)
        }
    }
    acc.reduce_and_store(lane, &frames[(size_t)pr.out_first + f]);
}

__global__ __launch_bounds__(PCMDIFF_TILE) void k_pcm_diff_pairs(
    const mp3s_pcm_pair *__restrict__ pairs, const mp3s_pcm_frame_diff *__restrict__ frames, int nch, mp3s_pcm_pair_diff *__restrict__ out)
{
    constexpr int WAVES = PCMDIFF_TILE / 64;
    __shared__ uint64_t w_part[WAVES][4];                 // err2, sig2, n_diff, first
    __shared__ uint32_t w_max[WAVES];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const mp3s_pcm_pair pr = pairs[blockIdx.x];
    const mp3s_pcm_frame_diff *rec = frames + pr.out_first;
    const uint64_t per_frame = (uint64_t)1152 * (uint64_t)nch;
    uint64_t err2 = 0, sig2 = 0, n_diff = 0, first = ~(uint64_t)0;   // first: the smallest index so far, all ones = none
    uint32_t max_abs = 0;
    for (uint32_t f = (uint32_t)tid; f < pr.n_frames; f += PCMDIFF_TILE) {
        const mp3s_pcm_frame_diff r = rec[f];
        err2 += r.err2; sig2 += r.sig2; n_diff += r.n_diff;
        max_abs = max(max_abs, r.max_abs);
        if (r.first_diff != 0xffffffffu) first = min(first, (uint64_t)f * per_frame + r.first_diff);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        err2 += __shfl_down(err2, off); sig2 += __shfl_down(sig2, off); n_diff += __shfl_down(n_diff, off);
        first = min(first, (uint64_t)__shfl_down(first, off));
        max_abs = max(max_abs, (uint32_t)__shfl_down(max_abs, off));
    }
    if (lane == 0) { w_part[wave][0] = err2; w_part[wave][1] = sig2; w_part[wave][2] = n_diff; w_part[wave][3] = first; w_max[wave] = max_abs; }
    __syncthreads();
    if (tid == 0) {
        mp3s_pcm_pair_diff r;
        r.err2 = 0; r.sig2 = 0; r.n_diff = 0; r.max_abs = 0; r.reserved = 0;
        uint64_t fd = ~(uint64_t)0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) {
            r.err2 += w_part[w][0]; r.sig2 += w_part[w][1]; r.n_diff += w_part[w][2];
            fd = min(fd, w_part[w][3]);
            r.max_abs = max(r.max_abs, w_max[w]);
        }
        r.first_diff = (int64_t)fd;                       // all ones = -1: no difference
        out[blockIdx.x] = r;
    }
}

}  // namespace mp3s
