// A cover file against its stego file: the lag that aligns two int16 PCM runs, and their exact difference at that lag, on the device
// (gfx950).  Included by mp3s_device.hip only, behind k_pcmdiff.hpp (whose PcmDiffAcc and whose pass 2 are used here).
//
// A re-encode delays the audio, so two files that hold "the same" audio are not sample-aligned.  A run pair is rows
// [a_first, a_first + a_rows) against rows [b_first, b_first + b_rows) of one PCM buffer, [row][nch] int16 interleaved, the runs anywhere
// in it: a stereo row is only 4-byte aligned, a mono row only 2-byte aligned.  Lag L pairs row i + L of A with row i of B, d = a[i+L] - b[i].
// Everything is exact integer arithmetic, bit for bit what numpy computes in int64, and does not depend on the order of anything.
//
//   k_pcm_lag_scores : pass 1, score[pair][L + M] = sum over the window's rows i in [s0, s0 + S) and the channels of (a[i+L] - b[i])^2 for
//                every lag L in [-M, +M].  Brute force: S * (2M + 1) * nch squared differences a pair (4.2e7 at the defaults).  One WAVE
//                is a workgroup and takes a tile of PCMALIGN_LAGS = 256 consecutive lags of one pair, FOUR CONSECUTIVE LAGS A LANE; the
//                window goes through LDS in chunks of PCMALIGN_CHUNK = 256 rows of B and the 256 + 256 rows of A the tile pairs with them,
//                one dword a row (stereo: the row as it lies; mono: the sample in the low half).  Four rows a step: lane t needs the seven
//                rows A[r + 4t .. r + 4t + 6] -- two aligned 16-byte LDS reads, consecutive lanes on consecutive 16 bytes (conflict-free),
//                and the second is the next step's first, so ONE ds_read_b128 of A a step -- and the four rows of B, one 16-byte
//                broadcast read.  A step is 32 squared differences a lane (4 rows x 4 lags x 2 channels) for two LDS reads.
//                Global loads are dwords only (the mono sample is shifted out of its dword); rows of A past the run (lags of the last
//                tile beyond +M) are staged as 0 and their scores are not written.
//                Per sample |d| <= 65 535, d*d <= 65 535^2 < 2^32: it does not fit in int32, and two of them do not fit in uint32, so
//                every product is formed as a signed 64-bit value and added to a 64-bit accumulator (in the ISA: v_sub_u32_sdwa takes the
//                halves of the two dwords, |d| < 2^23 makes d * d a v_mul_i32_i24 / v_mul_hi_i32_i24 pair, v_lshl_add_u64 adds: four
//                vector instructions a squared difference).  A lag's sum
//                is at most S * nch * 65 535^2 with S <= 2^31 rows: < 2^64; at the default S = 4 608 it is < 2^46.
//                Ordinary vector stores, one writer a score: no atomics, nothing to zero beforehand, no scratch.
//   k_pcm_lag_pick   : pass 2, one workgroup per pair over its 2M + 1 scores: the minimum, among equal scores the smaller |L|, between
//                +k and -k the +k (the order of rank(L) = 2|L| - (L > 0)); n_best = the lags that reach the minimum.  It writes the lag
//                record and the geometry pass 3 and k_pcm_diff_pairs read -- the host never learns the lag between the passes.  With
//                lags given by the caller (or a pair too short to search) there is nothing to pick: the record carries the lag, n_best 0.
//   k_pcm_diff_lagged: pass 3, one WAVE per chunk of 1152 rows of the overlap, PCMDIFF_WAVES chunks to a workgroup, found through the
//                same host-made PcmTile table as k_pcm_diff_frames -- sized by the bound ceil(min(rows_a, rows_b) / 1152), which holds
//                for every lag; waves past the pair's real chunk count leave.  A lane takes one row a step (a dword load of A and of B,
//                18 steps a chunk); rows past the overlap's end are masked and contribute nothing, sig2 included (zeros against zeros).
//                A lane sums at most 36 samples in 64 bits, < 36 * 2^32 < 2^38: PcmDiffAcc (k_pcmdiff.hpp) holds.
//                The per-pair reduction is k_pcm_diff_pairs, unchanged, over the geometry's chunk count.
#pragma once

namespace mp3s {

constexpr int PCMALIGN_LAGS = 256;     // lags of a workgroup (one wave) of pass 1: four a lane
constexpr int PCMALIGN_CHUNK = 256;    // rows of B staged at a time
constexpr int PCMALIGN_PICK = 256;     // threads of a workgroup of pass 2

// row `r` of a run as one dword: the stereo row as it lies, the mono sample in the low half (dword loads only)
template <int NCH>
__device__ __forceinline__ uint32_t pcmalign_row(const uint32_t *__restrict__ pcm32, uint64_t r)
{
    if (NCH == 2) return pcm32[r];
    const uint32_t w = pcm32[r >> 1];
    return (r & 1) ? w >> 16 : w & 0xffffu;
}
__device__ __forceinline__ int32_t pcmalign_lo(uint32_t w) { return (int32_t)(w << 16) >> 16; }
__device__ __forceinline__ int32_t pcmalign_hi(uint32_t w) { return (int32_t)w >> 16; }

// the window of a search: false when the pair is too short for it
__device__ __forceinline__ bool pcmalign_window(const mp3s_pcm_run_pair &pr, int M, int search_rows, int64_t *s0, int64_t *S)
{
    const int64_t W = (int64_t)min(pr.a_rows, pr.b_rows) - 2 * (int64_t)M;
    if (W < 1) return false;
    *S = min(W, (int64_t)search_rows);
    *s0 = (int64_t)M + (W - *S) / 2;
    return true;
}

template <int NCH>
__global__ __launch_bounds__(64) void k_pcm_lag_scores(
    const int16_t *__restrict__ pcm, const mp3s_pcm_run_pair *__restrict__ runs, int M, int search_rows, int tiles_per_pair,
    uint64_t *__restrict__ scores)
{
    __shared__ uint4 sA[(PCMALIGN_CHUNK + PCMALIGN_LAGS) / 4];   // rows [c + Lt, c + Lt + CHUNK + LAGS) of A, from the window's first row
    __shared__ uint4 sB[PCMALIGN_CHUNK / 4];                     // rows [c, c + CHUNK) of B
    const int t = (int)threadIdx.x;
    const int pair = (int)(blockIdx.x / (unsigned)tiles_per_pair), tile = (int)(blockIdx.x % (unsigned)tiles_per_pair);
    const mp3s_pcm_run_pair pr = runs[pair];
    int64_t s0, S;
    if (!pcmalign_window(pr, M, search_rows, &s0, &S)) return;   // (the whole workgroup)
    const uint32_t *pcm32 = reinterpret_cast<const uint32_t *>(pcm);
    const int64_t Lt = (int64_t)tile * PCMALIGN_LAGS - M;        // the tile's first lag; lane t owns Lt + 4t .. Lt + 4t + 3
    const int64_t a_lo = s0 + Lt;                                // A row (inside the run) of the window's first row at the tile's first lag: >= 0
    int64_t acc[4] = {0, 0, 0, 0};
    uint32_t *wA = reinterpret_cast<uint32_t *>(sA), *wB = reinterpret_cast<uint32_t *>(sB);
    for (int64_t c = 0; c < S; c += PCMALIGN_CHUNK) {
        const int nv = (int)min((int64_t)PCMALIGN_CHUNK, S - c);  // rows of B in this chunk
        __syncthreads();                                         // (the chunk before has been read)
#pragma unroll
        for (int k = 0; k < (PCMALIGN_CHUNK + PCMALIGN_LAGS) / 64; k++) {
            const int j = k * 64 + t;
            const int64_t ra = a_lo + c + j;                     // row of A inside its run
            wA[j] = ra < (int64_t)pr.a_rows ? pcmalign_row<NCH>(pcm32, (uint64_t)pr.a_first + (uint64_t)ra) : 0u;
        }
#pragma unroll
        for (int k = 0; k < PCMALIGN_CHUNK / 64; k++) {
            const int j = k * 64 + t;
            wB[j] = j < nv ? pcmalign_row<NCH>(pcm32, (uint64_t)pr.b_first + (uint64_t)(s0 + c + j)) : 0u;
        }
        __syncthreads();
        uint4 q0 = sA[t];                                        // rows r + 4t .. r + 4t + 3 of the chunk's A
        for (int r = 0; r < nv; r += 4) {
            const uint4 q1 = sA[(r >> 2) + t + 1], qb = sB[r >> 2];
            const uint32_t a[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w}, b[4] = {qb.x, qb.y, qb.z, qb.w};
            int32_t al[7], ah[7];
#pragma unroll
            for (int k = 0; k < 7; k++) { al[k] = pcmalign_lo(a[k]); ah[k] = pcmalign_hi(a[k]); }
#pragma unroll
            for (int rr = 0; rr < 4; rr++) {
                if (r + rr < nv) {                               // (the same for the whole wave: the last step of the window may be partial)
                    const int32_t bl = pcmalign_lo(b[rr]), bh = pcmalign_hi(b[rr]);
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int32_t dl = al[rr + j] - bl;
                        acc[j] += (int64_t)dl * (int64_t)dl;
                        if (NCH == 2) {
                            const int32_t dh = ah[rr + j] - bh;
                            acc[j] += (int64_t)dh * (int64_t)dh;
                        }
                    }
                }
            }
            q0 = q1;
        }
    }
    const int n_lags = 2 * M + 1;
    uint64_t *out = scores + (size_t)pair * (size_t)n_lags;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int idx = tile * PCMALIGN_LAGS + 4 * t + j;
        if (idx < n_lags) out[idx] = (uint64_t)acc[j];
    }
}

// rank of a lag among equal scores: 0, +1, -1, +2, -2, ...
__device__ __forceinline__ uint32_t pcmalign_rank(int L) { return L > 0 ? 2u * (uint32_t)L - 1u : 2u * (uint32_t)(-L); }

__global__ __launch_bounds__(PCMALIGN_PICK) void k_pcm_lag_pick(
    const mp3s_pcm_run_pair *__restrict__ runs, const uint64_t *__restrict__ scores, const int32_t *__restrict__ given, int M, int search_rows,
    mp3s_pcm_lag *__restrict__ lags, mp3s_pcm_pair *__restrict__ geo)
{
    constexpr int WAVES = PCMALIGN_PICK / 64;
    __shared__ uint64_t w_score[WAVES];
    __shared__ uint32_t w_rank[WAVES], w_count[WAVES];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int pair = (int)blockIdx.x;
    const mp3s_pcm_run_pair pr = runs[pair];
    mp3s_pcm_lag rec;
    rec.lag = 0; rec.n_best = 0; rec.err2_best = 0; rec.err2_at_0 = 0; rec.search_first = 0; rec.search_rows = 0;
    int64_t s0 = 0, S = 0;
    if (given) rec.lag = given[pair];
    else if (pcmalign_window(pr, M, search_rows, &s0, &S)) {     // (the same for the whole workgroup)
        const int n_lags = 2 * M + 1;
        const uint64_t *sc = scores + (size_t)pair * (size_t)n_lags;
        uint64_t best = ~(uint64_t)0;
        uint32_t rank = ~0u;
        for (int i = tid; i < n_lags; i += PCMALIGN_PICK) {
            const uint64_t v = sc[i];
            const uint32_t rk = pcmalign_rank(i - M);
            if (v < best || (v == best && rk < rank)) { best = v; rank = rk; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t v = __shfl_down(best, off);
            const uint32_t rk = (uint32_t)__shfl_down(rank, off);
            if (v < best || (v == best && rk < rank)) { best = v; rank = rk; }
        }
        if (lane == 0) { w_score[wave] = best; w_rank[wave] = rank; }
        __syncthreads();
        best = w_score[0]; rank = w_rank[0];
#pragma unroll
        for (int w = 1; w < WAVES; w++)
            if (w_score[w] < best || (w_score[w] == best && w_rank[w] < rank)) { best = w_score[w]; rank = w_rank[w]; }
        uint32_t count = 0;
        for (int i = tid; i < n_lags; i += PCMALIGN_PICK) count += sc[i] == best;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) count += (uint32_t)__shfl_down(count, off);
        if (lane == 0) w_count[wave] = count;
        __syncthreads();
        count = 0;
#pragma unroll
        for (int w = 0; w < WAVES; w++) count += w_count[w];
        rec.lag = (rank & 1) ? (int32_t)((rank + 1) >> 1) : -(int32_t)(rank >> 1);
        rec.n_best = count; rec.err2_best = best; rec.err2_at_0 = sc[M];
        rec.search_first = (uint32_t)s0; rec.search_rows = (uint32_t)S;
    }
    if (tid != 0) return;
    // the overlap at the lag: B rows [i0, i1), A rows [i0 + L, i1 + L), in chunks of 1152 rows from i0
    const int64_t L = rec.lag;
    const int64_t i0 = max((int64_t)0, -L), i1 = min((int64_t)pr.b_rows, (int64_t)pr.a_rows - L);
    const int64_t n_rows = max((int64_t)0, i1 - i0);
    rec.n_rows = (uint32_t)n_rows; rec.n_chunks = (uint32_t)((n_rows + 1151) / 1152);
    lags[pair] = rec;
    mp3s_pcm_pair g;
    g.a_first = (uint32_t)((int64_t)pr.a_first + i0 + L); g.b_first = (uint32_t)((int64_t)pr.b_first + i0);   // rows, not frames
    g.n_frames = rec.n_chunks; g.out_first = pr.out_first;
    geo[pair] = g;
}

template <int NCH>
__global__ __launch_bounds__(PCMDIFF_WAVES * 64) void k_pcm_diff_lagged(
    const int16_t *__restrict__ pcm, const mp3s_pcm_pair *__restrict__ geo, const mp3s_pcm_lag *__restrict__ lags, const PcmTile *__restrict__ tiles,
    mp3s_pcm_frame_diff *__restrict__ frames)
{
    constexpr int STEPS = 1152 / 64;                      // 18: a row a lane a step
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const PcmTile tile = tiles[blockIdx.x];
    const mp3s_pcm_pair g = geo[tile.pair];
    const uint32_t f = tile.first + (uint32_t)wave;       // (the same for the whole wave)
    if (f >= g.n_frames) return;                          // the table is sized by a bound: this lag's overlap has fewer chunks
    const uint32_t n_rows = lags[tile.pair].n_rows;
    const int nr = (int)min(1152u, n_rows - f * 1152u);   // rows of this chunk: the last one may be partial
    const uint32_t *pcm32 = reinterpret_cast<const uint32_t *>(pcm);
    const uint64_t a0 = (uint64_t)g.a_first + (uint64_t)f * 1152u, b0 = (uint64_t)g.b_first + (uint64_t)f * 1152u;
    uint32_t a[STEPS], b[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; s++) {
        const int i = s * 64 + lane;
        const bool in = i < nr;
        a[s] = in ? pcmalign_row<NCH>(pcm32, a0 + (uint64_t)i) : 0u;
        b[s] = in ? pcmalign_row<NCH>(pcm32, b0 + (uint64_t)i) : 0u;   // (zeros against zeros: no difference, nothing to the sums)
    }
    PcmDiffAcc acc;
#pragma unroll
    for (int s = 0; s < STEPS; s++) {
#pragma unroll
        for (int k = 0; k < NCH; k++)
            PCMDIFF_ADD(acc, k ? pcmalign_hi(a[s]) : pcmalign_lo(a[s]), k ? pcmalign_hi(b[s]) : pcmalign_lo(b[s]), (s * 64 + lane) * NCH + k)
    }
    acc.reduce_and_store(lane, &frames[(size_t)g.out_first + f]);
}

}  // namespace mp3s
