// int16 stereo rows of any sampling rate -> the PCM buffer of an encode batch at 32 000 / 44 100 / 48 000 Hz (included by mp3s_device.hip).
//
// An extension beyond the reference (its encoder refuses every other rate): MP3S_OPT_WAV_RESAMPLE, the rules are stated at
// mp3s_wav_resample_info in include/mp3s.h.  A polyphase FIR in exact integer arithmetic: output row n of a stream sits at input
// position n M / L, i0 = floor(n M / L), phase p = n M mod L, and is
//     y[n] = clamp((sum_k c[p][k] x[i0 - H + 1 + k] + 2^14) >> 15),  k = 0 .. T - 1,  T = 2 H,  x = 0 outside [0, n_in).
// The host made c (wav_resample_taps: every phase sums to 32768).  sum |c| of a phase is up to 69 292, so one int32 sum could overflow
// on full-scale input; the taps below 2 (H / 2) and the rest are added apart -- the host has checked sum |c| <= 65535 for either part,
// so each fits int32 whatever x holds -- and joined in 64 bits in front of the shift: the result is the exact one.
//
// Input: the unchanged k_wav_import has laid the stream's samples, at the SOURCE rate, as [left | right] int16 rows into a scratch
// buffer (mono already in both halves).  One grid row per stream, a workgroup owns tiles of kResTile = 1024 output rows.  Per tile it
// stages the span of input rows the tile needs (tile M / L + T rows, `span` of the record: at most 8 441 rows = 33.8 KB, 544 rows for
// 22 050 -> 44 100 Hz) into LDS as [L | R] dwords -- coalesced dword loads, every row outside [0, n_in) a zero, so the inner loop has
// no bounds test -- and every lane computes four consecutive output rows and stores them as ONE aligned 16-byte piece.
// Taps: pairs of consecutive taps as packed int16 dwords [p][T / 2], uploaded once per ratio and context.  A table of up to
// kResTapsLds dwords (8 KB: L = 2, 4, 7 .. of the usual rates) is staged in LDS once per workgroup; a larger one (147 x 18 dwords for
// 48 000 -> 44 100) is read through the vector cache, 21 .. 160 KB that all workgroups share.
// Inner product: two v_perm_b32 make (x[i], x[i + 1]) of the left and of the right channel out of two [L | R] dwords, two
// v_dot2_i32_i16 take a pair of taps each.  A mono stream computes the left sum only.  No byte or short accesses to global memory,
// no per-lane arrays that are indexed at run time, no scratch.
#pragma once

namespace mp3s {

typedef short resample_s2 __attribute__((ext_vector_type(2)));
// a record's tap pointer names global memory: said to the compiler, so that the taps are global loads, not flat ones
typedef const __attribute__((address_space(1))) uint32_t *resample_gtaps;

template <bool MONO, typename TP>
__device__ __forceinline__ uint32_t wav_resample_row(const uint32_t *__restrict__ x /* LDS: the row's first input dword */,
                                                     TP tp /* the phase's T / 2 tap pairs */, uint32_t n_pairs)
{
    int aL[2] = {1 << 14, 0}, aR[2] = {1 << 14, 0};          // the two parts of the sum (each inside int32: the host's check)
    const uint32_t split = n_pairs >> 1;
#pragma unroll
    for (int part = 0; part < 2; part++) {
        for (uint32_t k = part ? split : 0u; k < (part ? n_pairs : split); k++) {
            const resample_s2 c = __builtin_bit_cast(resample_s2, tp[k]);
            const uint32_t d0 = x[2 * k], d1 = x[2 * k + 1];
            // v_perm_b32 D, S0, S1, sel: byte k of D = byte sel[k] of {S0, S1} (S1 = bytes 0..3, S0 = bytes 4..7)
            aL[part] = __builtin_amdgcn_sdot2(__builtin_bit_cast(resample_s2, __builtin_amdgcn_perm(d1, d0, 0x05040100u)), c, aL[part], false);
            if constexpr (!MONO) aR[part] = __builtin_amdgcn_sdot2(__builtin_bit_cast(resample_s2, __builtin_amdgcn_perm(d1, d0, 0x07060302u)), c, aR[part], false);
        }
    }
    const int64_t sL = ((int64_t)aL[0] + (int64_t)aL[1]) >> 15, sR = ((int64_t)aR[0] + (int64_t)aR[1]) >> 15;
    const int yL = (int)min(max(sL, (int64_t)-32768), (int64_t)32767);
    const int yR = MONO ? yL : (int)min(max(sR, (int64_t)-32768), (int64_t)32767);
    return ((uint32_t)yL & 0xffffu) | ((uint32_t)yR << 16);
}

template <bool MONO, typename TP>
__device__ __forceinline__ uint4 wav_resample_piece(const WavResampleRun &r, const uint32_t *__restrict__ xs, TP taps,
                                                    uint32_t e /* (n M) - (the tile's first input row) L, of the piece's first row */, uint64_t n)
{
    const uint32_t n_pairs = r.T >> 1;
    uint32_t o[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t j = e / r.L, p = e - j * r.L;               // the row's first input row in the span, its phase
        o[q] = n + (uint64_t)q < r.n_out ? wav_resample_row<MONO>(xs + j, taps + (size_t)p * n_pairs, n_pairs) : 0u;
        e += r.M;
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

__global__ __launch_bounds__(256) void k_wav_resample(const uint32_t *__restrict__ rows /* the scratch k_wav_import filled */,
                                                      const WavResampleRun *__restrict__ runs, int run0, int16_t *__restrict__ pcm)
{
    extern __shared__ uint32_t res_lds[];
    const WavResampleRun r = runs[run0 + blockIdx.y];
    uint32_t *xs = res_lds, *ts = res_lds + r.span;
    const resample_gtaps gt = (resample_gtaps)(uintptr_t)r.taps;
    const uint32_t *__restrict__ src = rows + r.src_row;
    uint4 *__restrict__ dst = reinterpret_cast<uint4 *>(pcm + (size_t)r.first_frame * 2304);
    const uint64_t n_rows = (uint64_t)r.n_frames * 1152;                       // rows of the stream in the batch: a multiple of 4
    const uint32_t n_tiles = (uint32_t)((n_rows + kResTile - 1) / kResTile);
    if (r.taps_lds)                                                            // (uniform; visible behind the first barrier below)
        for (uint32_t i = threadIdx.x; i < r.L * (r.T >> 1); i += 256) ts[i] = gt[i];
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {      // (uniform: every lane of the workgroup meets the barriers)
        const uint64_t n0 = (uint64_t)tile * kResTile, a = n0 * r.M;
        const uint64_t q0 = a / r.L;                                           // input row of the tile's first output row
        const uint32_t r0 = (uint32_t)(a - q0 * r.L);
        const int64_t base = (int64_t)q0 - (int64_t)(r.T >> 1) + 1;            // input row of xs[0]
        __syncthreads();                                                       // (the tile before is read)
        for (uint32_t j = threadIdx.x; j < r.span; j += 256) {
            const int64_t i = base + (int64_t)j;
            xs[j] = i >= 0 && (uint64_t)i < r.n_in ? src[i] : 0u;
        }
        __syncthreads();
        const uint64_t n = n0 + 4 * threadIdx.x;
        if (n < n_rows) {
            const uint32_t e = r0 + 4 * threadIdx.x * r.M;                     // < 1280 + 1020 x 10240: the host refuses M / L > 8 (T > 256)
            uint4 o;                                                           // (uniform branches; taps in LDS and in global memory stay apart)
            if (r.taps_lds) o = r.mono ? wav_resample_piece<true>(r, xs, (const uint32_t *)ts, e, n) : wav_resample_piece<false>(r, xs, (const uint32_t *)ts, e, n);
            else o = r.mono ? wav_resample_piece<true>(r, xs, gt, e, n) : wav_resample_piece<false>(r, xs, gt, e, n);
            dst[n >> 2] = o;
        }
    }
}

}  // namespace mp3s
