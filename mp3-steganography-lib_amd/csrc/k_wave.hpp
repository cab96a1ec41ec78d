// Reductions over the 64 lanes of a wave in the ALU (DPP), no LDS (gfx950).  Included by mp3s_device.hip only, ahead of the kernel headers.
//
// One ladder of six steps serves them all: inside the rows of 16 by shifts of 1, 2, 4, 8 (row_shr), then the last lane of rows 0 and 2
// into rows 1 and 3 (row_bcast:15), then lane 31 into rows 2 and 3 (row_bcast:31).  A lane without a source reads the 0 the DPP move
// leaves it, which is neutral for an unsigned sum and an unsigned maximum.  After the ladder lane l holds the result over lanes 0 .. l:
// an inclusive scan, and the wave's total in lane 63.  (Through __shfl_up a step was an LDS permute, a compare, a select and the
// operation, with the address arithmetic of the permute on top.)
//
// Not here, because their steps differ: dpp_f64 (k_decode.hpp) sums doubles by quad_perm and row mirrors, the order the fp64 sums of
// the reference are reproduced in; the band sums of k_enc_pack stop after the four row shifts; k_reveal.hpp, k_chain.hpp,
// k_huffman.hpp, k_parse.hpp and the per-pair passes of k_pcmdiff.hpp / k_pcmalign.hpp shuffle (16-bit pairs, records, 64-bit
// values, butterflies of 4 lanes).
#pragma once

namespace mp3s {

// one DPP step: lanes without a source read 0 (ctrl and row mask must be literals)
#define WAVE_DPP(v, ctrl, rm) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), ctrl, rm, 0xf, false))
// the ladder: row_shr:1, 2, 4, 8, row_bcast:15, row_bcast:31
#define WAVE_LADDER(STEP) STEP(0x111, 0xf) STEP(0x112, 0xf) STEP(0x114, 0xf) STEP(0x118, 0xf) STEP(0x142, 0xa) STEP(0x143, 0xc)

__device__ __forceinline__ uint32_t lane63(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)v, 63); }

// inclusive prefix sums / maxima over the lanes: the wave's sum / maximum is valid in lane 63
__device__ __forceinline__ uint32_t wave_scan_u32(uint32_t v)
{
#define WAVE_STEP(ctrl, rm) v += WAVE_DPP(v, ctrl, rm);
    WAVE_LADDER(WAVE_STEP)
#undef WAVE_STEP
    return v;
}
__device__ __forceinline__ uint32_t wave_scan_max_u32(uint32_t v)
{
#define WAVE_STEP(ctrl, rm) v = max(v, WAVE_DPP(v, ctrl, rm));
    WAVE_LADDER(WAVE_STEP)
#undef WAVE_STEP
    return v;
}
// ... and the same in every lane (a scalar, read from lane 63)
__device__ __forceinline__ uint32_t wave_add_u32(uint32_t v) { return lane63(wave_scan_u32(v)); }
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { return lane63(wave_scan_max_u32(v)); }

// Several reductions at once: a DPP step has to wait two issue slots for the VALU write in front of it, so independent
// chains are written step by step side by side -- the second and third fill the slots the first would idle in.
__device__ __forceinline__ void wave_add2(uint32_t &a, uint32_t &b)
{
#define WAVE_STEP(ctrl, rm) { const uint32_t ta = WAVE_DPP(a, ctrl, rm), tb = WAVE_DPP(b, ctrl, rm); a += ta; b += tb; }
    WAVE_LADDER(WAVE_STEP)
#undef WAVE_STEP
    a = lane63(a); b = lane63(b);
}
__device__ __forceinline__ void wave_add3(uint32_t &a, uint32_t &b, uint32_t &c)
{
#define WAVE_STEP(ctrl, rm) { const uint32_t ta = WAVE_DPP(a, ctrl, rm), tb = WAVE_DPP(b, ctrl, rm), tc = WAVE_DPP(c, ctrl, rm); a += ta; b += tb; c += tc; }
    WAVE_LADDER(WAVE_STEP)
#undef WAVE_STEP
    a = lane63(a); b = lane63(b); c = lane63(c);
}
__device__ __forceinline__ void wave_max3(uint32_t &a, uint32_t &b, uint32_t &c)
{
#define WAVE_STEP(ctrl, rm) { const uint32_t ta = WAVE_DPP(a, ctrl, rm), tb = WAVE_DPP(b, ctrl, rm), tc = WAVE_DPP(c, ctrl, rm); a = max(a, ta); b = max(b, tb); c = max(c, tc); }
    WAVE_LADDER(WAVE_STEP)
#undef WAVE_STEP
    a = lane63(a); b = lane63(b); c = lane63(c);
}

// A lane's 64-bit value below 2^38 -> the wave's sum (< 2^44), valid in lane 63.  The lane's value is split at bit 26: low parts
// < 2^26, 64 of them < 2^32; high parts < 2^12, 64 of them < 2^18 -- two 32-bit sums that cannot wrap, put together as lo + (hi << 26).
__device__ __forceinline__ uint64_t wave_add64(uint64_t v)
{
    const uint32_t lo = wave_scan_u32((uint32_t)v & 0x3ffffffu), hi = wave_scan_u32((uint32_t)(v >> 26));
    return (uint64_t)lo + ((uint64_t)hi << 26);
}

}  // namespace mp3s
