// PCM batches in the caller's device memory (gfx950): the decoder's interleaved int16 frames -> a planar [B][C][T] batch, and such a
// batch -> the encoder's int16 stereo frames.  Included by mp3s_device.hip only.  The rules: include/mp3s.h, section (vi-f).
//
// Both kernels are streaming copies with a change of layout, and both find their work in a table the host made (PcmBatchTile, 8 bytes
// a workgroup: item and tile inside it), so that one item of 10 000 frames and 250 items of 40 frames both spread over the device.
// Every output element has exactly one writer: ordinary vector stores, no LDS, no atomics, no scratch, nothing to clear beforehand.
//
//   k_pcm_batch   : a lane owns, per plane, one GROUP of 8 output elements that starts on a 16-byte boundary of the OUTPUT: with
//                off = the plane's first element counted from the 16-byte boundary in front of it (0 .. 7 for int16, 0 .. 3 for float32),
//                group g holds the plane's elements t in [8 g - off, 8 g - off + 8).  A group inside [0, T) is one 16-byte store
//                (int16) or two (float32), consecutive lanes on consecutive 16 (32) bytes; the group that hangs over the plane's start or
//                end -- there is at most one of each -- stores its elements one by one, and only those in [0, T).  Whatever T, first_row
//                and the base are, the wide store is used wherever the plane allows it, and nothing outside the item's slot is touched.
//                The two planes of a slot may sit differently (T odd): each plane has its own groups, and the 8 source rows are loaded
//                again only when they are other rows.  The source is the narrow side: 8 consecutive rows (16 or 32 bytes) per lane, as one
//                or two 16-byte loads where the rows start on a 16-byte boundary (uniform per plane) and lie inside the stream, row by
//                row otherwise; rows behind the stream's end are not read, the element is 0.
//   k_pcm_unbatch : a lane owns 4 rows of an item's frames = one aligned 16-byte store of [l r l r l r l r]; its 4 elements per plane
//                come as one 8- or 16-byte load where both planes start on such a boundary (uniform per item), one by one otherwise.
//                Rows at and behind n_rows are 0 whatever the tensor holds; float32 by the rule of k_wav_import (k_wav.hpp).
#pragma once

namespace mp3s {

constexpr int PCMBATCH_THREADS = kPcmBatchThreads;

// rows [t0, t0 + 8) of a stream whose row 0 is at `rows`, as int32 left / right (mono: both the sample); 0 outside [0, valid)
template <int NCH>
__device__ __forceinline__ void pcm_batch_load8(const int16_t *__restrict__ rows, int64_t t0, int64_t valid, bool wide, int32_t (&l)[8], int32_t (&r)[8])
{
    if (wide && t0 >= 0 && t0 + 8 <= valid) {
        const uint4 *p = reinterpret_cast<const uint4 *>(rows + t0 * NCH);
        if constexpr (NCH == 2) {
            const uint4 a = p[0], b = p[1];
            const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int k = 0; k < 8; k++) { l[k] = (int32_t)(w[k] << 16) >> 16; r[k] = (int32_t)w[k] >> 16; }
        } else {
            const uint4 a = p[0];
            const uint32_t w[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int k = 0; k < 4; k++) { l[2 * k] = r[2 * k] = (int32_t)(w[k] << 16) >> 16; l[2 * k + 1] = r[2 * k + 1] = (int32_t)w[k] >> 16; }
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int64_t t = t0 + k;
        const bool in = t >= 0 && t < valid;
        if constexpr (NCH == 2) {
            const uint32_t w = in ? reinterpret_cast<const uint32_t *>(rows)[t] : 0u;   // (a stereo row is a dword: d_pcm is aligned to it)
            l[k] = (int32_t)(w << 16) >> 16; r[k] = (int32_t)w >> 16;
        } else l[k] = r[k] = in ? (int32_t)rows[t] : 0;
    }
}

// elements [t0, t0 + 8) of a plane whose element 0 is at `plane`: int16 v, or float32 v * scale (exact: |v| < 2^17, scale a power of two)
template <bool F32>
__device__ __forceinline__ void pcm_batch_store8(uint8_t *__restrict__ plane, int64_t t0, int64_t T, const int32_t (&v)[8], float scale)
{
    if (t0 >= 0 && t0 + 8 <= T) {                                  // (plane + t0 elements is a multiple of 16: the lane's group)
        if constexpr (F32) {
            float4 *dst = reinterpret_cast<float4 *>(plane + t0 * 4);
            dst[0] = make_float4((float)v[0] * scale, (float)v[1] * scale, (float)v[2] * scale, (float)v[3] * scale);
            dst[1] = make_float4((float)v[4] * scale, (float)v[5] * scale, (float)v[6] * scale, (float)v[7] * scale);
        } else {
            uint4 o;
            o.x = ((uint32_t)v[0] & 0xffffu) | ((uint32_t)v[1] << 16); o.y = ((uint32_t)v[2] & 0xffffu) | ((uint32_t)v[3] << 16);
            o.z = ((uint32_t)v[4] & 0xffffu) | ((uint32_t)v[5] << 16); o.w = ((uint32_t)v[6] & 0xffffu) | ((uint32_t)v[7] << 16);
            *reinterpret_cast<uint4 *>(plane + t0 * 2) = o;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int64_t t = t0 + k;
        if (t < 0 || t >= T) continue;
        if constexpr (F32) reinterpret_cast<float *>(plane)[t] = (float)v[k] * scale;
        else reinterpret_cast<int16_t *>(plane)[t] = (int16_t)v[k];
    }
}

template <int NCH, int C, bool F32>
__global__ __launch_bounds__(PCMBATCH_THREADS) void k_pcm_batch(
    const int16_t *__restrict__ pcm, const mp3s_pcm_batch_item *__restrict__ items, const PcmBatchTile *__restrict__ tiles, int64_t T,
    uint8_t *__restrict__ out)
{
    constexpr int ESZ = F32 ? 4 : 2;
    const PcmBatchTile tile = tiles[blockIdx.x];
    const mp3s_pcm_batch_item it = items[tile.item];
    const int64_t left = it.n_rows - it.first_row, valid = left < 0 ? 0 : (left > T ? T : left);
    const int16_t *rows = pcm + (it.src_row + it.first_row) * NCH;   // (read below `valid` only)
    const int64_t g = (int64_t)tile.first * PCMBATCH_THREADS + (int64_t)threadIdx.x;
    int32_t l[8], r[8], v[8];
    int64_t loaded = -1;                                            // the off the rows in l / r were loaded for
#pragma unroll
    for (int c = 0; c < C; c++) {
        uint8_t *plane = out + ((int64_t)it.slot * C + c) * T * ESZ;
        const int64_t off = (int64_t)(((uintptr_t)plane & 15u) / ESZ), t0 = 8 * g - off;   // (uniform: the plane's place)
        if (t0 >= T) continue;
        if (off != loaded) {
            const bool wide = (((uintptr_t)rows - (uintptr_t)(off * NCH * 2)) & 15u) == 0;   // (uniform; 8 g rows are a multiple of 16 bytes)
            pcm_batch_load8<NCH>(rows, t0, valid, wide, l, r);
            loaded = off;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if constexpr (NCH == 2 && C == 1) v[k] = F32 ? l[k] + r[k] : (l[k] + r[k]) >> 1;   // int16: floor; float32: (l + r) / 65536
            else v[k] = c == 0 ? l[k] : r[k];
        }
        pcm_batch_store8<F32>(plane, t0, T, v, NCH == 2 && C == 1 ? 1.0f / 65536.0f : 1.0f / 32768.0f);
    }
}

// element t of a plane -> the int16 the encoder takes: float32 by k_wav_import's rule (round half to even, clamp, NaN -> 0)
__device__ __forceinline__ int32_t pcm_unbatch_f32(float x)
{
    const float y = fminf(fmaxf(__builtin_rintf(x * 32768.0f), -32768.0f), 32767.0f);
    return x != x ? 0 : (int)y;
}

template <int C, bool F32>
__global__ __launch_bounds__(PCMBATCH_THREADS) void k_pcm_unbatch(
    const uint8_t *__restrict__ in, const mp3s_pcm_unbatch_item *__restrict__ items, const PcmBatchTile *__restrict__ tiles, int64_t T,
    int16_t *__restrict__ pcm)
{
    constexpr int ESZ = F32 ? 4 : 2;
    const PcmBatchTile tile = tiles[blockIdx.x];
    const mp3s_pcm_unbatch_item it = items[tile.item];
    const int64_t rows_out = (it.n_rows + 1151) / 1152 * 1152;
    const int64_t t0 = ((int64_t)tile.first * PCMBATCH_THREADS + (int64_t)threadIdx.x) * 4;
    if (t0 >= rows_out) return;
    const uint8_t *plane[2] = {in + (int64_t)it.slot * C * T * ESZ, in + ((int64_t)it.slot * C + (C - 1)) * T * ESZ};
    const bool wide = ((((uintptr_t)plane[0] | (uintptr_t)plane[1]) & (uintptr_t)(4 * ESZ - 1)) == 0) && t0 + 4 <= it.n_rows;
    int32_t v[2][4];
#pragma unroll
    for (int c = 0; c < C; c++) {
        if (wide) {
            if constexpr (F32) {
                const float4 x = *reinterpret_cast<const float4 *>(plane[c] + t0 * 4);
                v[c][0] = pcm_unbatch_f32(x.x); v[c][1] = pcm_unbatch_f32(x.y); v[c][2] = pcm_unbatch_f32(x.z); v[c][3] = pcm_unbatch_f32(x.w);
            } else {
                const uint2 x = *reinterpret_cast<const uint2 *>(plane[c] + t0 * 2);
                v[c][0] = (int32_t)(x.x << 16) >> 16; v[c][1] = (int32_t)x.x >> 16; v[c][2] = (int32_t)(x.y << 16) >> 16; v[c][3] = (int32_t)x.y >> 16;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int64_t t = t0 + k;
                if (t >= it.n_rows) v[c][k] = 0;                   // (zero by select: the tensor is not read there)
                else if constexpr (F32) v[c][k] = pcm_unbatch_f32(reinterpret_cast<const float *>(plane[c])[t]);
                else v[c][k] = (int32_t)reinterpret_cast<const int16_t *>(plane[c])[t];
            }
        }
    }
    uint4 o;
    o.x = ((uint32_t)v[0][0] & 0xffffu) | ((uint32_t)v[C - 1][0] << 16); o.y = ((uint32_t)v[0][1] & 0xffffu) | ((uint32_t)v[C - 1][1] << 16);
    o.z = ((uint32_t)v[0][2] & 0xffffu) | ((uint32_t)v[C - 1][2] << 16); o.w = ((uint32_t)v[0][3] & 0xffffu) | ((uint32_t)v[C - 1][3] << 16);
    *reinterpret_cast<uint4 *>(pcm + (it.dst_frame * 1152 + t0) * 2) = o;
}

}  // namespace mp3s
