// WAV bytes -> the PCM buffer of an encode batch (included by mp3s_device.hip).
//
// replaces: WavReader.read_samples' np.fromfile(f, 'int16', ...) + the frame slicing of the encoder's loop -- reference
//           encoder/WAV_Reader.py:108, encoder/MP3_Encoder.py:596-618 -- for every stream of a batch at once.
// The job's byte image holds the files as the caller has them (whole WAV files, each starting on a 16-byte boundary);
// per stream a record says where its first sample lies in the image -- data_offset of mp3s_wav_info, any residue mod 16:
// a chunk of odd length in front of "data" leaves the samples at an ODD address --, where its frames go in the batch
// and how many they are.  The frames are contiguous little-endian int16 from there, 4 608 bytes each.
//
// A streaming copy with a byte shift.  One wave takes a run of 1 KB of a stream's PCM per trip, 16 bytes per lane: two
// ALIGNED 16-byte loads (the second one is the neighbour lane's first: it comes from the L1), a uniform choice of five
// of the eight dwords (the shift in dwords is the same for a whole stream, so the branch is scalar) and four
// v_alignbyte_b32 for the shift in bytes; one aligned 16-byte store.  No byte or short accesses, no LDS.
//
// What is READ reaches up to 31 bytes behind a stream's last sample (the second load of the last lane); the image is
// allocated with kWavSlack bytes of room behind the last file.  What is TAKEN are exactly the n_frames * 4 608 bytes from the
// record's offset: the host has refused every file that ends inside its last frame (wav_frame_count), so
// they all lie inside the stream's own file and nothing of the neighbouring file in the image reaches a PCM frame.
#pragma once

namespace mp3s {

__global__ __launch_bounds__(256) void k_wav_gather(const uint8_t *__restrict__ image, const WavRun *__restrict__ runs, int run0,
                                                    int16_t *__restrict__ pcm)
{
    const WavRun r = runs[run0 + blockIdx.y];
    const size_t n16 = (size_t)r.n_frames * 288;                  // 16-byte pieces of the stream's PCM
    const uint32_t shift = (uint32_t)(r.src & 15u), dsh = shift >> 2, bsh = shift & 3u;
    const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(image + (r.src - shift));
    uint4 *__restrict__ dst = reinterpret_cast<uint4 *>(pcm + (size_t)r.first_frame * 2304);
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) {
        const uint4 a = src[i];
        uint4 o = a;
        if (shift) {                                              // (uniform)
            const uint4 b = src[i + 1];
            uint32_t d0, d1, d2, d3, d4;
            switch (dsh) {                                        // (uniform)
            case 0: d0 = a.x; d1 = a.y; d2 = a.z; d3 = a.w; d4 = b.x; break;
            case 1: d0 = a.y; d1 = a.z; d2 = a.w; d3 = b.x; d4 = b.y; break;
            case 2: d0 = a.z; d1 = a.w; d2 = b.x; d3 = b.y; d4 = b.z; break;
            default: d0 = a.w; d1 = b.x; d2 = b.y; d3 = b.z; d4 = b.w; break;
            }
            // v_alignbyte_b32: ({hi, lo} >> 8 * shift) & 0xffffffff -- the dword that starts bsh bytes into lo
            o.x = __builtin_amdgcn_alignbyte(d1, d0, bsh);
            o.y = __builtin_amdgcn_alignbyte(d2, d1, bsh);
            o.z = __builtin_amdgcn_alignbyte(d3, d2, bsh);
            o.w = __builtin_amdgcn_alignbyte(d4, d3, bsh);
        }
        dst[i] = o;
    }
}

// ---- k_wav_import: the streams of a batch that are NOT contiguous int16 stereo frames (MP3S_OPT_WAV_IMPORT) -> the same PCM buffer.
//
// Unsigned 8-bit, 16-, 24- and 32-bit integer and float32 samples of one or two channels become int16 stereo rows: the upper two
// bytes of an integer sample (8-bit: (u - 128) << 8), clamp(rint(x * 32768.0f)) of a float (round-half-even, NaN -> 0), a mono
// sample in both channels, zeros from row n_samples on (include/mp3s.h, mp3s_wav_import_info).
//
// The same shape as k_wav_gather: one grid row per stream, per lane and trip ONE aligned 16-byte store = 4 stereo rows, made of
// S = 4 rows x channels x bytes per sample = 4 .. 32 source bytes.  A lane's source bytes start at src + i * S: S is a multiple of
// four, so the shift in bytes is the stream's (src & 3), and the address modulo the load width W (the largest power of two that
// divides S, 16 at most) is the stream's too.  The lane loads S / W + 1 aligned units of W bytes, a uniform switch names the first
// dword (template DSH: the dwords stay in registers, nothing is indexed at run time), v_alignbyte_b32 shifts, and v_perm_b32 with
// constant selectors picks the two upper bytes of every sample.  Format, channels and both shifts are the same for a whole grid row:
// every branch on them is scalar.  No byte or short accesses, no LDS, no scratch.
//
// What is READ: only by lanes whose first row is a sample of the stream (the others store zeros without loading), from the aligned
// unit that holds the lane's first source byte over S / W + 1 units: less than S + W bytes from that first byte, of which at least
// one sample row (channels x bytes) lies inside the stream.  The over-read behind the last sample is therefore below
// S + W - channels x bytes <= 32 + 16 - 8 = 40 bytes (stereo 32-bit); kWavSlack (64) behind the last file of the image covers it.
// What is TAKEN: rows below n_samples, chosen by a select on the row number -- whatever the bytes behind a stream hold (the next
// file of the image, the slack) never reaches a PCM frame.
// row R (0..3) of a lane's piece: one dword [left int16 | right int16] out of the lane's dword-aligned source bytes s[]
template <int FMT, int CH, int R>
__device__ __forceinline__ uint32_t wav_import_row(const uint32_t *s)
{
    constexpr int BPS = FMT == MP3S_WAV_U8 ? 1 : FMT == MP3S_WAV_S16 ? 2 : FMT == MP3S_WAV_S24 ? 3 : 4;
    if constexpr (FMT == MP3S_WAV_F32) {
        int v[2];
#pragma unroll
        for (int c = 0; c < CH; c++) {
            const float x = __uint_as_float(s[R * CH + c]);
            const float y = fminf(fmaxf(__builtin_rintf(x * 32768.0f), -32768.0f), 32767.0f);
            v[c] = x != x ? 0 : (int)y;
        }
        return ((uint32_t)v[0] & 0xffffu) | (((uint32_t)v[CH - 1] & 0xffffu) << 16);
    } else {
        // bytes of the row's left and right sample that become the int16: the sample's upper two (8-bit: a zero and the byte)
        constexpr int hiL = R * CH * BPS + BPS - 1, hiR = hiL + (CH - 1) * BPS;
        constexpr int w0 = (BPS == 1 ? hiL : hiL - 1) / 4;                    // the dword the selection starts in; it ends in w0 + 1 at most
        constexpr uint32_t zero = 0x0c;                                        // v_perm_b32 selector for a constant 0x00
        constexpr uint32_t sel = BPS == 1 ? (zero | (uint32_t)(hiL - 4 * w0) << 8 | zero << 16 | (uint32_t)(hiR - 4 * w0) << 24)
                                          : ((uint32_t)(hiL - 1 - 4 * w0) | (uint32_t)(hiL - 4 * w0) << 8 | (uint32_t)(hiR - 1 - 4 * w0) << 16 | (uint32_t)(hiR - 4 * w0) << 24);
        static_assert(hiR - 4 * w0 < 8, "a row's bytes span two dwords at most");
        // v_perm_b32 D, S0, S1, sel: byte k of D = byte sel[k] of {S0, S1} (S1 = bytes 0..3, S0 = bytes 4..7)
        const uint32_t o = __builtin_amdgcn_perm(s[w0 + 1], s[w0], sel);
        return BPS == 1 ? o ^ 0x80008000u : o;                                 // (u - 128) << 8
    }
}

template <int FMT, int CH, int DSH>
__device__ __forceinline__ uint4 wav_import_piece(const uint8_t *__restrict__ p /* aligned to W */, uint32_t bsh)
{
    constexpr int BPS = FMT == MP3S_WAV_U8 ? 1 : FMT == MP3S_WAV_S16 ? 2 : FMT == MP3S_WAV_S24 ? 3 : 4;
    constexpr int S = 4 * CH * BPS, W = (S % 16 == 0) ? 16 : (S % 8 == 0) ? 8 : 4, ND = S / 4, NL = (S / W + 1) * (W / 4);
    uint32_t d[NL];
    if constexpr (W == 16) {
#pragma unroll
        for (int k = 0; k < NL / 4; k++) { const uint4 v = reinterpret_cast<const uint4 *>(p)[k]; d[4 * k] = v.x; d[4 * k + 1] = v.y; d[4 * k + 2] = v.z; d[4 * k + 3] = v.w; }
    } else if constexpr (W == 8) {
#pragma unroll
        for (int k = 0; k < NL / 2; k++) { const uint2 v = reinterpret_cast<const uint2 *>(p)[k]; d[2 * k] = v.x; d[2 * k + 1] = v.y; }
    } else {
#pragma unroll
        for (int k = 0; k < NL; k++) d[k] = reinterpret_cast<const uint32_t *>(p)[k];
    }
    uint32_t s[ND + 1];                                    // the lane's S source bytes, dword-aligned (s[ND]: never selected)
#pragma unroll
    for (int k = 0; k < ND; k++) s[k] = __builtin_amdgcn_alignbyte(d[DSH + k + 1], d[DSH + k], bsh);
    s[ND] = 0;
    return make_uint4(wav_import_row<FMT, CH, 0>(s), wav_import_row<FMT, CH, 1>(s), wav_import_row<FMT, CH, 2>(s), wav_import_row<FMT, CH, 3>(s));
}

template <int FMT, int CH>
__device__ __forceinline__ void wav_import_stream(const uint8_t *__restrict__ image, const WavImportRun &r, int16_t *__restrict__ pcm)
{
    constexpr int BPS = FMT == MP3S_WAV_U8 ? 1 : FMT == MP3S_WAV_S16 ? 2 : FMT == MP3S_WAV_S24 ? 3 : 4;
    constexpr int S = 4 * CH * BPS, W = (S % 16 == 0) ? 16 : (S % 8 == 0) ? 8 : 4;
    const size_t n16 = (size_t)r.n_frames * 288;                  // 16-byte pieces of the stream's PCM, 4 rows each
    const uint32_t shift = (uint32_t)(r.src & (uint64_t)(W - 1)), dsh = shift >> 2, bsh = shift & 3u;   // (uniform)
    const uint8_t *__restrict__ src = image + (r.src - shift);
    uint4 *__restrict__ dst = reinterpret_cast<uint4 *>(pcm + (size_t)r.first_frame * 2304);
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += stride) {
        const uint64_t row = (uint64_t)i * 4;
        uint4 o = make_uint4(0, 0, 0, 0);
        if (row < r.n_samples) {                                   // (lanes behind the stream's last sample load nothing)
            const uint8_t *p = src + i * S;
            if constexpr (W == 4) o = wav_import_piece<FMT, CH, 0>(p, bsh);
            else if constexpr (W == 8) o = dsh == 0 ? wav_import_piece<FMT, CH, 0>(p, bsh) : wav_import_piece<FMT, CH, 1>(p, bsh);   // (uniform)
            else {
                switch (dsh) {                                     // (uniform)
                case 0: o = wav_import_piece<FMT, CH, 0>(p, bsh); break;
                case 1: o = wav_import_piece<FMT, CH, 1>(p, bsh); break;
                case 2: o = wav_import_piece<FMT, CH, 2>(p, bsh); break;
                default: o = wav_import_piece<FMT, CH, 3>(p, bsh); break;
                }
            }
            const uint64_t left = r.n_samples - row;              // rows of this piece that are samples: zero by select, not by what memory holds
            o.y = left > 1 ? o.y : 0u; o.z = left > 2 ? o.z : 0u; o.w = left > 3 ? o.w : 0u;
        }
        dst[i] = o;
    }
}

__global__ __launch_bounds__(256) void k_wav_import(const uint8_t *__restrict__ image, const WavImportRun *__restrict__ runs, int run0,
                                                    int16_t *__restrict__ pcm)
{
    const WavImportRun r = runs[run0 + blockIdx.y];
    const bool mono = r.channels == 1;                             // (format and channels: uniform, scalar branches)
    switch (r.format) {
    case MP3S_WAV_U8:  if (mono) wav_import_stream<MP3S_WAV_U8, 1>(image, r, pcm); else wav_import_stream<MP3S_WAV_U8, 2>(image, r, pcm); break;
    case MP3S_WAV_S16: if (mono) wav_import_stream<MP3S_WAV_S16, 1>(image, r, pcm); else wav_import_stream<MP3S_WAV_S16, 2>(image, r, pcm); break;
    case MP3S_WAV_S24: if (mono) wav_import_stream<MP3S_WAV_S24, 1>(image, r, pcm); else wav_import_stream<MP3S_WAV_S24, 2>(image, r, pcm); break;
    case MP3S_WAV_S32: if (mono) wav_import_stream<MP3S_WAV_S32, 1>(image, r, pcm); else wav_import_stream<MP3S_WAV_S32, 2>(image, r, pcm); break;
    case MP3S_WAV_F32: if (mono) wav_import_stream<MP3S_WAV_F32, 1>(image, r, pcm); else wav_import_stream<MP3S_WAV_F32, 2>(image, r, pcm); break;
    default: break;                                                // (the host makes no such record)
    }
}

}  // namespace mp3s
