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
// allocated with that much room behind the last file.  What is TAKEN are exactly the n_frames * 4 608 bytes from the
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

}  // namespace mp3s
