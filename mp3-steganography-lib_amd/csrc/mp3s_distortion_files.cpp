// C-ABI of the library (include/mp3s.h), part 3e: what hiding changed -- the exact PCM difference of pairs of MP3 files, on the frame
// of the pair-list calls (pcm_pairs.cpp).  With the int16 PCM of a group's A and B streams in HBM, k_pcm_diff_frames and
// k_pcm_diff_pairs (k_pcmdiff.hpp) reduce every pair to a record.  40 bytes per pair come down, and 32 per compared frame when
// the profile is asked for; no PCM does.
#include "mp3s_internal.h"

namespace {

// The pairs `idx` as one batch (PcmPairBatch): the two kernels behind the decode, the pair records down and with the profile the frame
// records, which the results then point into.
int diff_group(mp3s_ctx *c, mp3s_multi &m, int n_pairs, const std::vector<int> &idx, int nch, bool want_profile, mp3s_buf *top, mp3s_pcm_distortion *out)
{
    PcmPairBatch b;
    if (const int rc = b.lay(m, n_pairs, idx, 0x7fffffff / 8)) return rc;
    std::vector<mp3s_pcm_pair> pairs(idx.size());
    for (size_t k = 0; k < idx.size(); k++)
        pairs[k] = {(uint32_t)b.first[k], (uint32_t)(b.first[k] + b.frames_a[k]), (uint32_t)std::min(b.frames_a[k], b.frames_b[k]), (uint32_t)b.out_first[k]};
    // ---- the host-made inputs as one block [pairs | tiles], the results as one block [pair records | frame records]
    std::vector<PcmTile> tiles;
    if (!pcm_diff_tiles(pairs.data(), (int)pairs.size(), tiles)) return fail(MP3S_E_ARG, "too many frames to compare");
    const size_t o_tiles = up16(pairs.size() * sizeof(mp3s_pcm_pair)), in_bytes = o_tiles + tiles.size() * sizeof(PcmTile);
    const size_t o_frames = up16(pairs.size() * sizeof(mp3s_pcm_pair_diff)), res_bytes = o_frames + (size_t)b.cmp_frames * sizeof(mp3s_pcm_frame_diff),
                 down_bytes = want_profile ? res_bytes : pairs.size() * sizeof(mp3s_pcm_pair_diff);
    std::vector<uint8_t> &in = c->h_in;
    in.resize(in_bytes);
    std::memcpy(in.data(), pairs.data(), pairs.size() * sizeof(mp3s_pcm_pair));
    if (!tiles.empty()) std::memcpy(in.data() + o_tiles, tiles.data(), tiles.size() * sizeof(PcmTile));
    const int rc = b.run(c, m, nch, in.data(), in_bytes, res_bytes, down_bytes, [&](const int16_t *d_pcm, const uint8_t *d_in, uint8_t *d_res) {
        const int e = launch_pcm_diff(c->stream, d_pcm, nch, (const mp3s_pcm_pair *)d_in, (int)pairs.size(), (const PcmTile *)(d_in + o_tiles),
                                      (int)tiles.size(), (mp3s_pcm_frame_diff *)(d_res + o_frames), (mp3s_pcm_pair_diff *)d_res);
        return e ? fail(MP3S_E_HIP, "pcm diff launch: %s", hipGetErrorString((hipError_t)e)) : MP3S_OK;
    });
    if (rc) return rc;
    if (trace_on())
        fprintf(stderr, "mp3s:   pcm distortion: %zu pair(s) of %d channel(s), %lld frames decoded, %lld compared in %zu workgroup(s), %zu bytes down\n", idx.size(), nch,
                (long long)b.rows_frames, (long long)b.cmp_frames, tiles.size(), down_bytes);
    const mp3s_pcm_pair_diff *rec = (const mp3s_pcm_pair_diff *)b.res;
    const mp3s_pcm_frame_diff *frames = want_profile ? (const mp3s_pcm_frame_diff *)(b.res + o_frames) : nullptr;
    for (size_t k = 0; k < idx.size(); k++)
        distortion_from_record(rec[k], m.parsed[idx[k]], m.parsed[n_pairs + idx[k]], pairs[k].n_frames, (int64_t)pairs[k].n_frames * 1152 * nch, frames ? frames + pairs[k].out_first : nullptr, &out[idx[k]]);
    top->parts.push_back(std::move(b.part));
    return MP3S_OK;
}

}  // namespace

extern "C" {

int mp3s_pcm_diff_dev(mp3s_ctx *c, const int16_t *d_pcm, int nch, const mp3s_pcm_pair *d_pairs, const mp3s_pcm_pair *h_pairs, int n_pairs,
                      mp3s_pcm_frame_diff *d_frames, mp3s_pcm_pair_diff *d_out)
{
    if (!c || !d_pcm || !d_pairs || !h_pairs || !d_frames || !d_out) return fail(MP3S_E_ARG, "null pointer");
    if (n_pairs <= 0) return fail(MP3S_E_ARG, "n_pairs=%d", n_pairs);
    if (nch != 1 && nch != 2) return fail(MP3S_E_ARG, "nch=%d", nch);
    if ((uintptr_t)d_pcm & 15) return fail(MP3S_E_ARG, "d_pcm is not 16-byte aligned");
    HIPCHK(hipSetDevice(c->device));
    std::vector<PcmTile> &tiles = c->h_pcm_tiles;
    void *d_tiles = nullptr;
    const int rc = pcm_dev_host_block(c, [&]() {
        tiles.clear();
        if (!pcm_diff_tiles(h_pairs, n_pairs, tiles)) return fail(MP3S_E_ARG, "too many frames to compare");
        d_tiles = c->grab(kPoolInputs, tiles.size() * sizeof(PcmTile));
        if (!d_tiles) return fail(MP3S_E_NOMEM, "hipMalloc failed for %zu workgroup entries", tiles.size());
        if (!tiles.empty()) HIPCHK(hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(PcmTile), hipMemcpyHostToDevice, c->stream));
        return (int)MP3S_OK;
    });
    if (rc) return rc;
    const int e = launch_pcm_diff(c->stream, d_pcm, nch, d_pairs, n_pairs, (const PcmTile *)d_tiles, (int)tiles.size(), d_frames, d_out);
    if (e) return fail(MP3S_E_HIP, "pcm diff launch: %s", hipGetErrorString((hipError_t)e));
    return MP3S_OK;
}

int mp3s_pcm_distortion_files(mp3s_ctx *c, const uint8_t *const *a, const size_t *a_lens, const uint8_t *const *b, const size_t *b_lens, int n_pairs,
                              int want_profile, mp3s_buf **owner, mp3s_pcm_distortion *out, int32_t *status)
{
    if (!c || !a || !a_lens || !b || !b_lens || !owner || !out || n_pairs <= 0) return fail(MP3S_E_ARG, "bad argument");
    if (n_pairs > 0x3fffffff) return fail(MP3S_E_ARG, "n_pairs=%d", n_pairs);
    const mp3s_pcm_pair_diff nothing = {0, 0, 0, -1, 0, 0};
    return pcm_pairs_call(c, a, a_lens, b, b_lens, n_pairs, out, sizeof *out, owner, status,
                          // nothing to compare (and nothing for a decode batch): the record of a pair of 0 frames
                          [&](const mp3s_multi &m, int i) { distortion_from_record(nothing, m.parsed[i], m.parsed[n_pairs + i], 0, 0, nullptr, &out[i]); },
                          nullptr,
                          [&](mp3s_multi &m, const std::vector<int> &idx, int nch, mp3s_buf *top) { return diff_group(c, m, n_pairs, idx, nch, want_profile != 0, top, out); });
}

}  // extern "C"
