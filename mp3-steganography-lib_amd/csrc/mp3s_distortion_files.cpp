// C-ABI of the library (include/mp3s.h), part 3e: what hiding changed -- the exact PCM difference of pairs of MP3 files, on the frame
// of the list-of-files calls (mp3s_internal.h).  The files go the way of mp3s_decode_streams up to the point where their int16 PCM lies
// in HBM (decode_group with d_keep: one batch per channel count, A and B streams side by side in ONE buffer); there k_pcm_diff_frames
// and k_pcm_diff_pairs (k_pcmdiff.hpp) reduce every pair to a record.  40 bytes per pair come down, and 32 per compared frame when
// the profile is asked for; no PCM does.
#include <cmath>
#include <limits>

#include "mp3s_internal.h"

// out = a pair's record and what the host knows of its two streams: the ONE place a mp3s_pcm_pair_diff becomes an mp3s_pcm_distortion
// (n_frames records of n_samples compared samples in all)
void distortion_from_record(const mp3s_pcm_pair_diff &r, const ParsedStream &a, const ParsedStream &b, int64_t n_frames, int64_t n_samples,
                            const mp3s_pcm_frame_diff *profile, mp3s_pcm_distortion *out)
{
    std::memset(out, 0, sizeof *out);
    const ParsedStream &named = a.n_frames > 0 ? a : b;   // (a stream without a frame has no header to ask)
    out->err2 = r.err2; out->sig2 = r.sig2; out->n_diff = (int64_t)r.n_diff; out->first_diff = r.first_diff; out->max_abs = r.max_abs;
    out->channels = named.nch; out->sampling_rate = named.sampling_rate; out->n_frames = (int32_t)n_frames;
    out->n_samples = n_samples;
    out->rows_a = 1152 * pcm_frames(a); out->rows_b = 1152 * pcm_frames(b);
    const double inf = std::numeric_limits<double>::infinity();
    out->snr_db = r.err2 ? 10.0 * std::log10((double)r.sig2 / (double)r.err2) : inf;
    out->psnr_db = r.err2 ? 10.0 * std::log10(32767.0 * 32767.0 * (double)out->n_samples / (double)r.err2) : inf;
    out->profile = profile;
}

// The front of the pair-list calls: all 2 n files as ONE list (file i = a[i], file n + i = b[i]) through the front end of
// mp3s_decode_streams on the host threads, then per pair its code and text, or `empty(i)` for a pair one of whose streams has no frame
// (nothing for a decode batch), or `valid(i)`, which groups it or refuses it.
void pcm_pairs_front_end(const uint8_t *const *a, const size_t *a_lens, const uint8_t *const *b, const size_t *b_lens, int n_pairs, mp3s_multi &m,
                         FileStatus &fs, const std::function<void(int)> &empty, const std::function<void(int)> &valid)
{
    const int n_files = 2 * n_pairs;
    m.parsed.resize(n_files); m.scanned.resize(n_files); m.pcm.assign(n_files, nullptr); m.files.resize(n_files);
    std::vector<int32_t> fst((size_t)n_files, MP3S_OK);   // per file: the front end's code
    size_t total = 0;
    for (int i = 0; i < n_files; i++) {
        const uint8_t *f = i < n_pairs ? a[i] : b[i - n_pairs];
        const size_t len = i < n_pairs ? a_lens[i] : b_lens[i - n_pairs];
        if (!f) { fst[(size_t)i] = MP3S_E_ARG; continue; }
        m.files[i] = {f, len};
        total += len;
    }
    parallel_files(file_workers(n_files, total, host_threads16()), n_files, [&](int, int i) { if (!fst[(size_t)i]) fst[(size_t)i] = front_end(m, i); });
    for (int i = 0; i < n_pairs; i++) {
        const ParsedStream &pa = m.parsed[i], &pb = m.parsed[n_pairs + i];
        const int bad = fst[(size_t)i] ? i : (fst[(size_t)(n_pairs + i)] ? n_pairs + i : -1);
        if (bad >= 0) {
            fs.set(i, fst[(size_t)bad] == MP3S_E_ARG ? fail(MP3S_E_ARG, "pair %d: file %s: null pointer", i, bad < n_pairs ? "a" : "b")
                                                    : fail(fst[(size_t)bad], "pair %d: file %s: malformed or unsupported MP3 stream", i, bad < n_pairs ? "a" : "b"));
            continue;
        }
        if (pa.n_frames <= 0 || pb.n_frames <= 0) { empty(i); continue; }
        if (pa.nch != pb.nch) { fs.set(i, fail(MP3S_E_UNSUPPORTED, "pair %d: %d channel(s) against %d channel(s)", i, pa.nch, pb.nch)); continue; }
        if (pa.sampling_rate != pb.sampling_rate) {
            fs.set(i, fail(MP3S_E_UNSUPPORTED, "pair %d: a sampling rate of %d Hz against %d Hz", i, pa.sampling_rate, pb.sampling_rate));
            continue;
        }
        if (pa.nch < 1 || pa.nch > 2) { fs.set(i, fail(MP3S_E_MALFORMED, "pair %d: channel count %d", i, pa.nch)); continue; }
        valid(i);
    }
}

// decode_group may have replaced a stream's record by a whole-file parse on the host.  The batch's layout and the size of its PCM buffer
// stand on the frame counts read before it, and decode_group's own layout on the same ones: the scan and the parse are one walk
// (scan_core) over the same bytes, so a parse that succeeds finds the same frames and the same repeated last frame.  Held to it here,
// stream by stream.
int pcm_pairs_same_frames(const mp3s_multi &m, int n_pairs, const std::vector<int> &idx, const std::vector<int64_t> &na, const std::vector<int64_t> &nb)
{
    for (size_t k = 0; k < idx.size(); k++)
        if (pcm_frames(m.parsed[idx[k]]) != na[k] || pcm_frames(m.parsed[n_pairs + idx[k]]) != nb[k])
            return fail(MP3S_E_MALFORMED, "pair %d: the decode found other frame counts than the scan", idx[k]);
    return MP3S_OK;
}

namespace {

// The pairs `idx` (file idx[k] against file n_pairs + idx[k] of m, all of `nch` channels, every stream with a frame) as one batch: one
// decode of all their streams into pool slot 7, the two kernels behind it, one copy down.  What the results point into (the profile) is
// kept in a new part of `top`.
int diff_group(mp3s_ctx *c, mp3s_multi &m, int n_pairs, const std::vector<int> &idx, int nch, bool want_profile, mp3s_buf *top, mp3s_pcm_distortion *out)
{
    // ---- the batch's streams, A and B of a pair side by side, and where each lies in the PCM buffer (decode_group: frames back to back,
    //      a repeated last frame behind its stream)
    std::vector<int> streams;
    std::vector<mp3s_pcm_pair> pairs(idx.size());
    std::vector<int64_t> frames_a(idx.size()), frames_b(idx.size());
    int64_t rows_frames = 0, cmp_frames = 0;
    for (size_t k = 0; k < idx.size(); k++) {
        const int fa = idx[k], fb = n_pairs + idx[k];
        const int64_t na = pcm_frames(m.parsed[fa]), nb = pcm_frames(m.parsed[fb]), n = std::min(na, nb);
        if (rows_frames + na + nb > 0x7fffffff / 8) return fail(MP3S_E_ARG, "batch of more than %d frames is too large", 0x7fffffff / 8);
        pairs[k] = {(uint32_t)rows_frames, (uint32_t)(rows_frames + na), (uint32_t)n, (uint32_t)cmp_frames};
        streams.push_back(fa); streams.push_back(fb);
        frames_a[k] = na; frames_b[k] = nb;
        rows_frames += na + nb; cmp_frames += n;
    }
    // ---- the host-made inputs as one block [pairs | tiles], the results as one block [pair records | frame records]
    std::vector<PcmTile> tiles;
    if (!pcm_diff_tiles(pairs.data(), (int)pairs.size(), tiles)) return fail(MP3S_E_ARG, "too many frames to compare");
    const size_t o_tiles = up16(pairs.size() * sizeof(mp3s_pcm_pair)), in_bytes = o_tiles + tiles.size() * sizeof(PcmTile);
    const size_t o_frames = up16(pairs.size() * sizeof(mp3s_pcm_pair_diff)), res_bytes = o_frames + (size_t)cmp_frames * sizeof(mp3s_pcm_frame_diff),
                 down_bytes = want_profile ? res_bytes : pairs.size() * sizeof(mp3s_pcm_pair_diff);
    std::vector<uint8_t> &in = c->h_in;
    in.resize(in_bytes);
    std::memcpy(in.data(), pairs.data(), pairs.size() * sizeof(mp3s_pcm_pair));
    if (!tiles.empty()) std::memcpy(in.data() + o_tiles, tiles.data(), tiles.size() * sizeof(PcmTile));
    if (hipSetDevice(c->device) != hipSuccess) return fail(MP3S_E_HIP, "hipSetDevice failed");
    void *d_keep = c->grab(7, (size_t)rows_frames * 1152 * nch * 2);
    uint8_t *d_in = (uint8_t *)c->grab(9, in_bytes), *d_res = (uint8_t *)c->grab(18, res_bytes);
    if (!d_keep || !d_in || !d_res) return fail(MP3S_E_NOMEM, "hipMalloc failed for %lld frames of PCM", (long long)rows_frames);
    std::unique_ptr<mp3s_buf> part(new mp3s_buf());
    if (!part->big[2].reserve(down_bytes)) return fail(MP3S_E_NOMEM, "host memory for %zu bytes of records", down_bytes);
    uint8_t *const res = part->big[2].data();
    int rc = decode_group(c, m, streams, nch, MP3S_PCM_I16, d_keep);
    if (!rc) rc = pcm_pairs_same_frames(m, n_pairs, idx, frames_a, frames_b);
    if (!rc && hipMemcpyAsync(d_in, in.data(), in_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = fail(MP3S_E_HIP, "input upload failed");
    if (!rc) {
        const int e = launch_pcm_diff(c->stream, (const int16_t *)d_keep, nch, (const mp3s_pcm_pair *)d_in, (int)pairs.size(), (const PcmTile *)(d_in + o_tiles),
                                      (int)tiles.size(), (mp3s_pcm_frame_diff *)(d_res + o_frames), (mp3s_pcm_pair_diff *)d_res);
        if (e) rc = fail(MP3S_E_HIP, "pcm diff launch: %s", hipGetErrorString((hipError_t)e));
    }
    if (!rc && hipMemcpyAsync(res, d_res, down_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = fail(MP3S_E_HIP, "download failed");
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail(MP3S_E_HIP, "sync failed");   // (also on failure: `in` is the source of a copy)
    if (rc) return rc;
    if (trace_on())
        fprintf(stderr, "mp3s:   pcm distortion: %zu pair(s) of %d channel(s), %lld frames decoded, %lld compared in %zu workgroup(s), %zu bytes down\n", idx.size(), nch,
                (long long)rows_frames, (long long)cmp_frames, tiles.size(), down_bytes);
    const mp3s_pcm_pair_diff *rec = (const mp3s_pcm_pair_diff *)res;
    const mp3s_pcm_frame_diff *frames = want_profile ? (const mp3s_pcm_frame_diff *)(res + o_frames) : nullptr;
    for (size_t k = 0; k < idx.size(); k++)
        distortion_from_record(rec[k], m.parsed[idx[k]], m.parsed[n_pairs + idx[k]], pairs[k].n_frames, (int64_t)pairs[k].n_frames * 1152 * nch, frames ? frames + pairs[k].out_first : nullptr, &out[idx[k]]);
    top->parts.push_back(std::move(part));
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
    // the table of the call before may still be on its way: its copy reads the vector that is written next
    if (c->ev_pcm_tiles) HIPCHK(hipEventSynchronize(c->ev_pcm_tiles));
    else HIPCHK(hipEventCreateWithFlags(&c->ev_pcm_tiles, hipEventDisableTiming));
    std::vector<PcmTile> &tiles = c->h_pcm_tiles;
    tiles.clear();
    if (!pcm_diff_tiles(h_pairs, n_pairs, tiles)) return fail(MP3S_E_ARG, "too many frames to compare");
    void *d_tiles = c->grab(9, tiles.size() * sizeof(PcmTile));
    if (!d_tiles) return fail(MP3S_E_NOMEM, "hipMalloc failed for %zu workgroup entries", tiles.size());
    if (!tiles.empty()) HIPCHK(hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(PcmTile), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->ev_pcm_tiles, c->stream));
    const int e = launch_pcm_diff(c->stream, d_pcm, nch, d_pairs, n_pairs, (const PcmTile *)d_tiles, (int)tiles.size(), d_frames, d_out);
    if (e) return fail(MP3S_E_HIP, "pcm diff launch: %s", hipGetErrorString((hipError_t)e));
    return MP3S_OK;
}

int mp3s_pcm_distortion_files(mp3s_ctx *c, const uint8_t *const *a, const size_t *a_lens, const uint8_t *const *b, const size_t *b_lens, int n_pairs,
                              int want_profile, mp3s_buf **owner, mp3s_pcm_distortion *out, int32_t *status)
{
    if (!c || !a || !a_lens || !b || !b_lens || !owner || !out || n_pairs <= 0) return fail(MP3S_E_ARG, "bad argument");
    if (n_pairs > 0x3fffffff) return fail(MP3S_E_ARG, "n_pairs=%d", n_pairs);
    // ---- the front of mp3s_decode_streams for all 2 n files as ONE list: file i = a[i], file n + i = b[i]
    std::unique_ptr<mp3s_buf> top(new mp3s_buf());
    top->multi.reset(new mp3s_multi());
    mp3s_multi &m = *top->multi;
    FileStatus fs(n_pairs);                               // per pair
    FileGroups groups;                                    // by channel count
    for (int i = 0; i < n_pairs; i++) std::memset(&out[i], 0, sizeof out[i]);
    const mp3s_pcm_pair_diff nothing = {0, 0, 0, -1, 0, 0};
    pcm_pairs_front_end(a, a_lens, b, b_lens, n_pairs, m, fs,
                        // nothing to compare (and nothing for a decode batch): the record of a pair of 0 frames
                        [&](int i) { distortion_from_record(nothing, m.parsed[i], m.parsed[n_pairs + i], 0, 0, nullptr, &out[i]); },
                        [&](int i) { groups.add(m.parsed[i].nch, 0, i); });
    // ---- per channel count: decode into HBM, compare there
    run_groups(groups, [&](int nch, int, const std::vector<int> &idx) {
        const int rc = diff_group(c, m, n_pairs, idx, nch, want_profile != 0, top.get(), out);
        if (rc) for (int i : idx) std::memset(&out[i], 0, sizeof out[i]);
        return rc;
    }, fs, [] {});
    m.files.clear();   // borrowed pointers
    m.parsed.clear(); m.scanned.clear();   // (the results point into the parts only)
    const int first_bad = finish_files(fs, status);
    if (!status && first_bad) return first_bad;
    *owner = top.release();
    return MP3S_OK;
}

}  // extern "C"
