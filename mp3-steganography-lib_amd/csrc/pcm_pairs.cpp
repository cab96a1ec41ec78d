// Pairs of MP3 files whose int16 PCM is compared on the device (mp3s_internal.h): what mp3s_pcm_distortion_files and
// mp3s_pcm_alignment_files share.  The files go the way of mp3s_decode_streams up to the point where their PCM lies in HBM
// (decode_group with d_keep: one batch per channel count, A and B streams side by side in ONE buffer); what runs there, what it
// reads and what comes down is the caller's (PcmPairBatch::run).  No PCM comes down.
#include <cmath>
#include <limits>

#include "mp3s_internal.h"

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

int PcmPairBatch::lay(const mp3s_multi &m, int n_pairs_, const std::vector<int> &idx_, int64_t max_frames)
{
    n_pairs = n_pairs_; idx = &idx_;
    const size_t n = idx_.size();
    first.resize(n); frames_a.resize(n); frames_b.resize(n); out_first.resize(n);
    for (size_t k = 0; k < n; k++) {
        const int fa = idx_[k], fb = n_pairs + idx_[k];
        const int64_t na = pcm_frames(m.parsed[fa]), nb = pcm_frames(m.parsed[fb]);
        if (rows_frames + na + nb > max_frames) return fail(MP3S_E_ARG, "batch of more than %d frames is too large", (int)max_frames);
        first[k] = rows_frames; frames_a[k] = na; frames_b[k] = nb; out_first[k] = cmp_frames;
        streams.push_back(fa); streams.push_back(fb);
        rows_frames += na + nb; cmp_frames += std::min(na, nb);
    }
    return MP3S_OK;
}

int PcmPairBatch::run(mp3s_ctx *c, mp3s_multi &m, int nch, const uint8_t *in, size_t in_bytes, size_t res_bytes, size_t down_bytes,
                      const std::function<int(const int16_t *d_pcm, const uint8_t *d_in, uint8_t *d_res)> &launch)
{
    if (hipSetDevice(c->device) != hipSuccess) return fail(MP3S_E_HIP, "hipSetDevice failed");
    void *d_keep = c->grab(kPoolPcm0, (size_t)rows_frames * 1152 * nch * 2);
    uint8_t *d_in = (uint8_t *)c->grab(kPoolInputs, in_bytes), *d_res = (uint8_t *)c->grab(kPoolSmall, res_bytes);
    if (!d_keep || !d_in || !d_res) return fail(MP3S_E_NOMEM, "hipMalloc failed for %lld frames of PCM", (long long)rows_frames);
    part.reset(new mp3s_buf());
    if (!part->big[2].reserve(down_bytes)) return fail(MP3S_E_NOMEM, "host memory for %zu bytes of records", down_bytes);
    res = part->big[2].data();
    int rc = decode_group(c, m, streams, nch, MP3S_PCM_I16, d_keep);
    // decode_group may have replaced a stream's record by a whole-file parse on the host.  The batch's layout and the size of its PCM
    // buffer stand on the frame counts read before it, and decode_group's own layout on the same ones: the scan and the parse are one
    // walk (scan_core) over the same bytes, so a parse that succeeds finds the same frames and the same repeated last frame.  Held to
    // it here, stream by stream.
    for (size_t k = 0; !rc && k < idx->size(); k++)
        if (pcm_frames(m.parsed[(*idx)[k]]) != frames_a[k] || pcm_frames(m.parsed[n_pairs + (*idx)[k]]) != frames_b[k])
            rc = fail(MP3S_E_MALFORMED, "pair %d: the decode found other frame counts than the scan", (*idx)[k]);
    if (!rc && hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = fail(MP3S_E_HIP, "input upload failed");
    if (!rc) rc = launch((const int16_t *)d_keep, d_in, d_res);
    if (!rc && hipMemcpyAsync(part->big[2].data(), d_res, down_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = fail(MP3S_E_HIP, "download failed");
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail(MP3S_E_HIP, "sync failed");   // (also on failure: `in` is the source of a copy)
    return rc;
}

int pcm_pairs_call(mp3s_ctx *c, const uint8_t *const *a, const size_t *a_lens, const uint8_t *const *b, const size_t *b_lens, int n_pairs, void *out,
                   size_t out_size, mp3s_buf **owner, int32_t *status, const std::function<void(const mp3s_multi &m, int i)> &empty,
                   const std::function<bool(const mp3s_multi &m, FileStatus &fs, int i)> &refuse,
                   const std::function<int(mp3s_multi &m, const std::vector<int> &idx, int nch, mp3s_buf *top)> &group)
{
    std::unique_ptr<mp3s_buf> top(new mp3s_buf());
    top->multi.reset(new mp3s_multi());
    mp3s_multi &m = *top->multi;
    FileStatus fs(n_pairs);                               // per pair
    FileGroups groups;                                    // by channel count
    std::memset(out, 0, (size_t)n_pairs * out_size);
    // ---- all 2 n files as ONE list: file i = a[i], file n + i = b[i]
    const std::vector<int32_t> fst = mp3_list_front(c, m, 2 * n_pairs, [&](int i) {
        return i < n_pairs ? std::pair<const uint8_t *, size_t>(a[i], a_lens[i]) : std::pair<const uint8_t *, size_t>(b[i - n_pairs], b_lens[i - n_pairs]);
    });
    for (int i = 0; i < n_pairs; i++) {
        const ParsedStream &pa = m.parsed[i], &pb = m.parsed[n_pairs + i];
        const int bad = fst[(size_t)i] ? i : (fst[(size_t)(n_pairs + i)] ? n_pairs + i : -1);
        if (bad >= 0) {
            fs.set(i, fst[(size_t)bad] == MP3S_E_ARG ? fail(MP3S_E_ARG, "pair %d: file %s: null pointer", i, bad < n_pairs ? "a" : "b")
                                                    : fail(fst[(size_t)bad], "pair %d: file %s: malformed or unsupported MP3 stream", i, bad < n_pairs ? "a" : "b"));
            continue;
        }
        if (pa.n_frames <= 0 || pb.n_frames <= 0) {       // nothing for a decode batch
            if (!refuse || !refuse(m, fs, i)) empty(m, i);
            continue;
        }
        if (pa.nch != pb.nch) { fs.set(i, fail(MP3S_E_UNSUPPORTED, "pair %d: %d channel(s) against %d channel(s)", i, pa.nch, pb.nch)); continue; }
        if (pa.sampling_rate != pb.sampling_rate) {
            fs.set(i, fail(MP3S_E_UNSUPPORTED, "pair %d: a sampling rate of %d Hz against %d Hz", i, pa.sampling_rate, pb.sampling_rate));
            continue;
        }
        if (pa.nch < 1 || pa.nch > 2) { fs.set(i, fail(MP3S_E_MALFORMED, "pair %d: channel count %d", i, pa.nch)); continue; }
        if (!refuse || !refuse(m, fs, i)) groups.add(pa.nch, 0, i);
    }
    // ---- per channel count: decode into HBM, the caller's passes there
    run_groups(groups, [&](int nch, int, const std::vector<int> &idx) {
        const int rc = group(m, idx, nch, top.get());
        if (rc) for (int i : idx) std::memset((uint8_t *)out + (size_t)i * out_size, 0, out_size);
        return rc;
    }, fs, [] {});
    mp3_list_done(c, m);
    m.parsed.clear(); m.scanned.clear();   // (the results point into the parts only)
    return finish_list(fs, status, top, owner);
}

int pcm_dev_host_block(mp3s_ctx *c, const std::function<int()> &fill_and_copy)
{
    if (c->ev_pcm_tiles) HIPCHK(hipEventSynchronize(c->ev_pcm_tiles));
    else HIPCHK(hipEventCreateWithFlags(&c->ev_pcm_tiles, hipEventDisableTiming));
    if (const int rc = fill_and_copy()) return rc;
    HIPCHK(hipEventRecord(c->ev_pcm_tiles, c->stream));
    return MP3S_OK;
}
