// C-ABI of the library (include/mp3s.h), part 3b: a list of WAV files in, MP3 files out -- the files of one (sampling rate,
// bitrate) as ONE device batch.  The WAV bytes go to the device as the caller holds them; k_wav_gather (k_wav.hpp) -- and k_wav_import
// for the files only MP3S_OPT_WAV_IMPORT lets in -- make the PCM buffer of the batch out of them there, and encode_batch takes it from HBM as it takes the PCM a decode left.
#include "pipe_internal.h"

// what mp3s_encode_file checks of a file before the device sees it, in its order: the header (wav_parse: MP3S_E_EXIT with the
// reference's text, MP3S_E_MALFORMED), the frame count (wav_frame_count: MP3S_E_UNSUPPORTED), the message arguments
int wav_encode_check(const uint8_t *wav, size_t len, int bitrate_kbps, const uint8_t *hide_bits, int n_hide, mp3s_wav_info *w, int64_t *count)
{
    if (!wav) return fail(MP3S_E_ARG, "null pointer");
    const char *msg = "";
    int rc = wav_parse(wav, len, bitrate_kbps, w, &msg);
    if (!rc) rc = wav_frame_count(*w, count, &msg);
    if (rc) return fail(rc, "%s", msg);
    if (n_hide < 0 || (n_hide > 0 && !hide_bits)) return fail(MP3S_E_ARG, "bad hide arguments");
    if (*count > 0x7fffffff / 8) return fail(MP3S_E_ARG, "too many frames");
    return MP3S_OK;
}

WavRead wav_read_of(const mp3s_ctx *c)
{
    const int resample = (int)c->opt[MP3S_OPT_WAV_RESAMPLE];
    return {c->opt[MP3S_OPT_WAV_IMPORT] != 0 || resample != 0, resample};
}

// the same for either reader.  With how.import (MP3S_OPT_WAV_IMPORT) the header is wav_import_parse's, with its codes and texts; a
// 16-bit stereo file of whole frames is what the strict reader makes of it (the compatibility rule), so it keeps k_wav_gather
// With how.resample (MP3S_OPT_WAV_RESAMPLE) a file whose rate is not the target's is planned for
// k_wav_resample: samplerate and count are the OUTPUT's, n_samples and in_frames the input's
int wav_encode_plan(WavRead how, const uint8_t *wav, size_t len, int bitrate_kbps, const uint8_t *hide_bits, int n_hide, WavPlan *p)
{
    *p = WavPlan();
    if (!how.import) {
        mp3s_wav_info w;
        const int rc = wav_encode_check(wav, len, bitrate_kbps, hide_bits, n_hide, &w, &p->count);
        if (rc) return rc;
        p->samplerate = w.samplerate; p->format = MP3S_WAV_S16; p->channels = 2; p->data_offset = w.data_offset; p->n_samples = p->count * 1152;
        p->need = (size_t)w.data_offset + (size_t)p->count * 4608;   // (inside the file: wav_frame_count)
        return MP3S_OK;
    }
    if (!wav) return fail(MP3S_E_ARG, "null pointer");
    const char *msg = "";
    mp3s_wav_import w;
    mp3s_wav_resample rs;
    const int rc = wav_import_parse(wav, len, bitrate_kbps, &w, &msg, how.resample, &rs);
    if (rc) return fail(rc, "%s", msg);
    if (n_hide < 0 || (n_hide > 0 && !hide_bits)) return fail(MP3S_E_ARG, "bad hide arguments");
    if (w.n_frames > 0x7fffffff / 8 || rs.n_frames > 0x7fffffff / 8) return fail(MP3S_E_ARG, "too many frames");
    if (rs.L != rs.M) {
        p->samplerate = rs.out_rate; p->format = w.format; p->channels = w.channels; p->data_offset = w.data_offset;
        p->count = rs.n_frames; p->n_samples = w.n_samples;
        p->need = (size_t)w.data_offset + (size_t)w.n_samples * (size_t)w.block_align;
        p->gather = false; p->resample = true;
        p->L = rs.L; p->M = rs.M; p->T = rs.taps; p->in_frames = w.n_frames; p->n_out = rs.n_out;
        return MP3S_OK;
    }
    p->samplerate = w.samplerate; p->format = w.format; p->channels = w.channels; p->data_offset = w.data_offset;
    p->count = w.n_frames; p->n_samples = w.n_samples;
    p->need = (size_t)w.data_offset + (size_t)w.n_samples * (size_t)w.block_align;   // (inside the file: the samples present)
    p->gather = w.format == MP3S_WAV_S16 && w.channels == 2 && w.n_samples % 1152 == 0;
    return MP3S_OK;
}

// the packed tap table of a ratio on the device: made and uploaded when the context meets the ratio first, kept until it goes
int resample_taps_dev(mp3s_ctx *c, int L, int M, const uint32_t **d_out)
{
    for (const mp3s_ctx::ResampleTaps &t : c->res_taps)
        if (t.L == L && t.M == M) { *d_out = t.d; return MP3S_OK; }
    HIPCHK(hipSetDevice(c->device));                              // (the table belongs to the context's device whatever the thread selected last)
    std::vector<int32_t> taps;
    int T = 0;
    if (wav_resample_taps(L, M, taps, &T)) return fail(MP3S_E_EXIT, "Unsupported sampling frequency.");
    std::vector<uint32_t> packed(taps.size() / 2);                 // pairs of consecutive taps, int16 each (|c| < 2^15: 0.95 x 2^15 and the residual)
    for (size_t i = 0; i < packed.size(); i++) packed[i] = ((uint32_t)taps[2 * i] & 0xffffu) | ((uint32_t)taps[2 * i + 1] << 16);
    uint32_t *d = nullptr;
    if (hipMalloc((void **)&d, packed.size() * 4) != hipSuccess) { (void)hipGetLastError(); return fail(MP3S_E_NOMEM, "hipMalloc failed for a resampler's tap table"); }
    if (hipMemcpy(d, packed.data(), packed.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return fail(MP3S_E_HIP, "upload of a resampler's tap table failed"); }
    c->res_taps.push_back({L, M, T, d});
    *d_out = d;
    return MP3S_OK;
}

// the files `idx` to the device: their images up, the batch's kernels (launch_wav_batch) queued on the context's stream -> *d_pcm_out =
// [b.n_all][1152][2] int16 in the context's PCM buffer, the streams back to back in the order of idx (segs[k] = stream k).  Nothing is
// waited for; the batch's records and the callers' bytes are read by copies in flight until the stream is synchronised.
// Buffers: image and records in kPoolWavImage (the records behind the image and its slack), PCM in kPoolPcm0, the resampler's scratch in
// kPoolResampleRows, the short files' staging in h_blob.
int wav_to_device(mp3s_ctx *c, const std::vector<WavIn> &in, const std::vector<int> &idx, std::vector<EncSeg> &segs, WavBatch &b, void **d_pcm_out)
{
    segs.assign(idx.size(), EncSeg());
    b.clear();
    HIPCHK(hipSetDevice(c->device));                               // (in front of every allocation below, the tap tables' included)
    for (size_t k = 0; k < idx.size(); k++) {
        const WavIn &f = in[(size_t)idx[k]];
        segs[k].n_frames = (int)f.p.count; segs[k].hide = f.hide; segs[k].n_hide = f.n_hide;
        const uint32_t *d_taps = nullptr;
        int rc = f.p.resample ? resample_taps_dev(c, f.p.L, f.p.M, &d_taps) : MP3S_OK;
        if (!rc) rc = b.add(f.p, f.wav, d_taps);
        if (rc) return rc;
    }
    b.place_records(b.img + kWavSlack);
    uint8_t *d_image = (uint8_t *)c->grab(kPoolWavImage, b.rec_end);
    void *d_pcm = c->grab(kPoolPcm0, (size_t)b.n_all * 4608);
    void *d_rows = b.rruns.empty() ? nullptr : c->grab(kPoolResampleRows, (size_t)b.s_all * 4608);
    if (!d_image || !d_pcm || (!b.rruns.empty() && !d_rows)) return fail(MP3S_E_NOMEM, "hipMalloc failed for %lld frames of WAV input", (long long)b.n_all);
    std::vector<Upload> ups;
    plan_uploads(b.files, [&](size_t extent) { if (c->h_blob.size() < extent) c->h_blob.resize(extent); return c->h_blob.data(); }, ups);
    for (const Upload &u : ups) {
        const bool direct = u.src != c->h_blob.data() + u.dst;
        const double t0 = direct && trace_on() ? now_ms() : 0;
        HIPCHK(hipMemcpyAsync(d_image + u.dst, u.src, u.bytes, hipMemcpyHostToDevice, c->stream));
        if (direct && trace_on()) fprintf(stderr, "mp3s:   encode_files: queueing the copy of %zu bytes from the caller's memory took %.3f ms\n", u.bytes, now_ms() - t0);
    }
    for (const WavBatch::Part &p : b.parts())
        if (p.bytes) HIPCHK(hipMemcpyAsync(d_image + p.at, p.data, p.bytes, hipMemcpyHostToDevice, c->stream));
    if (trace_on()) fprintf(stderr, "mp3s:   encode_files: %zu streams through k_wav_gather, %zu through k_wav_import\n", b.runs.size(), b.iruns.size());
    if (trace_on() && !b.rruns.empty()) fprintf(stderr, "mp3s:   encode_files: %zu streams through k_wav_import and k_wav_resample\n", b.rruns.size());
    const int rc = launch_wav_batch(c->stream, d_image, d_image, b, (int16_t *)d_pcm, (int16_t *)d_rows, &c->prof);
    if (rc) return rc;
    *d_pcm_out = d_pcm;
    return MP3S_OK;
}

namespace {

// the files `idx` (one sampling rate and bitrate) as one batch: images up, gather, encode_batch on the PCM in HBM.  The batch's
// bytes are kept in a new part of `top`; out[i] points into it.
int encode_group(mp3s_ctx *c, const std::vector<WavIn> &in, const std::vector<int> &idx, int samplerate, int kbps, mp3s_buf *top, mp3s_file *out)
{
    std::vector<EncSeg> segs;
    WavBatch wb;
    void *d_pcm = nullptr;
    int rc = wav_to_device(c, in, idx, segs, wb, &d_pcm);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    std::unique_ptr<mp3s_buf> part(new mp3s_buf());
    int passes = 0;
    rc = encode_batch(c, nullptr, (const int16_t *)d_pcm, segs, samplerate, kbps, part.get(), &passes, false);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }     // (the records are the source of copies that may still be in flight)
    for (size_t k = 0; k < idx.size(); k++) file_from_seg(segs[k], part->mp3, kbps, samplerate, segs[k].hide_offset, &out[idx[k]]);
    top->parts.push_back(std::move(part));
    return MP3S_OK;
}

}  // namespace

int encode_files_as(mp3s_ctx *c, WavRead how, const uint8_t *const *wavs, const size_t *lens, int n_files, const int32_t *bitrate_kbps,
                    const uint8_t *const *hide_bits, const int32_t *n_hide, mp3s_buf **owner, mp3s_file *out, int32_t *status)
{
    if (!c || !wavs || !lens || !bitrate_kbps || !owner || !out || n_files <= 0 || (hide_bits && !n_hide)) return fail(MP3S_E_ARG, "bad argument");
    std::unique_ptr<mp3s_buf> top(new mp3s_buf());
    std::vector<WavIn> in((size_t)n_files);
    FileStatus fs(n_files);
    FileGroups groups;                       // by (sampling rate, kbps)
    for (int i = 0; i < n_files; i++) {
        WavIn &f = in[(size_t)i];
        std::memset(&out[i], 0, sizeof out[i]);
        f.wav = wavs[i]; f.len = lens[i];
        f.hide = hide_bits ? hide_bits[i] : nullptr; f.n_hide = hide_bits ? n_hide[i] : 0;
        fs.set(i, wav_encode_plan(how, f.wav, f.len, bitrate_kbps[i], f.hide, f.n_hide, &f.p));
        if (!fs.st[(size_t)i]) groups.add(f.p.samplerate, bitrate_kbps[i], i);
    }
    run_groups(groups, [&](int rate, int kbps, const std::vector<int> &idx) {
        const int rc = encode_group(c, in, idx, rate, kbps, top.get(), out);
        if (rc) for (int i : idx) std::memset(&out[i], 0, sizeof out[i]);
        return rc;
    }, fs, [&] { (void)hipStreamSynchronize(c->stream); });   // (copies of the failed batch may still read the callers' bytes and the staging)
    return finish_list(fs, status, top, owner);
}

extern "C" {

int mp3s_encode_files(mp3s_ctx *c, const uint8_t *const *wavs, const size_t *lens, int n_files, const int32_t *bitrate_kbps,
                      const uint8_t *const *hide_bits, const int32_t *n_hide, mp3s_buf **owner, mp3s_file *out, int32_t *status)
{
    if (!c || !wavs || !lens || !bitrate_kbps || !owner || !out || n_files <= 0 || (hide_bits && !n_hide)) return fail(MP3S_E_ARG, "bad argument");   // (before the context is looked at)
    return encode_files_as(c, wav_read_of(c), wavs, lens, n_files, bitrate_kbps, hide_bits, n_hide, owner, out, status);
}

int mp3s_debug_wav_gather(mp3s_ctx *c, const uint8_t *const *wavs, const size_t *lens, int n_files, int16_t *pcm, int64_t cap_frames, int64_t *n_frames)
{
    if (!c || !wavs || !lens || !pcm || !n_frames || n_files <= 0) return fail(MP3S_E_ARG, "bad argument");
    std::vector<WavIn> in((size_t)n_files);
    std::vector<int> idx((size_t)n_files);
    const WavRead how = wav_read_of(c);
    int64_t total = 0;
    for (int i = 0; i < n_files; i++) {
        WavIn &f = in[(size_t)i];
        f.wav = wavs[i]; f.len = lens[i]; f.hide = nullptr; f.n_hide = 0;
        const int rc = wav_encode_plan(how, f.wav, f.len, 128, nullptr, 0, &f.p);
        if (rc) return rc;
        idx[(size_t)i] = i; total += f.p.count;
    }
    *n_frames = total;
    if (total > cap_frames) return fail(MP3S_E_ARG, "%lld frames, room for %lld", (long long)total, (long long)cap_frames);
    std::vector<EncSeg> segs;
    WavBatch wb;
    void *d_pcm = nullptr;
    int rc = wav_to_device(c, in, idx, segs, wb, &d_pcm);
    if (!rc) rc = mp3s_dev_download(c, pcm, d_pcm, (size_t)wb.n_all * 4608);
    else (void)hipStreamSynchronize(c->stream);
    return rc;
}

}  // extern "C"
