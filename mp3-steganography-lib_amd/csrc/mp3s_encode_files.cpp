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

// the same for either reader.  With `import` (MP3S_OPT_WAV_IMPORT) the header is wav_import_parse's, with its codes and texts; a
// 16-bit stereo file of whole frames is what the strict reader makes of it (the compatibility rule), so it keeps k_wav_gather
// With `resample` (MP3S_OPT_WAV_RESAMPLE, which implies the import reader) a file whose rate is not the target's is planned for
// k_wav_resample: samplerate and count are the OUTPUT's, n_samples and in_frames the input's
int wav_encode_plan(bool import, int resample, const uint8_t *wav, size_t len, int bitrate_kbps, const uint8_t *hide_bits, int n_hide, WavPlan *p)
{
    *p = WavPlan();
    if (!import && !resample) {
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
    const int rc = wav_import_parse(wav, len, bitrate_kbps, &w, &msg, resample, &rs);
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
static int resample_taps_dev(mp3s_ctx *c, int L, int M, const uint32_t **d_out)
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

namespace {

struct WavIn {
    const uint8_t *wav; size_t len;
    const uint8_t *hide; int n_hide;
    WavPlan p;
};

// the files `idx` to the device: their images up, the gather (and, for what it does not take, the import kernel) queued on the context's stream -> *d_pcm_out = [n_all][1152][2] int16 in
// the context's PCM buffer, the streams back to back in the order of idx (segs[k] = stream k).  Nothing is waited for; `runs` and the
// callers' bytes are read by copies in flight until the stream is synchronised.
// Streams of MP3S_OPT_WAV_RESAMPLE go the same way in two steps: k_wav_import lays their samples, at the source rate, into a scratch
// buffer of their own (sruns), k_wav_resample computes their frames of the PCM buffer from there (rruns).
struct WavRecords {
    std::vector<WavRun> runs;
    std::vector<WavImportRun> iruns, sruns;
    std::vector<WavResampleRun> rruns;
};

int wav_to_device(mp3s_ctx *c, const std::vector<WavIn> &in, const std::vector<int> &idx, std::vector<EncSeg> &segs, WavRecords &rec,
                  void **d_pcm_out, int64_t *n_all_out)
{
    std::vector<WavRun> &runs = rec.runs;
    std::vector<WavImportRun> &iruns = rec.iruns, &sruns = rec.sruns;
    std::vector<WavResampleRun> &rruns = rec.rruns;
    segs.assign(idx.size(), EncSeg());
    runs.clear(); iruns.clear(); sruns.clear(); rruns.clear();
    runs.reserve(idx.size());
    std::vector<size_t> at(idx.size());
    int64_t n_all = 0, max_frames = 0, max_iframes = 0, max_sframes = 0, max_rframes = 0, s_all = 0 /* frames of the resampler's scratch */;
    size_t img = 0, staged = 0, res_lds = 0;
    HIPCHK(hipSetDevice(c->device));                               // (in front of every allocation below, the tap tables' included)
    for (size_t k = 0; k < idx.size(); k++) {
        const WavIn &f = in[(size_t)idx[k]];
        segs[k].n_frames = (int)f.p.count; segs[k].hide = f.hide; segs[k].n_hide = f.n_hide;
        img = (img + 15) & ~(size_t)15;
        at[k] = img;
        if (f.p.resample) {
            const WavPlan &p = f.p;
            const uint32_t *d_taps = nullptr;
            const int rc = resample_taps_dev(c, p.L, p.M, &d_taps);
            if (rc) return rc;
            const uint32_t span = resample_span((uint32_t)p.L, (uint32_t)p.M, (uint32_t)p.T), pairs = (uint32_t)p.L * (uint32_t)p.T / 2;
            const bool lds = pairs <= kResTapsLds;
            sruns.push_back({(uint64_t)img + (uint64_t)p.data_offset, (uint64_t)p.n_samples, (uint32_t)s_all, (uint32_t)p.in_frames, (uint32_t)p.format, (uint32_t)p.channels});
            rruns.push_back({d_taps, (uint64_t)s_all * 1152, (uint64_t)p.n_samples, (uint64_t)p.n_out, (uint32_t)n_all, (uint32_t)p.count,
                             (uint32_t)p.L, (uint32_t)p.M, (uint32_t)p.T, span, p.channels == 1 ? 1u : 0u, lds ? 1u : 0u});
            res_lds = std::max(res_lds, ((size_t)span + (lds ? pairs : 0)) * 4);
            s_all += p.in_frames;
            max_sframes = std::max(max_sframes, p.in_frames); max_rframes = std::max(max_rframes, p.count);
            if (s_all > 0x7fffffff / 8) return fail(MP3S_E_ARG, "encode batch too large");
        } else wav_plan_record(f.p, img, (uint32_t)n_all, runs, iruns);
        const size_t need = f.p.need;
        if (need < kDirectUpload) staged = img + need;
        img += need;
        n_all += f.p.count;
        if (f.p.gather) max_frames = std::max(max_frames, f.p.count);
        else if (!f.p.resample) max_iframes = std::max(max_iframes, f.p.count);
        if (n_all > 0x7fffffff / 8) return fail(MP3S_E_ARG, "encode batch too large");
    }
    const size_t runs_at = (img + kWavSlack + 15) & ~(size_t)15;
    const size_t iruns_at = runs_at + ((runs.size() * sizeof(WavRun) + 15) & ~(size_t)15);
    const size_t sruns_at = iruns_at + ((iruns.size() * sizeof(WavImportRun) + 15) & ~(size_t)15);
    const size_t rruns_at = sruns_at + ((sruns.size() * sizeof(WavImportRun) + 15) & ~(size_t)15);
    uint8_t *d_image = (uint8_t *)c->grab(27, rruns_at + rruns.size() * sizeof(WavResampleRun));
    void *d_pcm = c->grab(7, (size_t)n_all * 4608);
    void *d_rows = rruns.empty() ? nullptr : c->grab(28, (size_t)s_all * 4608);
    if (!d_image || !d_pcm || (!rruns.empty() && !d_rows)) return fail(MP3S_E_NOMEM, "hipMalloc failed for %lld frames of WAV input", (long long)n_all);
    // long files go up from where they lie; short ones are laid end to end first, bytes as they are, and travel in runs
    // (one copy per run instead of one per file: a copy from ordinary memory costs its thread 10 us and more whatever its size)
    std::vector<uint8_t> &stage = c->h_blob;
    if (stage.size() < staged) stage.resize(staged);
    size_t run_lo = 0, run_hi = 0;
    auto flush = [&]() {
        if (run_hi > run_lo) HIPCHK(hipMemcpyAsync(d_image + run_lo, stage.data() + run_lo, run_hi - run_lo, hipMemcpyHostToDevice, c->stream));
        run_lo = run_hi = 0;
        return (int)MP3S_OK;
    };
    for (size_t k = 0; k < idx.size(); k++) {
        const WavIn &f = in[(size_t)idx[k]];
        const size_t need = f.p.need;
        if (need >= kDirectUpload) {
            const int rc = flush();
            if (rc) return rc;
            const double t0 = trace_on() ? now_ms() : 0;
            HIPCHK(hipMemcpyAsync(d_image + at[k], f.wav, need, hipMemcpyHostToDevice, c->stream));
            if (trace_on()) fprintf(stderr, "mp3s:   encode_files: queueing the copy of %zu bytes from the caller's memory took %.3f ms\n", need, now_ms() - t0);
        } else {
            if (run_hi == run_lo) run_lo = at[k];
            std::memcpy(stage.data() + at[k], f.wav, need);
            run_hi = at[k] + need;
        }
    }
    int rc = flush();
    if (rc) return rc;
    if (!runs.empty()) HIPCHK(hipMemcpyAsync(d_image + runs_at, runs.data(), runs.size() * sizeof(WavRun), hipMemcpyHostToDevice, c->stream));
    if (!iruns.empty()) HIPCHK(hipMemcpyAsync(d_image + iruns_at, iruns.data(), iruns.size() * sizeof(WavImportRun), hipMemcpyHostToDevice, c->stream));
    if (trace_on()) fprintf(stderr, "mp3s:   encode_files: %zu streams through k_wav_gather, %zu through k_wav_import\n", runs.size(), iruns.size());
    if (!rruns.empty()) {
        HIPCHK(hipMemcpyAsync(d_image + sruns_at, sruns.data(), sruns.size() * sizeof(WavImportRun), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(d_image + rruns_at, rruns.data(), rruns.size() * sizeof(WavResampleRun), hipMemcpyHostToDevice, c->stream));
        if (trace_on()) fprintf(stderr, "mp3s:   encode_files: %zu streams through k_wav_import and k_wav_resample\n", rruns.size());
        if (launch_wav_import(c->stream, d_image, (const WavImportRun *)(d_image + sruns_at), (int)sruns.size(), (int)max_sframes, (int16_t *)d_rows) ||
            launch_wav_resample(c->stream, (const uint32_t *)d_rows, (const WavResampleRun *)(d_image + rruns_at), (int)rruns.size(), (int)max_rframes, res_lds,
                                (int16_t *)d_pcm, &c->prof))
            return fail(MP3S_E_HIP, "resampling the WAV samples failed");
    }
    if (launch_wav_gather(c->stream, d_image, (const WavRun *)(d_image + runs_at), (int)runs.size(), (int)max_frames, (int16_t *)d_pcm) ||
        launch_wav_import(c->stream, d_image, (const WavImportRun *)(d_image + iruns_at), (int)iruns.size(), (int)max_iframes, (int16_t *)d_pcm))
        return fail(MP3S_E_HIP, "gathering the WAV samples failed");
    *d_pcm_out = d_pcm; *n_all_out = n_all;
    return MP3S_OK;
}

// the files `idx` (one sampling rate and bitrate) as one batch: images up, gather, encode_batch on the PCM in HBM.  The batch's
// bytes are kept in a new part of `top`; out[i] points into it.
int encode_group(mp3s_ctx *c, const std::vector<WavIn> &in, const std::vector<int> &idx, int samplerate, int kbps, mp3s_buf *top, mp3s_file *out)
{
    std::vector<EncSeg> segs;
    WavRecords rec;
    void *d_pcm = nullptr;
    int64_t n_all = 0;
    int rc = wav_to_device(c, in, idx, segs, rec, &d_pcm, &n_all);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    std::unique_ptr<mp3s_buf> part(new mp3s_buf());
    int passes = 0;
    rc = encode_batch(c, nullptr, (const int16_t *)d_pcm, segs, samplerate, kbps, part.get(), &passes, false);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }     // (the records are the source of copies that may still be in flight)
    for (size_t k = 0; k < idx.size(); k++) {
        mp3s_file &o = out[idx[k]];
        std::memset(&o, 0, sizeof o);
        o.data = part->mp3 + segs[k].mp3_off; o.len = segs[k].mp3_len;
        o.kbps = kbps; o.sampling_rate = samplerate; o.channels = 2; o.n_frames = segs[k].n_frames;
        o.hide_offset = segs[k].hide_offset;
        o.too_long = segs[k].hide_offset < (int64_t)segs[k].n_hide - 1 ? 1 : 0;
    }
    top->parts.push_back(std::move(part));
    return MP3S_OK;
}

}  // namespace

int encode_files_as(mp3s_ctx *c, bool import, int resample, const uint8_t *const *wavs, const size_t *lens, int n_files, const int32_t *bitrate_kbps,
                    const uint8_t *const *hide_bits, const int32_t *n_hide, mp3s_buf **owner, mp3s_file *out, int32_t *status)
{
    if (!c || !wavs || !lens || !bitrate_kbps || !owner || !out || n_files <= 0 || (hide_bits && !n_hide)) return fail(MP3S_E_ARG, "bad argument");
    std::unique_ptr<mp3s_buf> top(new mp3s_buf());
    std::vector<WavIn> in((size_t)n_files);
    std::vector<int32_t> st((size_t)n_files, MP3S_OK);
    std::vector<std::string> why((size_t)n_files);
    struct Group { int rate, kbps; std::vector<int> idx; };
    std::vector<Group> groups;
    for (int i = 0; i < n_files; i++) {
        WavIn &f = in[(size_t)i];
        std::memset(&out[i], 0, sizeof out[i]);
        f.wav = wavs[i]; f.len = lens[i];
        f.hide = hide_bits ? hide_bits[i] : nullptr; f.n_hide = hide_bits ? n_hide[i] : 0;
        st[(size_t)i] = wav_encode_plan(import, resample, f.wav, f.len, bitrate_kbps[i], f.hide, f.n_hide, &f.p);
        if (st[(size_t)i]) { why[(size_t)i] = mp3s_last_error(); continue; }
        size_t g = 0;
        while (g < groups.size() && (groups[g].rate != f.p.samplerate || groups[g].kbps != bitrate_kbps[i])) g++;
        if (g == groups.size()) groups.push_back({f.p.samplerate, bitrate_kbps[i], {}});
        groups[g].idx.push_back(i);
    }
    for (const Group &g : groups) {
        const int rc = encode_group(c, in, g.idx, g.rate, g.kbps, top.get(), out);
        if (!rc) continue;
        (void)hipStreamSynchronize(c->stream);   // (copies of the failed batch may still read the callers' bytes and the staging)
        // one file spoils its batch (a quantizer step that leaves the table ...): each file on its own, to name it
        std::string first = mp3s_last_error();
        for (int i : g.idx) {
            st[(size_t)i] = g.idx.size() == 1 ? rc : encode_group(c, in, std::vector<int>{i}, g.rate, g.kbps, top.get(), out);
            if (st[(size_t)i]) { why[(size_t)i] = g.idx.size() == 1 ? first : std::string(mp3s_last_error()); std::memset(&out[i], 0, sizeof out[i]); }
        }
    }
    int first_bad = MP3S_OK;
    for (int i = 0; i < n_files; i++) {
        if (status) status[i] = st[(size_t)i];
        if (st[(size_t)i] && !first_bad) { first_bad = st[(size_t)i]; fail(first_bad, "%s", why[(size_t)i].c_str()); }   // the text of the first file that failed
    }
    if (!status && first_bad) return first_bad;
    *owner = top.release();
    return MP3S_OK;
}

extern "C" {

int mp3s_encode_files(mp3s_ctx *c, const uint8_t *const *wavs, const size_t *lens, int n_files, const int32_t *bitrate_kbps,
                      const uint8_t *const *hide_bits, const int32_t *n_hide, mp3s_buf **owner, mp3s_file *out, int32_t *status)
{
    if (!c || !wavs || !lens || !bitrate_kbps || !owner || !out || n_files <= 0 || (hide_bits && !n_hide)) return fail(MP3S_E_ARG, "bad argument");   // (before the context is looked at)
    return encode_files_as(c, c->opt[MP3S_OPT_WAV_IMPORT] != 0, (int)c->opt[MP3S_OPT_WAV_RESAMPLE], wavs, lens, n_files, bitrate_kbps, hide_bits, n_hide, owner, out, status);
}

int mp3s_debug_wav_gather(mp3s_ctx *c, const uint8_t *const *wavs, const size_t *lens, int n_files, int16_t *pcm, int64_t cap_frames, int64_t *n_frames)
{
    if (!c || !wavs || !lens || !pcm || !n_frames || n_files <= 0) return fail(MP3S_E_ARG, "bad argument");
    std::vector<WavIn> in((size_t)n_files);
    std::vector<int> idx((size_t)n_files);
    int64_t total = 0;
    for (int i = 0; i < n_files; i++) {
        WavIn &f = in[(size_t)i];
        f.wav = wavs[i]; f.len = lens[i]; f.hide = nullptr; f.n_hide = 0;
        const int rc = wav_encode_plan(c->opt[MP3S_OPT_WAV_IMPORT] != 0, (int)c->opt[MP3S_OPT_WAV_RESAMPLE], f.wav, f.len, 128, nullptr, 0, &f.p);
        if (rc) return rc;
        idx[(size_t)i] = i; total += f.p.count;
    }
    *n_frames = total;
    if (total > cap_frames) return fail(MP3S_E_ARG, "%lld frames, room for %lld", (long long)total, (long long)cap_frames);
    std::vector<EncSeg> segs;
    WavRecords rec;
    void *d_pcm = nullptr;
    int64_t n_all = 0;
    int rc = wav_to_device(c, in, idx, segs, rec, &d_pcm, &n_all);
    if (!rc) rc = mp3s_dev_download(c, pcm, d_pcm, (size_t)n_all * 4608);
    else (void)hipStreamSynchronize(c->stream);
    return rc;
}

}  // extern "C"
