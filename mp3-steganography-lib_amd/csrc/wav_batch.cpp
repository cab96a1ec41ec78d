// Files into a device image: which of them go up from where they lie and which through staging (plan_uploads, for the pipe's hide /
// decode jobs too), and the layout of a batch of WAV files with the launches that turn it into PCM (WavBatch, launch_wav_batch) --
// what mp3s_encode_files and the pipe's encode jobs share.  Plain host code; the buffers and the streams are the callers'.
#include "mp3s_internal.h"

constexpr size_t kDirectUpload = (size_t)256 << 10;   // a file at least this long goes up from the caller's memory in a copy of its own

bool plan_uploads(const std::vector<Upload> &files, const std::function<uint8_t *(size_t extent)> &staging, std::vector<Upload> &ups)
{
    ups.clear();
    size_t extent = 0;
    for (const Upload &f : files) if (f.bytes < kDirectUpload) extent = f.dst + f.bytes;
    uint8_t *stage = extent ? staging(extent) : nullptr;
    if (extent && !stage) return false;
    size_t run_lo = 0, run_hi = 0;   // the short files laid since the last long one
    auto flush = [&]() {
        if (run_hi > run_lo) ups.push_back({run_lo, stage + run_lo, run_hi - run_lo});
        run_lo = run_hi = 0;
    };
    for (const Upload &f : files) {
        if (f.bytes >= kDirectUpload) {
            flush();
            ups.push_back(f);
        } else {
            if (run_hi == run_lo) run_lo = f.dst;
            std::memcpy(stage + f.dst, f.src, f.bytes);
            run_hi = f.dst + f.bytes;
        }
    }
    flush();
    return true;
}

void WavBatch::clear()
{
    files.clear(); first.clear(); runs.clear(); iruns.clear(); sruns.clear(); rruns.clear();
    max_frames = max_iframes = max_sframes = max_rframes = n_all = s_all = 0;
    img = res_lds = o_runs = o_iruns = o_sruns = o_rruns = rec_end = 0;
}

int WavBatch::add(const WavPlan &p, const uint8_t *wav, const uint32_t *d_taps)
{
    img = up16(img);
    const uint64_t src = (uint64_t)img + (uint64_t)p.data_offset;
    if (p.resample) {
        const uint32_t span = resample_span((uint32_t)p.L, (uint32_t)p.M, (uint32_t)p.T), pairs = (uint32_t)p.L * (uint32_t)p.T / 2;
        const bool lds = pairs <= kResTapsLds;
        sruns.push_back({src, (uint64_t)p.n_samples, (uint32_t)s_all, (uint32_t)p.in_frames, (uint32_t)p.format, (uint32_t)p.channels});
        rruns.push_back({d_taps, (uint64_t)s_all * 1152, (uint64_t)p.n_samples, (uint64_t)p.n_out, (uint32_t)n_all, (uint32_t)p.count,
                         (uint32_t)p.L, (uint32_t)p.M, (uint32_t)p.T, span, p.channels == 1 ? 1u : 0u, lds ? 1u : 0u});
        res_lds = std::max(res_lds, ((size_t)span + (lds ? pairs : 0)) * 4);
        s_all += p.in_frames;
        max_sframes = std::max(max_sframes, p.in_frames); max_rframes = std::max(max_rframes, p.count);
        if (s_all > 0x7fffffff / 8) return fail(MP3S_E_ARG, "encode batch too large");
    } else if (p.gather) {
        runs.push_back({src, (uint32_t)n_all, (uint32_t)p.count});
        max_frames = std::max(max_frames, p.count);
    } else {
        iruns.push_back({src, (uint64_t)p.n_samples, (uint32_t)n_all, (uint32_t)p.count, (uint32_t)p.format, (uint32_t)p.channels});
        max_iframes = std::max(max_iframes, p.count);
    }
    files.push_back({img, wav, p.need});
    first.push_back((uint32_t)n_all);
    img += p.need;
    n_all += p.count;
    if (n_all > 0x7fffffff / 8) return fail(MP3S_E_ARG, "encode batch too large");
    return MP3S_OK;
}

void WavBatch::place_records(size_t base)
{
    o_runs = up16(base);
    o_iruns = o_runs + up16(runs.size() * sizeof(WavRun));
    o_sruns = o_iruns + up16(iruns.size() * sizeof(WavImportRun));
    o_rruns = o_sruns + up16(sruns.size() * sizeof(WavImportRun));
    rec_end = o_rruns + rruns.size() * sizeof(WavResampleRun);
}

std::array<WavBatch::Part, 4> WavBatch::parts() const
{
    return {{{o_runs, runs.data(), runs.size() * sizeof(WavRun)}, {o_iruns, iruns.data(), iruns.size() * sizeof(WavImportRun)},
             {o_sruns, sruns.data(), sruns.size() * sizeof(WavImportRun)}, {o_rruns, rruns.data(), rruns.size() * sizeof(WavResampleRun)}}};
}

int launch_wav_batch(hipStream_t stream, const uint8_t *d_image, const uint8_t *d_records, const WavBatch &b, int16_t *d_pcm, int16_t *d_rows, Profiler *prof)
{
    if (launch_wav_import(stream, d_image, (const WavImportRun *)(d_records + b.o_sruns), (int)b.sruns.size(), (int)b.max_sframes, d_rows) ||
        launch_wav_resample(stream, (const uint32_t *)d_rows, (const WavResampleRun *)(d_records + b.o_rruns), (int)b.rruns.size(), (int)b.max_rframes, b.res_lds,
                            d_pcm, prof))
        return fail(MP3S_E_HIP, "resampling the WAV samples failed");
    if (launch_wav_gather(stream, d_image, (const WavRun *)(d_records + b.o_runs), (int)b.runs.size(), (int)b.max_frames, d_pcm) ||
        launch_wav_import(stream, d_image, (const WavImportRun *)(d_records + b.o_iruns), (int)b.iruns.size(), (int)b.max_iframes, d_pcm))
        return fail(MP3S_E_HIP, "gathering the WAV samples failed");
    return MP3S_OK;
}
