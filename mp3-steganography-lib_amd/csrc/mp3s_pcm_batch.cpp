// C-ABI of the library (include/mp3s.h), part 3f: PCM batches in the caller's device memory.  A list of MP3 files is decoded as
// mp3s_decode_streams decodes it up to the point where the int16 PCM lies in HBM (decode_group with d_keep, one batch per channel
// count); k_pcm_batch (k_pcmbatch.hpp) lays it into the caller's planar batch [B][C][T] there and no PCM comes down.  The other way
// k_pcm_unbatch makes the encoder's frames of such a batch and encode_batch takes them from HBM, as it takes the PCM a decode left.
// The calls that take a sampling rate: k_pcm_batch_resample (k_pcmresample.hpp) in the place of k_pcm_batch, every file with its own
// ratio in one launch; and k_pcm_unbatch into a scratch at the source rate with the WAV path's k_wav_resample behind it.
#include "mp3s_internal.h"

namespace {

inline size_t batch_elem(int fmt) { return fmt == MP3S_BATCH_F32 ? 4 : 2; }
inline bool batch_format_ok(int fmt) { return fmt == MP3S_BATCH_I16 || fmt == MP3S_BATCH_F32; }

// The host-made block of a launch, [items (item_bytes, may be 0: they are on the device already) | tiles], to kPoolInputs on the
// context's stream.  The block travels from the context's h_pcm_batch by the rule of pcm_dev_host_block.  *d_block: where it lies,
// the tiles at up16(item_bytes).
int batch_block_up(mp3s_ctx *c, const void *items, size_t item_bytes, const std::vector<PcmBatchTile> &tiles, const uint8_t **d_block)
{
    const size_t o_tiles = up16(item_bytes), bytes = o_tiles + tiles.size() * sizeof(PcmBatchTile);
    return pcm_dev_host_block(c, [&]() {
        std::vector<uint8_t> &h = c->h_pcm_batch;
        h.assign(bytes, 0);
        if (item_bytes) std::memcpy(h.data(), items, item_bytes);
        if (!tiles.empty()) std::memcpy(h.data() + o_tiles, tiles.data(), tiles.size() * sizeof(PcmBatchTile));
        void *d = c->grab(kPoolInputs, bytes);
        if (!d) return fail(MP3S_E_NOMEM, "hipMalloc failed for %zu workgroup entries", tiles.size());
        if (bytes) HIPCHK(hipMemcpyAsync(d, h.data(), bytes, hipMemcpyHostToDevice, c->stream));
        *d_block = (const uint8_t *)d;
        return (int)MP3S_OK;
    });
}

// what both directions check of the batch's shape before the context is looked at
int batch_shape_check(int channels, const char *what, int format, int64_t T)
{
    if (channels != 1 && channels != 2) return fail(MP3S_E_ARG, "%s=%d", what, channels);
    if (!batch_format_ok(format)) return fail(MP3S_E_ARG, "format=%d", format);
    if (T <= 0) return fail(MP3S_E_ARG, "T=%lld", (long long)T);
    return MP3S_OK;
}

// a file's (an item's) ratio: out / in = L / M in lowest terms, T taps per phase; 1 / 1: not resampled
struct PcmRatio { int L = 1, M = 1, T = 0; };
inline int64_t resampled_rows(int64_t n_in, int L, int M) { return (int64_t)(((unsigned __int128)n_in * (unsigned)L + (unsigned)M - 1) / (unsigned)M); }

// the record k_pcm_batch_resample takes of one item; the ratio's tap table goes to the device when the context meets it first
int resample_run(mp3s_ctx *c, int64_t src_row, int64_t n_in, int64_t first_row, int slot, const PcmRatio &q, int nch, PcmResampleRun *r)
{
    const bool copy = q.L == 1 && q.M == 1;
    const uint32_t *d_taps = nullptr;
    if (!copy)
        if (const int rc = resample_taps_dev(c, q.L, q.M, &d_taps)) return rc;
    const uint32_t L = (uint32_t)q.L, M = (uint32_t)q.M, taps = copy ? 0u : (uint32_t)q.T;
    *r = PcmResampleRun{d_taps, src_row, n_in, resampled_rows(n_in, q.L, q.M), first_row, L, M, taps, pcm_resample_span(L, M, taps),
                        !copy && L * (taps / 2) <= kResTapsLds ? 1u : 0u, nch == 1 ? 1u : 0u, slot, 0u};
    return MP3S_OK;
}

// [runs | tiles] up by the rule of batch_block_up, then the ONE k_pcm_batch_resample launch of the runs
int resample_launch(mp3s_ctx *c, const int16_t *d_pcm, int nch, const std::vector<PcmResampleRun> &runs, const std::vector<PcmBatchTile> &tiles,
                    int out_channels, int out_format, int64_t T, void *d_out)
{
    size_t lds = 0;
    for (const PcmResampleRun &r : runs) lds = std::max(lds, pcm_resample_lds(r));
    const uint8_t *d_block = nullptr;
    if (const int rc = batch_block_up(c, runs.data(), runs.size() * sizeof runs[0], tiles, &d_block)) return rc;
    const int e = launch_pcm_batch_resample(c->stream, d_pcm, nch, (const PcmResampleRun *)d_block, (const PcmBatchTile *)(d_block + up16(runs.size() * sizeof runs[0])),
                                            (int)tiles.size(), lds, out_channels, out_format, T, d_out);
    if (e) return fail(MP3S_E_HIP, "pcm batch resample launch: %s", hipGetErrorString((hipError_t)e));
    return MP3S_OK;
}

// batch_group with every slot at another rate: the same decode batch, file i's rows resampled by ratios[i] on their way into slot i
int batch_group_at(mp3s_ctx *c, mp3s_multi &m, const std::vector<int> &idx, int nch, const int64_t *first_rows, int64_t T, int out_channels,
                   int out_format, void *d_out, const std::vector<PcmRatio> &ratios)
{
    std::vector<int64_t> frames_of(idx.size());
    int64_t rows_frames = 0;                              // decode_group's layout: frames back to back, a repeated last frame behind its stream
    for (size_t k = 0; k < idx.size(); k++) {
        frames_of[k] = pcm_frames(m.parsed[idx[k]]);
        rows_frames += frames_of[k];
        if (rows_frames > 0x7fffffff / 8) return fail(MP3S_E_ARG, "batch of more than %d frames is too large", 0x7fffffff / 8);
    }
    std::vector<PcmBatchTile> tiles;
    if (!pcm_resample_tiles((int)idx.size(), T, tiles)) return fail(MP3S_E_ARG, "too many rows for one launch");
    void *d_keep = c->grab(kPoolPcm0, (size_t)rows_frames * 1152 * nch * 2);
    if (!d_keep) return fail(MP3S_E_NOMEM, "hipMalloc failed for %lld frames of PCM", (long long)rows_frames);
    int rc = decode_group(c, m, idx, nch, MP3S_PCM_I16, d_keep);
    std::vector<PcmResampleRun> runs(idx.size());
    int64_t at = 0;
    for (size_t k = 0; !rc && k < idx.size(); k++) {
        if (pcm_frames(m.parsed[idx[k]]) != frames_of[k]) { rc = fail(MP3S_E_MALFORMED, "file %d: the decode found other frame counts than the scan", idx[k]); break; }
        rc = resample_run(c, at * 1152, frames_of[k] * 1152, first_rows ? first_rows[idx[k]] : 0, idx[k], ratios[(size_t)idx[k]], nch, &runs[k]);
        at += frames_of[k];
    }
    if (!rc) rc = resample_launch(c, (const int16_t *)d_keep, nch, runs, tiles, out_channels, out_format, T, d_out);
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail(MP3S_E_HIP, "sync failed");
    if (trace_on())
        fprintf(stderr, "mp3s:   pcm batch: %zu stream(s) of %d channel(s), %lld frames decoded, %zu workgroup(s) of k_pcm_batch_resample\n", idx.size(), nch, (long long)rows_frames, tiles.size());
    return rc;
}

// The streams `idx` of m (one channel count, every one with a frame) as one decode batch, then one k_pcm_batch launch into the caller's
// d_out: file i's rows from first_row(i) on into slot i.  The stream is synchronised whatever happened.
// ratios (per file of m; NULL: nothing is resampled, the launch is k_pcm_batch's): k_pcm_batch_resample in its place, first_rows in output rows.
int batch_group(mp3s_ctx *c, mp3s_multi &m, const std::vector<int> &idx, int nch, const int64_t *first_rows, int64_t T, int out_channels,
                int out_format, void *d_out, const std::vector<PcmRatio> *ratios = nullptr)
{
    if (hipSetDevice(c->device) != hipSuccess) return fail(MP3S_E_HIP, "hipSetDevice failed");
    if (ratios) return batch_group_at(c, m, idx, nch, first_rows, T, out_channels, out_format, d_out, *ratios);
    std::vector<mp3s_pcm_batch_item> items(idx.size());
    int64_t rows_frames = 0;                              // decode_group's layout: frames back to back, a repeated last frame behind its stream
    for (size_t k = 0; k < idx.size(); k++) {
        const int64_t frames = pcm_frames(m.parsed[idx[k]]);
        items[k] = {rows_frames * 1152, frames * 1152, first_rows ? first_rows[idx[k]] : 0, idx[k], 0};
        rows_frames += frames;
        if (rows_frames > 0x7fffffff / 8) return fail(MP3S_E_ARG, "batch of more than %d frames is too large", 0x7fffffff / 8);
    }
    std::vector<PcmBatchTile> tiles;
    if (!pcm_batch_tiles((int)idx.size(), T, tiles)) return fail(MP3S_E_ARG, "too many rows for one launch");
    void *d_keep = c->grab(kPoolPcm0, (size_t)rows_frames * 1152 * nch * 2);
    if (!d_keep) return fail(MP3S_E_NOMEM, "hipMalloc failed for %lld frames of PCM", (long long)rows_frames);
    int rc = decode_group(c, m, idx, nch, MP3S_PCM_I16, d_keep);
    // (the layout stands on the frame counts read before the decode, as PcmPairBatch::run's does: held to it here)
    for (size_t k = 0; !rc && k < idx.size(); k++)
        if (pcm_frames(m.parsed[idx[k]]) * 1152 != items[k].n_rows) rc = fail(MP3S_E_MALFORMED, "file %d: the decode found other frame counts than the scan", idx[k]);
    const uint8_t *d_block = nullptr;
    if (!rc) rc = batch_block_up(c, items.data(), items.size() * sizeof items[0], tiles, &d_block);
    if (!rc) {
        const int e = launch_pcm_batch(c->stream, (const int16_t *)d_keep, nch, (const mp3s_pcm_batch_item *)d_block,
                                       (const PcmBatchTile *)(d_block + up16(items.size() * sizeof items[0])), (int)tiles.size(), out_channels, out_format, T, d_out);
        if (e) rc = fail(MP3S_E_HIP, "pcm batch launch: %s", hipGetErrorString((hipError_t)e));
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail(MP3S_E_HIP, "sync failed");
    if (trace_on())
        fprintf(stderr, "mp3s:   pcm batch: %zu stream(s) of %d channel(s), %lld frames decoded, %zu workgroup(s)\n", idx.size(), nch, (long long)rows_frames, tiles.size());
    return rc;
}

// The items `idx` of the caller's batch as one encode batch: k_pcm_unbatch into the context's PCM buffer, encode_batch from there.
// rs (NULL: the batch is at `samplerate`): the items are at another rate -- k_pcm_unbatch lays them into kPoolResampleRows, whose
// [frames][1152][2] int16 rows are the [L | R] dword rows k_wav_resample reads, and that kernel computes the PCM buffer at `samplerate`.
int encode_items(mp3s_ctx *c, const void *d_in, int in_channels, int in_format, int64_t T, const int64_t *n_rows, const uint8_t *const *hide_bits,
                 const int32_t *n_hide, const std::vector<int> &idx, int samplerate, int kbps, mp3s_buf *top, mp3s_file *out, const PcmRatio *rs = nullptr)
{
    HIPCHK(hipSetDevice(c->device));
    std::vector<EncSeg> segs(idx.size());
    std::vector<mp3s_pcm_unbatch_item> items(idx.size());
    std::vector<WavResampleRun> rruns(rs ? idx.size() : 0);
    const uint32_t *d_taps = nullptr;
    if (rs)
        if (const int rc = resample_taps_dev(c, rs->L, rs->M, &d_taps)) return rc;
    const uint32_t span = rs ? resample_span((uint32_t)rs->L, (uint32_t)rs->M, (uint32_t)rs->T) : 0, pairs = rs ? (uint32_t)rs->L * (uint32_t)rs->T / 2 : 0;
    int64_t n_all = 0, s_all = 0, max_frames = 0;         // frames of the PCM buffer, of the scratch at the source rate, of the longest stream
    for (size_t k = 0; k < idx.size(); k++) {
        const int i = idx[k];
        const int64_t in_frames = (n_rows[i] + 1151) / 1152, n_out = rs ? resampled_rows(n_rows[i], rs->L, rs->M) : n_rows[i], frames = (n_out + 1151) / 1152;
        items[k] = {rs ? s_all : n_all, n_rows[i], i, 0};
        if (rs)
            rruns[k] = WavResampleRun{d_taps, (uint64_t)s_all * 1152, (uint64_t)n_rows[i], (uint64_t)n_out, (uint32_t)n_all, (uint32_t)frames, (uint32_t)rs->L,
                                      (uint32_t)rs->M, (uint32_t)rs->T, span, in_channels == 1 ? 1u : 0u, pairs <= kResTapsLds ? 1u : 0u};
        segs[k].n_frames = (int)frames; segs[k].hide = hide_bits ? hide_bits[i] : nullptr; segs[k].n_hide = hide_bits ? n_hide[i] : 0;
        n_all += frames; s_all += in_frames; max_frames = std::max(max_frames, frames);
        if (n_all > 0x7fffffff / 8 || s_all > 0x7fffffff / 8) return fail(MP3S_E_ARG, "too many frames");
    }
    std::vector<PcmBatchTile> tiles;
    if (!pcm_unbatch_tiles(items.data(), (int)items.size(), tiles)) return fail(MP3S_E_ARG, "too many rows for one launch");
    void *d_pcm = c->grab(kPoolPcm0, (size_t)n_all * 4608);
    void *d_rows = rs ? c->grab(kPoolResampleRows, (size_t)s_all * 4608) : d_pcm;
    if (!d_pcm || !d_rows) return fail(MP3S_E_NOMEM, "hipMalloc failed for %lld frames of PCM", (long long)(n_all + (rs ? s_all : 0)));
    // the launches' records as ONE block: [unbatch items | resample runs | tiles]
    const size_t o_rruns = up16(items.size() * sizeof items[0]), rec_bytes = o_rruns + rruns.size() * sizeof(WavResampleRun);
    std::vector<uint8_t> recs(rec_bytes, 0);
    std::memcpy(recs.data(), items.data(), items.size() * sizeof items[0]);
    if (!rruns.empty()) std::memcpy(recs.data() + o_rruns, rruns.data(), rruns.size() * sizeof(WavResampleRun));
    const uint8_t *d_block = nullptr;
    int rc = batch_block_up(c, recs.data(), rec_bytes, tiles, &d_block);
    if (rc) return rc;
    const int e = launch_pcm_unbatch(c->stream, d_in, in_channels, in_format, T, (const mp3s_pcm_unbatch_item *)d_block,
                                     (const PcmBatchTile *)(d_block + up16(rec_bytes)), (int)tiles.size(), (int16_t *)d_rows);
    if (e) return fail(MP3S_E_HIP, "pcm unbatch launch: %s", hipGetErrorString((hipError_t)e));
    if (rs) {
        const int e2 = launch_wav_resample(c->stream, (const uint32_t *)d_rows, (const WavResampleRun *)(d_block + o_rruns), (int)rruns.size(), (int)max_frames,
                                           ((size_t)span + (pairs <= kResTapsLds ? pairs : 0)) * 4, (int16_t *)d_pcm, &c->prof);
        if (e2) return fail(MP3S_E_HIP, "resampling the batch failed: %s", hipGetErrorString((hipError_t)e2));
    }
    std::unique_ptr<mp3s_buf> part(new mp3s_buf());
    int passes = 0;
    rc = encode_batch(c, nullptr, (const int16_t *)d_pcm, segs, samplerate, kbps, part.get(), &passes, false);
    if (rc) return rc;
    for (size_t k = 0; k < idx.size(); k++) file_from_seg(segs[k], part->mp3, kbps, samplerate, segs[k].hide_offset, &out[idx[k]]);
    top->parts.push_back(std::move(part));
    return MP3S_OK;
}

// mp3s_pcm_batch_encode behind its argument checks: the items at `samplerate`, or (rs) resampled to it
int encode_list(mp3s_ctx *c, const void *d_in, int n_items, int in_channels, int in_format, int64_t T, const int64_t *n_rows, int samplerate,
                int bitrate_kbps, const uint8_t *const *hide_bits, const int32_t *n_hide, mp3s_buf **owner, mp3s_file *out, int32_t *status, const PcmRatio *rs)
{
    std::unique_ptr<mp3s_buf> top(new mp3s_buf());
    FileStatus fs(n_items);
    FileGroups groups;                                    // one: the call's (sampling rate, kbps)
    for (int i = 0; i < n_items; i++) {
        std::memset(&out[i], 0, sizeof out[i]);
        if (n_rows[i] < 1 || n_rows[i] > T) { fs.set(i, fail(MP3S_E_ARG, "item %d: n_rows=%lld outside [1, %lld]", i, (long long)n_rows[i], (long long)T)); continue; }
        if (hide_bits && (n_hide[i] < 0 || (n_hide[i] > 0 && !hide_bits[i]))) { fs.set(i, fail(MP3S_E_ARG, "item %d: bad hide arguments", i)); continue; }
        groups.add(samplerate, bitrate_kbps, i);
    }
    run_groups(groups, [&](int rate, int kbps, const std::vector<int> &idx) {
        const int rc = encode_items(c, d_in, in_channels, in_format, T, n_rows, hide_bits, n_hide, idx, rate, kbps, top.get(), out, rs);
        if (rc) for (int i : idx) std::memset(&out[i], 0, sizeof out[i]);
        return rc;
    }, fs, [&] { (void)hipStreamSynchronize(c->stream); });   // (copies of the failed batch may still read the context's host blocks)
    return finish_list(fs, status, top, owner);
}

// mp3s_pcm_batch_decode_files (Info = mp3s_pcm_batch_info: out_rate is not looked at) and mp3s_pcm_batch_decode_files_at (Info =
// mp3s_pcm_batch_info_at: every slot at out_rate) are ONE call: front end, groups, status rules and the zeroing of slots are shared
template <class Info>
int decode_files(mp3s_ctx *c, const uint8_t *const *mp3s, const size_t *lens, int n_files, int out_rate, const int64_t *first_rows, int64_t T,
                 int out_channels, int out_format, void *d_out, size_t out_bytes, Info *info, int32_t *status)
{
    constexpr bool kAt = std::is_same<Info, mp3s_pcm_batch_info_at>::value;
    if (!c || !mp3s || !lens || !info) return fail(MP3S_E_ARG, "null pointer");
    if (n_files <= 0) return fail(MP3S_E_ARG, "n_files=%d", n_files);
    if (kAt && out_rate <= 0) return fail(MP3S_E_ARG, "out_rate=%d", out_rate);
    if (out_channels != 1 && out_channels != 2) return fail(MP3S_E_ARG, "out_channels=%d", out_channels);
    if (!batch_format_ok(out_format)) return fail(MP3S_E_ARG, "format=%d", out_format);
    const size_t esz = batch_elem(out_format);
    size_t slot_bytes = 0;
    if (d_out) {
        if (T <= 0) return fail(MP3S_E_ARG, "T=%lld", (long long)T);
        if ((uintptr_t)d_out % esz) return fail(MP3S_E_ARG, "d_out is not aligned to an element");
        if ((uint64_t)T > (((uint64_t)1 << 40)) || (uint64_t)T * out_channels * esz > SIZE_MAX / (size_t)n_files) return fail(MP3S_E_ARG, "T=%lld is too large", (long long)T);
        slot_bytes = (size_t)T * (size_t)out_channels * esz;
        if (out_bytes < slot_bytes * (size_t)n_files) return fail(MP3S_E_ARG, "out_bytes=%zu, the batch takes %zu", out_bytes, slot_bytes * (size_t)n_files);
        for (int i = 0; first_rows && i < n_files; i++)
            if (first_rows[i] < 0) return fail(MP3S_E_ARG, "first_rows[%d]=%lld", i, (long long)first_rows[i]);
    }
    std::unique_ptr<mp3s_multi> mm(new mp3s_multi());
    mp3s_multi &m = *mm;
    FileStatus fs(n_files);
    FileGroups groups;                                    // by channel count
    std::vector<PcmRatio> ratios(kAt ? (size_t)n_files : 0);
    std::memset(info, 0, (size_t)n_files * sizeof *info);
    // (with status == NULL a file the front end refuses fails the call here, before any device work -- a null file before any work at all)
    for (int i = 0; i < n_files && !status; i++)
        if (!mp3s[i]) return fail(MP3S_E_ARG, "file %d is null", i);
    const std::vector<int32_t> frc = mp3_list_front(c, m, n_files, [&](int i) { return std::pair<const uint8_t *, size_t>(mp3s[i], lens[i]); });
    for (int i = 0; i < n_files; i++) {
        if (frc[(size_t)i]) {
            fs.set(i, mp3s[i] ? fail(frc[(size_t)i], "file %d: malformed or unsupported MP3 stream", i) : fail(MP3S_E_ARG, "file %d is null", i));
            if (!status) { mp3_list_done(c, m); return frc[(size_t)i]; }
            m.parsed[i] = ParsedStream();                 // nothing of it goes into a batch
            continue;
        }
        const ParsedStream &p = m.parsed[i];
        info[i].n_frames = p.n_frames; info[i].nch = p.nch; info[i].sampling_rate = p.sampling_rate; info[i].bit_rate = p.bit_rate;
        info[i].n_rows = 1152 * pcm_frames(p); info[i].first_row = first_rows ? first_rows[i] : 0;
        if constexpr (kAt) {
            info[i].in_rows = info[i].n_rows; info[i].out_rate = out_rate;
            if (p.n_frames > 0) {                         // (a file without a frame has no rate and no rows)
                PcmRatio &q = ratios[(size_t)i];
                int H = 0;
                if (pcm_resample_plan(p.sampling_rate, out_rate, &q.L, &q.M, &q.T, &H)) {
                    const int rc = fail(MP3S_E_UNSUPPORTED, "file %d: %d -> %d Hz is a ratio the resampler refuses", i, p.sampling_rate, out_rate);
                    fs.set(i, rc);
                    if (!status) { mp3_list_done(c, m); return rc; }
                    std::memset(&info[i], 0, sizeof info[i]);
                    m.parsed[i] = ParsedStream();
                    continue;
                }
                info[i].L = q.L; info[i].M = q.M;
                info[i].n_rows = resampled_rows(info[i].in_rows, q.L, q.M);
            }
        }
        if (d_out && p.n_frames > 0) groups.add(p.nch, 0, i);
    }
    if (d_out) {
        if (hipSetDevice(c->device) != hipSuccess) { mp3_list_done(c, m); return fail(MP3S_E_HIP, "hipSetDevice failed"); }
        run_groups(groups, [&](int nch, int, const std::vector<int> &idx) {
            return nch < 1 || nch > 2 ? fail(MP3S_E_MALFORMED, "channel count %d", nch)
                                      : batch_group(c, m, idx, nch, first_rows, T, out_channels, out_format, d_out, kAt ? &ratios : nullptr);
        }, fs, [] {});
        // what no batch has written: the slots of failed and of frameless files
        int hip_rc = MP3S_OK;
        for (int i = 0; i < n_files; i++) {
            if (fs.st[(size_t)i]) std::memset(&info[i], 0, sizeof info[i]);
            if (fs.st[(size_t)i] || info[i].n_frames <= 0) {
                if (hipMemsetAsync((uint8_t *)d_out + (size_t)i * slot_bytes, 0, slot_bytes, c->stream) != hipSuccess && !hip_rc) hip_rc = fail(MP3S_E_HIP, "hipMemsetAsync failed");
                continue;
            }
            const int64_t left = info[i].n_rows - info[i].first_row;
            info[i].valid_rows = left < 0 ? 0 : std::min(left, T);
        }
        if (hipStreamSynchronize(c->stream) != hipSuccess && !hip_rc) hip_rc = fail(MP3S_E_HIP, "sync failed");
        if (hip_rc) { mp3_list_done(c, m); return hip_rc; }
    }
    mp3_list_done(c, m);
    const int first_bad = finish_files(fs, status);
    return status ? MP3S_OK : first_bad;
}

}  // namespace

extern "C" {

int mp3s_pcm_batch_dev(mp3s_ctx *c, const int16_t *d_pcm, int nch, const mp3s_pcm_batch_item *d_items, const mp3s_pcm_batch_item *h_items,
                       int n_items, int out_channels, int out_format, int64_t T, void *d_out)
{
    if (!c || !d_pcm || !d_items || !h_items || !d_out) return fail(MP3S_E_ARG, "null pointer");
    if (n_items <= 0) return fail(MP3S_E_ARG, "n_items=%d", n_items);
    if (nch != 1 && nch != 2) return fail(MP3S_E_ARG, "nch=%d", nch);
    if (const int rc = batch_shape_check(out_channels, "out_channels", out_format, T)) return rc;
    if ((uintptr_t)d_pcm % (size_t)(2 * nch)) return fail(MP3S_E_ARG, "d_pcm is not aligned to a row");
    if ((uintptr_t)d_out % batch_elem(out_format)) return fail(MP3S_E_ARG, "d_out is not aligned to an element");
    if (!pcm_batch_items_ok(h_items, n_items)) return fail(MP3S_E_ARG, "an item with a negative field");
    std::vector<PcmBatchTile> tiles;
    if (!pcm_batch_tiles(n_items, T, tiles)) return fail(MP3S_E_ARG, "too many rows for one launch");
    HIPCHK(hipSetDevice(c->device));
    const uint8_t *d_tiles = nullptr;
    if (const int rc = batch_block_up(c, nullptr, 0, tiles, &d_tiles)) return rc;
    const int e = launch_pcm_batch(c->stream, d_pcm, nch, d_items, (const PcmBatchTile *)d_tiles, (int)tiles.size(), out_channels, out_format, T, d_out);
    if (e) return fail(MP3S_E_HIP, "pcm batch launch: %s", hipGetErrorString((hipError_t)e));
    return MP3S_OK;
}

int mp3s_pcm_unbatch_dev(mp3s_ctx *c, const void *d_in, int in_channels, int in_format, int64_t T, const mp3s_pcm_unbatch_item *d_items,
                         const mp3s_pcm_unbatch_item *h_items, int n_items, int16_t *d_pcm)
{
    if (!c || !d_in || !d_items || !h_items || !d_pcm) return fail(MP3S_E_ARG, "null pointer");
    if (n_items <= 0) return fail(MP3S_E_ARG, "n_items=%d", n_items);
    if (const int rc = batch_shape_check(in_channels, "in_channels", in_format, T)) return rc;
    if ((uintptr_t)d_in % batch_elem(in_format)) return fail(MP3S_E_ARG, "d_in is not aligned to an element");
    if ((uintptr_t)d_pcm & 15) return fail(MP3S_E_ARG, "d_pcm is not 16-byte aligned");
    if (!pcm_unbatch_items_ok(h_items, n_items, T)) return fail(MP3S_E_ARG, "an item with a negative field or with n_rows outside [1, T]");
    std::vector<PcmBatchTile> tiles;
    if (!pcm_unbatch_tiles(h_items, n_items, tiles)) return fail(MP3S_E_ARG, "too many rows for one launch");
    HIPCHK(hipSetDevice(c->device));
    const uint8_t *d_tiles = nullptr;
    if (const int rc = batch_block_up(c, nullptr, 0, tiles, &d_tiles)) return rc;
    const int e = launch_pcm_unbatch(c->stream, d_in, in_channels, in_format, T, d_items, (const PcmBatchTile *)d_tiles, (int)tiles.size(), d_pcm);
    if (e) return fail(MP3S_E_HIP, "pcm unbatch launch: %s", hipGetErrorString((hipError_t)e));
    return MP3S_OK;
}

int mp3s_pcm_batch_decode_files(mp3s_ctx *c, const uint8_t *const *mp3s, const size_t *lens, int n_files, const int64_t *first_rows, int64_t T,
                                int out_channels, int out_format, void *d_out, size_t out_bytes, mp3s_pcm_batch_info *info, int32_t *status)
{
    return decode_files(c, mp3s, lens, n_files, 0, first_rows, T, out_channels, out_format, d_out, out_bytes, info, status);
}

int mp3s_pcm_batch_decode_files_at(mp3s_ctx *c, const uint8_t *const *mp3s, const size_t *lens, int n_files, int out_rate, const int64_t *first_rows,
                                   int64_t T, int out_channels, int out_format, void *d_out, size_t out_bytes, mp3s_pcm_batch_info_at *info, int32_t *status)
{
    return decode_files(c, mp3s, lens, n_files, out_rate, first_rows, T, out_channels, out_format, d_out, out_bytes, info, status);
}

int mp3s_pcm_resample_plan(int in_rate, int out_rate, mp3s_pcm_resample_ratio *out)
{
    if (!out) return fail(MP3S_E_ARG, "null pointer");
    if (in_rate <= 0 || out_rate <= 0) return fail(MP3S_E_ARG, "in_rate=%d, out_rate=%d", in_rate, out_rate);
    int L, M, T, H;
    if (pcm_resample_plan(in_rate, out_rate, &L, &M, &T, &H)) return fail(MP3S_E_UNSUPPORTED, "%d -> %d Hz is a ratio the resampler refuses", in_rate, out_rate);
    *out = mp3s_pcm_resample_ratio{L, M, T, H};
    return MP3S_OK;
}

int mp3s_pcm_batch_resample_dev(mp3s_ctx *c, const int16_t *d_pcm, int nch, const mp3s_pcm_resample_item *h_items, int n_items, int out_channels,
                                int out_format, int64_t T, void *d_out)
{
    if (!c || !d_pcm || !h_items || !d_out) return fail(MP3S_E_ARG, "null pointer");
    if (n_items <= 0) return fail(MP3S_E_ARG, "n_items=%d", n_items);
    if (nch != 1 && nch != 2) return fail(MP3S_E_ARG, "nch=%d", nch);
    if (const int rc = batch_shape_check(out_channels, "out_channels", out_format, T)) return rc;
    if ((uintptr_t)d_pcm % (size_t)(2 * nch)) return fail(MP3S_E_ARG, "d_pcm is not aligned to a row");
    if ((uintptr_t)d_out % batch_elem(out_format)) return fail(MP3S_E_ARG, "d_out is not aligned to an element");
    constexpr int64_t kMost = (int64_t)1 << 40;
    std::vector<PcmRatio> ratios((size_t)n_items);
    for (int i = 0; i < n_items; i++) {
        const mp3s_pcm_resample_item &it = h_items[i];
        if (it.src_row < 0 || it.n_rows < 0 || it.first_row < 0 || it.slot < 0 || it.src_row > kMost || it.n_rows > kMost || it.first_row > kMost)
            return fail(MP3S_E_ARG, "item %d: a negative field, or one above 2^40", i);
        if (it.L <= 0 || it.M <= 0) return fail(MP3S_E_ARG, "item %d: L=%d, M=%d", i, it.L, it.M);
        PcmRatio &q = ratios[(size_t)i];
        int H = 0;
        if (pcm_resample_plan(it.M, it.L, &q.L, &q.M, &q.T, &H)) return fail(MP3S_E_UNSUPPORTED, "item %d: %d / %d is a ratio the resampler refuses", i, it.L, it.M);
        if (q.L != it.L || q.M != it.M) return fail(MP3S_E_UNSUPPORTED, "item %d: %d / %d is not in lowest terms", i, it.L, it.M);
    }
    std::vector<PcmBatchTile> tiles;
    if (!pcm_resample_tiles(n_items, T, tiles)) return fail(MP3S_E_ARG, "too many rows for one launch");
    HIPCHK(hipSetDevice(c->device));
    std::vector<PcmResampleRun> runs((size_t)n_items);
    for (int i = 0; i < n_items; i++)
        if (const int rc = resample_run(c, h_items[i].src_row, h_items[i].n_rows, h_items[i].first_row, h_items[i].slot, ratios[(size_t)i], nch, &runs[(size_t)i])) return rc;
    return resample_launch(c, d_pcm, nch, runs, tiles, out_channels, out_format, T, d_out);
}

int mp3s_pcm_batch_encode(mp3s_ctx *c, const void *d_in, int n_items, int in_channels, int in_format, int64_t T, const int64_t *n_rows,
                          int samplerate, int bitrate_kbps, const uint8_t *const *hide_bits, const int32_t *n_hide, mp3s_buf **owner, mp3s_file *out,
                          int32_t *status)
{
    if (!c || !d_in || !n_rows || !owner || !out || (hide_bits && !n_hide)) return fail(MP3S_E_ARG, "null pointer");
    if (n_items <= 0) return fail(MP3S_E_ARG, "n_items=%d", n_items);
    if (const int rc = batch_shape_check(in_channels, "in_channels", in_format, T)) return rc;
    if ((uintptr_t)d_in % batch_elem(in_format)) return fail(MP3S_E_ARG, "d_in is not aligned to an element");
    int sri, bri, whole;
    if (bitrate_kbps <= 0) return fail(MP3S_E_UNSUPPORTED, "bitrate %d", bitrate_kbps);
    if (stream_params(samplerate, bitrate_kbps, &sri, &bri, &whole)) return fail(MP3S_E_UNSUPPORTED, "unsupported samplerate/bitrate %d/%d", samplerate, bitrate_kbps);
    return encode_list(c, d_in, n_items, in_channels, in_format, T, n_rows, samplerate, bitrate_kbps, hide_bits, n_hide, owner, out, status, nullptr);
}

int mp3s_pcm_batch_encode_at(mp3s_ctx *c, const void *d_in, int n_items, int in_channels, int in_format, int64_t T, const int64_t *n_rows, int in_rate,
                             int mode, int bitrate_kbps, const uint8_t *const *hide_bits, const int32_t *n_hide, mp3s_buf **owner, mp3s_file *out,
                             int32_t *status)
{
    if (!c || !d_in || !n_rows || !owner || !out || (hide_bits && !n_hide)) return fail(MP3S_E_ARG, "null pointer");
    if (n_items <= 0) return fail(MP3S_E_ARG, "n_items=%d", n_items);
    if (const int rc = batch_shape_check(in_channels, "in_channels", in_format, T)) return rc;
    if ((uintptr_t)d_in % batch_elem(in_format)) return fail(MP3S_E_ARG, "d_in is not aligned to an element");
    if (mode != 1 && mode != 32000 && mode != 44100 && mode != 48000) return fail(MP3S_E_ARG, "mode=%d", mode);
    if (in_rate <= 0) return fail(MP3S_E_ARG, "in_rate=%d", in_rate);
    int target = 0, H = 0;
    PcmRatio q;
    if (wav_resample_plan(in_rate, mode, &target, &q.L, &q.M, &q.T, &H)) return fail(MP3S_E_EXIT, "Unsupported sampling frequency.");
    if (q.L == 1 && q.M == 1)
        return mp3s_pcm_batch_encode(c, d_in, n_items, in_channels, in_format, T, n_rows, target, bitrate_kbps, hide_bits, n_hide, owner, out, status);
    int sri, bri, whole;
    if (bitrate_kbps <= 0) return fail(MP3S_E_UNSUPPORTED, "bitrate %d", bitrate_kbps);
    if (stream_params(target, bitrate_kbps, &sri, &bri, &whole)) return fail(MP3S_E_UNSUPPORTED, "unsupported samplerate/bitrate %d/%d", target, bitrate_kbps);
    if (pcm_resample_plan(in_rate, target, &q.L, &q.M, &q.T, &H)) return fail(MP3S_E_EXIT, "Unsupported sampling frequency.");   // (no table: before any item is looked at)
    return encode_list(c, d_in, n_items, in_channels, in_format, T, n_rows, target, bitrate_kbps, hide_bits, n_hide, owner, out, status, &q);
}

}  // extern "C"
