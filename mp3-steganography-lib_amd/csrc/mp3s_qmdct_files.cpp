// C-ABI of the library (include/mp3s.h), part 3g: QMDCT on the device -- the Markov / histogram features of a list of MP3 files and
// their quantised spectra as a batch in the caller's device memory, on the frame of the list-of-files calls (mp3s_internal.h).  The
// files go the way of the table audit: decode_front (upload, Huffman decode, the host's repair, no transform), then k_qmdct_features
// or k_qmdct_batch (k_qmdct.hpp) on the samples where they lie.  2904 bytes per file come down for the features, nothing for a batch.
#include "mp3s_internal.h"

namespace {

// The host-made block of a launch, [head (head_bytes, may be 0) | tiles], to kPoolInputs on the context's stream, from the context's
// h_pcm_batch by the rule of pcm_dev_host_block.  *d_block: where it lies, the tiles at up16(head_bytes).
int block_up(mp3s_ctx *c, const void *head, size_t head_bytes, const void *tiles, size_t tile_bytes, const uint8_t **d_block)
{
    const size_t o_tiles = up16(head_bytes), bytes = o_tiles + tile_bytes;
    return pcm_dev_host_block(c, [&]() {
        std::vector<uint8_t> &h = c->h_pcm_batch;
        h.assign(bytes, 0);
        if (head_bytes) std::memcpy(h.data(), head, head_bytes);
        if (tile_bytes) std::memcpy(h.data() + o_tiles, tiles, tile_bytes);
        void *d = c->grab(kPoolInputs, bytes);
        if (!d) return fail(MP3S_E_NOMEM, "hipMalloc failed for %zu bytes of workgroup entries", bytes);
        if (bytes) HIPCHK(hipMemcpyAsync(d, h.data(), bytes, hipMemcpyHostToDevice, c->stream));
        *d_block = (const uint8_t *)d;
        return (int)MP3S_OK;
    });
}

void no_frames(const ParsedStream &p, int n_lines, mp3s_qmdct_features *out)
{
    std::memset(out, 0, sizeof *out);
    out->channels = p.nch; out->sampling_rate = p.sampling_rate; out->kbps = p.bit_rate / 1000; out->n_lines = n_lines;
}

// decode_front of the streams `idx`, held to the frame counts the scan found (a stream the host parser took over as a whole may count
// other frames than the layout stands on)
int front_of(mp3s_ctx *c, mp3s_multi &m, const std::vector<int> &idx, int nch, DecodeFront &F)
{
    std::vector<int> frames(idx.size());
    for (size_t k = 0; k < idx.size(); k++) frames[k] = m.parsed[idx[k]].n_frames;
    const int rc = decode_front(c, m, idx, nch, 0, F);
    if (rc) return rc;
    if (F.n <= 0) return fail(MP3S_E_ARG, "a batch without frames");
    for (size_t k = 0; k < idx.size(); k++)
        if (m.parsed[idx[k]].n_frames != frames[k]) return fail(MP3S_E_MALFORMED, "file %d: the decode found other frame counts than the scan", idx[k]);
    return MP3S_OK;
}

// The streams `idx` of m (one channel count, every one with a frame) as one batch; out[idx[k]] = stream k.
int features_group(mp3s_ctx *c, mp3s_multi &m, const std::vector<int> &idx, int nch, int n_lines, mp3s_qmdct_features *out)
{
    DecodeFront F;
    int rc = front_of(c, m, idx, nch, F);
    if (rc) return rc;
    const size_t ns = idx.size();
    std::vector<mp3s_table_audit_seg> segs(ns);
    for (size_t k = 0; k < ns; k++) segs[k] = {(int32_t)F.first_of[k], (int32_t)m.parsed[idx[k]].n_frames};
    std::vector<QmdctTile> tiles;
    if (!qmdct_feature_tiles(segs.data(), (int)ns, tiles)) return fail(MP3S_E_ARG, "too many granules for one launch");
    const size_t res_bytes = ns * sizeof(mp3s_qmdct_features);
    void *d_res = c->grab(kPoolSmall, res_bytes);
    if (!d_res) return fail(MP3S_E_NOMEM, "hipMalloc failed for the features of %zu stream(s)", ns);
    const uint8_t *d_block = nullptr;
    rc = block_up(c, segs.data(), ns * sizeof segs[0], tiles.data(), tiles.size() * sizeof(QmdctTile), &d_block);
    if (rc) return rc;
    const int e = launch_qmdct_features(c->stream, (const int16_t *)F.d_is, nch, (const mp3s_table_audit_seg *)d_block, (int)ns,
                                        (const QmdctTile *)(d_block + up16(ns * sizeof segs[0])), (int)tiles.size(), n_lines, (mp3s_qmdct_features *)d_res);
    if (e) return fail(MP3S_E_HIP, "qmdct features launch: %s", hipGetErrorString((hipError_t)e));
    std::vector<mp3s_qmdct_features> rec(ns);
    rc = mp3s_dev_download(c, rec.data(), d_res, res_bytes);
    if (rc) return rc;
    if (trace_on()) fprintf(stderr, "mp3s:   qmdct features: %zu stream(s), %ld frames, %zu workgroup(s) x %d channel(s), %zu bytes down\n", ns, F.n, tiles.size(), nch, res_bytes);
    for (size_t k = 0; k < ns; k++) {
        const ParsedStream &p = m.parsed[idx[k]];
        mp3s_qmdct_features &o = out[idx[k]];
        o = rec[k];
        o.sampling_rate = p.sampling_rate; o.kbps = p.bit_rate / 1000;
    }
    return MP3S_OK;
}

// The streams `idx` of m (one channel count, every one with a frame) through the front half of the decode, then one k_qmdct_batch
// launch into the caller's d_out: file i's rows from first_granule(i) on into slot i.  The stream is synchronised whatever happened.
int batch_group(mp3s_ctx *c, mp3s_multi &m, const std::vector<int> &idx, int nch, const int64_t *first_granules, int64_t Gt, int out_channels, int16_t *d_out)
{
    DecodeFront F;
    int rc = front_of(c, m, idx, nch, F);
    std::vector<mp3s_qmdct_batch_item> items(idx.size());
    std::vector<PcmBatchTile> tiles;
    if (!rc) {
        for (size_t k = 0; k < idx.size(); k++)
            items[k] = {(int64_t)F.first_of[k], (int64_t)m.parsed[idx[k]].n_frames, first_granules ? first_granules[idx[k]] : 0, idx[k], 0};
        if (!qmdct_batch_tiles((int)idx.size(), out_channels, Gt, tiles)) rc = fail(MP3S_E_ARG, "too many rows for one launch");
    }
    const uint8_t *d_block = nullptr;
    if (!rc) rc = block_up(c, items.data(), items.size() * sizeof items[0], tiles.data(), tiles.size() * sizeof(PcmBatchTile), &d_block);
    if (!rc) {
        const int e = launch_qmdct_batch(c->stream, (const int16_t *)F.d_is, nch, (const mp3s_qmdct_batch_item *)d_block,
                                         (const PcmBatchTile *)(d_block + up16(items.size() * sizeof items[0])), (int)tiles.size(), out_channels, Gt, d_out);
        if (e) rc = fail(MP3S_E_HIP, "qmdct batch launch: %s", hipGetErrorString((hipError_t)e));
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) rc = fail(MP3S_E_HIP, "sync failed");
    if (trace_on()) fprintf(stderr, "mp3s:   qmdct batch: %zu stream(s) of %d channel(s), %ld frames, %zu workgroup(s)\n", idx.size(), nch, F.n, tiles.size());
    return rc;
}

}  // namespace

extern "C" {

int mp3s_qmdct_features_dev(mp3s_ctx *c, const int16_t *d_is, int n_frames, int nch, const mp3s_table_audit_seg *d_segs,
                            const mp3s_table_audit_seg *h_segs, int n_segs, int n_lines, mp3s_qmdct_features *d_out)
{
    if (!c || !d_is || !d_segs || !h_segs || !d_out) return fail(MP3S_E_ARG, "null pointer");
    if (n_frames <= 0 || n_segs <= 0) return fail(MP3S_E_ARG, "n_frames=%d, n_segs=%d", n_frames, n_segs);
    if (nch != 1 && nch != 2) return fail(MP3S_E_ARG, "nch=%d", nch);
    if (n_lines < 1 || n_lines > 576) return fail(MP3S_E_ARG, "n_lines=%d", n_lines);
    if (((uintptr_t)d_is & 3) || ((uintptr_t)d_out & 7)) return fail(MP3S_E_ARG, "d_is must be 4-byte, d_out 8-byte aligned");
    for (int s = 0; s < n_segs; s++)
        if (h_segs[s].first_frame < 0 || h_segs[s].n_frames < 0 || (int64_t)h_segs[s].first_frame + h_segs[s].n_frames > n_frames)
            return fail(MP3S_E_ARG, "segment %d reaches outside the batch", s);
    std::vector<QmdctTile> tiles;
    if (!qmdct_feature_tiles(h_segs, n_segs, tiles)) return fail(MP3S_E_ARG, "too many granules for one launch");
    HIPCHK(hipSetDevice(c->device));
    const uint8_t *d_tiles = nullptr;
    if (const int rc = block_up(c, nullptr, 0, tiles.data(), tiles.size() * sizeof(QmdctTile), &d_tiles)) return rc;
    const int e = launch_qmdct_features(c->stream, d_is, nch, d_segs, n_segs, (const QmdctTile *)d_tiles, (int)tiles.size(), n_lines, d_out);
    if (e) return fail(MP3S_E_HIP, "qmdct features launch: %s", hipGetErrorString((hipError_t)e));
    return MP3S_OK;
}

int mp3s_qmdct_features_files(mp3s_ctx *c, const uint8_t *const *mp3s, const size_t *lens, int n_files, int n_lines, mp3s_qmdct_features *out,
                              int32_t *status)
{
    if (!c || !mp3s || !lens || !out || n_files <= 0) return fail(MP3S_E_ARG, "bad argument");
    if (n_lines < 1 || n_lines > 576) return fail(MP3S_E_ARG, "n_lines=%d", n_lines);
    std::unique_ptr<mp3s_multi> mm(new mp3s_multi());
    mp3s_multi &m = *mm;
    FileStatus fs(n_files);
    FileGroups groups;                       // by channel count
    for (int i = 0; i < n_files; i++) std::memset(&out[i], 0, sizeof out[i]);
    const std::vector<int32_t> front = mp3_list_front(c, m, n_files, [&](int i) { return std::pair<const uint8_t *, size_t>(mp3s[i], lens[i]); });
    for (int i = 0; i < n_files; i++) {
        if (front[(size_t)i]) { fs.set(i, front_end_failed(front[(size_t)i], i)); continue; }
        const ParsedStream &p = m.parsed[i];
        if (p.n_frames <= 0) { no_frames(p, n_lines, &out[i]); continue; }
        if (p.nch < 1 || p.nch > 2) { fs.set(i, fail(MP3S_E_MALFORMED, "file %d: channel count %d", i, p.nch)); continue; }
        groups.add(p.nch, 0, i);
    }
    run_groups(groups, [&](int nch, int, const std::vector<int> &idx) {
        const int rc = features_group(c, m, idx, nch, n_lines, out);
        if (rc) for (int i : idx) std::memset(&out[i], 0, sizeof out[i]);
        return rc;
    }, fs, [&] { (void)hipStreamSynchronize(c->stream); });   // (the block of the failed batch may still be on its way)
    mp3_list_done(c, m);
    const int first_bad = finish_files(fs, status);
    return status ? MP3S_OK : first_bad;
}

int mp3s_qmdct_batch_dev(mp3s_ctx *c, const int16_t *d_is, int nch, const mp3s_qmdct_batch_item *d_items, const mp3s_qmdct_batch_item *h_items,
                         int n_items, int out_channels, int64_t Gt, int16_t *d_out)
{
    if (!c || !d_is || !d_items || !h_items || !d_out) return fail(MP3S_E_ARG, "null pointer");
    if (n_items <= 0) return fail(MP3S_E_ARG, "n_items=%d", n_items);
    if (nch != 1 && nch != 2) return fail(MP3S_E_ARG, "nch=%d", nch);
    if (out_channels != 1 && out_channels != 2) return fail(MP3S_E_ARG, "out_channels=%d", out_channels);
    if (nch == 2 && out_channels == 1) return fail(MP3S_E_ARG, "a stereo stream has no one-channel spectrum");
    if (Gt <= 0 || Gt > kQmdctMaxRows) return fail(MP3S_E_ARG, "Gt=%lld", (long long)Gt);
    if (((uintptr_t)d_is & 15) || ((uintptr_t)d_out & 15)) return fail(MP3S_E_ARG, "d_is and d_out must be 16-byte aligned");
    if (!qmdct_batch_items_ok(h_items, n_items)) return fail(MP3S_E_ARG, "an item with a negative field");
    for (int i = 0; i < n_items; i++)
        if ((uint64_t)h_items[i].slot >= ((uint64_t)1 << 62) / ((uint64_t)out_channels * (uint64_t)Gt * 1152)) return fail(MP3S_E_ARG, "item %d: slot %d lies outside any address", i, h_items[i].slot);
    std::vector<PcmBatchTile> tiles;
    if (!qmdct_batch_tiles(n_items, out_channels, Gt, tiles)) return fail(MP3S_E_ARG, "too many rows for one launch");
    HIPCHK(hipSetDevice(c->device));
    const uint8_t *d_tiles = nullptr;
    if (const int rc = block_up(c, nullptr, 0, tiles.data(), tiles.size() * sizeof(PcmBatchTile), &d_tiles)) return rc;
    const int e = launch_qmdct_batch(c->stream, d_is, nch, d_items, (const PcmBatchTile *)d_tiles, (int)tiles.size(), out_channels, Gt, d_out);
    if (e) return fail(MP3S_E_HIP, "qmdct batch launch: %s", hipGetErrorString((hipError_t)e));
    return MP3S_OK;
}

int mp3s_qmdct_batch_decode_files(mp3s_ctx *c, const uint8_t *const *mp3s, const size_t *lens, int n_files, const int64_t *first_granules, int64_t Gt,
                                  int out_channels, int16_t *d_out, size_t out_bytes, mp3s_qmdct_batch_info *info, int32_t *status)
{
    if (!c || !mp3s || !lens || !info) return fail(MP3S_E_ARG, "null pointer");
    if (n_files <= 0) return fail(MP3S_E_ARG, "n_files=%d", n_files);
    if (out_channels != 1 && out_channels != 2) return fail(MP3S_E_ARG, "out_channels=%d", out_channels);
    size_t slot_bytes = 0;
    if (d_out) {
        if (Gt <= 0 || Gt > kQmdctMaxRows) return fail(MP3S_E_ARG, "Gt=%lld", (long long)Gt);
        if ((uintptr_t)d_out & 15) return fail(MP3S_E_ARG, "d_out is not 16-byte aligned");
        slot_bytes = (size_t)Gt * (size_t)out_channels * 1152;
        if (slot_bytes > SIZE_MAX / (size_t)n_files) return fail(MP3S_E_ARG, "Gt=%lld is too large", (long long)Gt);
        if (out_bytes < slot_bytes * (size_t)n_files) return fail(MP3S_E_ARG, "out_bytes=%zu, the batch takes %zu", out_bytes, slot_bytes * (size_t)n_files);
        for (int i = 0; first_granules && i < n_files; i++)
            if (first_granules[i] < 0 || first_granules[i] > ((int64_t)1 << 40)) return fail(MP3S_E_ARG, "first_granules[%d]=%lld", i, (long long)first_granules[i]);
    }
    std::unique_ptr<mp3s_multi> mm(new mp3s_multi());
    mp3s_multi &m = *mm;
    FileStatus fs(n_files);
    FileGroups groups;                                    // by channel count
    std::memset(info, 0, (size_t)n_files * sizeof *info);
    // (with status == NULL a file the front end refuses fails the call here, before any device work -- a null file before any work at all)
    for (int i = 0; i < n_files && !status; i++)
        if (!mp3s[i]) return fail(MP3S_E_ARG, "file %d is null", i);
    const std::vector<int32_t> frc = mp3_list_front(c, m, n_files, [&](int i) { return std::pair<const uint8_t *, size_t>(mp3s[i], lens[i]); });
    for (int i = 0; i < n_files; i++) {
        int rc = MP3S_OK;
        if (frc[(size_t)i]) rc = mp3s[i] ? fail(frc[(size_t)i], "file %d: malformed or unsupported MP3 stream", i) : fail(MP3S_E_ARG, "file %d is null", i);
        else if (m.parsed[i].n_frames > 0 && m.parsed[i].nch == 2 && out_channels == 1)
            rc = fail(MP3S_E_ARG, "file %d: a stereo stream has no one-channel spectrum", i);
        if (rc) {
            fs.set(i, rc);
            if (!status) { mp3_list_done(c, m); return rc; }
            m.parsed[i] = ParsedStream();                 // nothing of it goes into a batch
            continue;
        }
        const ParsedStream &p = m.parsed[i];
        info[i].n_frames = p.n_frames; info[i].nch = p.nch; info[i].sampling_rate = p.sampling_rate; info[i].bit_rate = p.bit_rate;
        info[i].n_granules = 2 * (int64_t)p.n_frames; info[i].first_granule = first_granules ? first_granules[i] : 0;
        if (d_out && p.n_frames > 0) groups.add(p.nch, 0, i);
    }
    if (d_out) {
        if (hipSetDevice(c->device) != hipSuccess) { mp3_list_done(c, m); return fail(MP3S_E_HIP, "hipSetDevice failed"); }
        run_groups(groups, [&](int nch, int, const std::vector<int> &idx) {
            return nch < 1 || nch > 2 ? fail(MP3S_E_MALFORMED, "channel count %d", nch) : batch_group(c, m, idx, nch, first_granules, Gt, out_channels, d_out);
        }, fs, [] {});
        // what no batch has written: the slots of failed and of frameless files
        int hip_rc = MP3S_OK;
        for (int i = 0; i < n_files; i++) {
            if (fs.st[(size_t)i]) std::memset(&info[i], 0, sizeof info[i]);
            if (fs.st[(size_t)i] || info[i].n_frames <= 0) {
                if (hipMemsetAsync((uint8_t *)d_out + (size_t)i * slot_bytes, 0, slot_bytes, c->stream) != hipSuccess && !hip_rc) hip_rc = fail(MP3S_E_HIP, "hipMemsetAsync failed");
                continue;
            }
            const int64_t left = info[i].n_granules - info[i].first_granule;
            info[i].valid_granules = left < 0 ? 0 : std::min(left, Gt);
        }
        if (hipStreamSynchronize(c->stream) != hipSuccess && !hip_rc) hip_rc = fail(MP3S_E_HIP, "sync failed");
        if (hip_rc) { mp3_list_done(c, m); return hip_rc; }
    }
    mp3_list_done(c, m);
    const int first_bad = finish_files(fs, status);
    return status ? MP3S_OK : first_bad;
}

}  // extern "C"
