// C-ABI of the library (include/mp3s.h), part 3f: a cover file against its stego file -- the lag that aligns the PCM of two MP3 files
// and their exact difference at it, on the frame of the pair-list calls (pcm_pairs.cpp).  With the int16 PCM of a group's A and B streams in HBM, k_pcm_lag_scores, k_pcm_lag_pick and k_pcm_diff_lagged
// (k_pcmalign.hpp) and k_pcm_diff_pairs run behind the decode; 80 bytes per pair come down, and with the profile 32 per chunk of 1152
// rows and 8 per score; no PCM does.
#include "mp3s_internal.h"

namespace {

// W of a pair of rows_a / rows_b rows: the rows a search over +-max_lag can place its window in (< 1: none)
inline int64_t search_room(int64_t rows_a, int64_t rows_b, int max_lag) { return std::min(rows_a, rows_b) - 2 * (int64_t)max_lag; }

int check_search(int n_pairs, int nch, int max_lag, int search_rows, const int32_t *lags)
{
    if (n_pairs <= 0) return fail(MP3S_E_ARG, "n_pairs=%d", n_pairs);
    if (nch != 1 && nch != 2) return fail(MP3S_E_ARG, "nch=%d", nch);
    if (max_lag < 0 || max_lag > kPcmMaxLag) return fail(MP3S_E_ARG, "max_lag=%d is outside 0 .. %d", max_lag, kPcmMaxLag);
    if (search_rows < 1) return fail(MP3S_E_ARG, "search_rows=%d", search_rows);
    for (int p = 0; lags && p < n_pairs; p++)
        if (lags[p] < -kPcmMaxLag || lags[p] > kPcmMaxLag) return fail(MP3S_E_ARG, "pair %d: a lag of %d is outside +-%d", p, (int)lags[p], kPcmMaxLag);
    return MP3S_OK;
}

// the host-made inputs of the passes as one block: [runs (with_runs) | tiles | given lags (lags != NULL)], every part 16-byte aligned
struct AlignIn { size_t o_tiles = 0, o_lags = 0, bytes = 0; int n_tiles = 0; };
int align_inputs(const mp3s_pcm_run_pair *runs, int n_pairs, bool with_runs, const int32_t *lags, std::vector<uint8_t> &in, AlignIn *L)
{
    std::vector<mp3s_pcm_pair> bound;
    std::vector<PcmTile> tiles;
    pcm_align_bound_pairs(runs, n_pairs, bound);
    if (!pcm_diff_tiles(bound.data(), n_pairs, tiles)) return fail(MP3S_E_ARG, "too many rows to compare");
    L->n_tiles = (int)tiles.size();
    L->o_tiles = with_runs ? up16((size_t)n_pairs * sizeof(mp3s_pcm_run_pair)) : 0;
    L->o_lags = L->o_tiles + up16(tiles.size() * sizeof(PcmTile));
    L->bytes = L->o_lags + (lags ? (size_t)n_pairs * sizeof(int32_t) : 0);
    in.assign(std::max<size_t>(L->bytes, 16), 0);
    if (with_runs) std::memcpy(in.data(), runs, (size_t)n_pairs * sizeof(mp3s_pcm_run_pair));
    if (!tiles.empty()) std::memcpy(in.data() + L->o_tiles, tiles.data(), tiles.size() * sizeof(PcmTile));
    if (lags) std::memcpy(in.data() + L->o_lags, lags, (size_t)n_pairs * sizeof(int32_t));
    return MP3S_OK;
}

// The pairs `idx` as one batch (PcmPairBatch): the passes behind the decode, the pair and lag records down and with the profile the
// chunk records and the scores, which the results then point into.
int align_group(mp3s_ctx *c, mp3s_multi &m, int n_pairs, const std::vector<int> &idx, int nch, int max_lag, int search_rows, const int32_t *lags,
                bool want_profile, mp3s_buf *top, mp3s_pcm_alignment *out)
{
    const size_t n = idx.size(), n_lags = (size_t)2 * (size_t)max_lag + 1;
    PcmPairBatch b;
    if (const int rc = b.lay(m, n_pairs, idx, 0x7fffffff / 1152 / 8)) return rc;
    std::vector<mp3s_pcm_run_pair> runs(n);
    std::vector<int32_t> given(lags ? n : 0);
    for (size_t k = 0; k < n; k++) {
        runs[k] = {(uint32_t)(b.first[k] * 1152), (uint32_t)(b.frames_a[k] * 1152), (uint32_t)((b.first[k] + b.frames_a[k]) * 1152), (uint32_t)(b.frames_b[k] * 1152),
                   (uint32_t)b.out_first[k], 0};   // (chunk records in whole frames: the bound of a pair is its smaller frame count)
        if (lags) given[k] = lags[idx[k]];
    }
    const int64_t chunks = b.cmp_frames;
    AlignIn L;
    std::vector<uint8_t> &in = c->h_in;
    if (const int rc = align_inputs(runs.data(), (int)n, true, lags ? given.data() : nullptr, in, &L)) return rc;
    // the results as one block [pair records | lag records | chunk records | scores | geometry]: the first two come down, the next two with the profile
    const size_t o_lag = up16(n * sizeof(mp3s_pcm_pair_diff)), o_frames = o_lag + up16(n * sizeof(mp3s_pcm_lag)),
                 o_scores = o_frames + up16((size_t)chunks * sizeof(mp3s_pcm_frame_diff)), o_geo = o_scores + (lags ? 0 : up16(n * n_lags * sizeof(uint64_t))),
                 res_bytes = o_geo + n * sizeof(mp3s_pcm_pair), down_bytes = want_profile ? o_geo : o_frames;
    const int rc = b.run(c, m, nch, in.data(), L.bytes, res_bytes, down_bytes, [&](const int16_t *d_pcm, const uint8_t *d_in, uint8_t *d_res) {
        const int e = launch_pcm_align(c->stream, d_pcm, nch, (const mp3s_pcm_run_pair *)d_in, (int)n, max_lag, search_rows,
                                       lags ? (const int32_t *)(d_in + L.o_lags) : nullptr, (const PcmTile *)(d_in + L.o_tiles), L.n_tiles,
                                       lags ? nullptr : (uint64_t *)(d_res + o_scores), (mp3s_pcm_lag *)(d_res + o_lag), (mp3s_pcm_pair *)(d_res + o_geo),
                                       (mp3s_pcm_frame_diff *)(d_res + o_frames), (mp3s_pcm_pair_diff *)d_res);
        return e ? fail(MP3S_E_HIP, "pcm align launch: %s", hipGetErrorString((hipError_t)e)) : MP3S_OK;
    });
    if (rc) return rc;
    if (trace_on())
        fprintf(stderr, "mp3s:   pcm alignment: %zu pair(s) of %d channel(s), %lld frames decoded, %zu lag(s) %s, %lld chunk record(s), %zu bytes down\n", n, nch,
                (long long)b.rows_frames, n_lags, lags ? "given" : "searched", (long long)chunks, down_bytes);
    const uint8_t *const res = b.res;
    const mp3s_pcm_pair_diff *rec = (const mp3s_pcm_pair_diff *)res;
    const mp3s_pcm_lag *lag = (const mp3s_pcm_lag *)(res + o_lag);
    for (size_t k = 0; k < n; k++) {
        mp3s_pcm_alignment &o = out[idx[k]];
        const mp3s_pcm_frame_diff *profile = want_profile ? (const mp3s_pcm_frame_diff *)(res + o_frames) + runs[k].out_first : nullptr;
        distortion_from_record(rec[k], m.parsed[idx[k]], m.parsed[n_pairs + idx[k]], lag[k].n_chunks, (int64_t)lag[k].n_rows * nch, profile, &o.at_lag);
        o.lag = lag[k];
        o.scores = want_profile && !lags && lag[k].n_best ? (const uint64_t *)(res + o_scores) + k * n_lags : nullptr;
    }
    top->parts.push_back(std::move(b.part));
    return MP3S_OK;
}

}  // namespace

extern "C" {

int mp3s_pcm_align_dev(mp3s_ctx *c, const int16_t *d_pcm, int nch, const mp3s_pcm_run_pair *d_runs, const mp3s_pcm_run_pair *h_runs, int n_pairs,
                       int max_lag, int search_rows, const int32_t *h_lags, uint64_t *d_scores, mp3s_pcm_lag *d_lags, mp3s_pcm_frame_diff *d_frames,
                       mp3s_pcm_pair_diff *d_out)
{
    if (!c || !d_pcm || !d_runs || !h_runs || !d_lags || !d_frames || !d_out || (!h_lags && !d_scores)) return fail(MP3S_E_ARG, "null pointer");
    if (const int rc = check_search(n_pairs, nch, max_lag, search_rows, h_lags)) return rc;
    if ((uintptr_t)d_pcm & 15) return fail(MP3S_E_ARG, "d_pcm is not 16-byte aligned");
    HIPCHK(hipSetDevice(c->device));
    AlignIn L;
    size_t o_geo = 0;
    uint8_t *d_in = nullptr;
    const int rc = pcm_dev_host_block(c, [&]() {
        if (const int rc = align_inputs(h_runs, n_pairs, false, h_lags, c->h_pcm_align, &L)) return rc;
        o_geo = up16(L.bytes);
        d_in = (uint8_t *)c->grab(kPoolInputs, o_geo + (size_t)n_pairs * sizeof(mp3s_pcm_pair));   // [tiles | given lags | geometry]
        if (!d_in) return fail(MP3S_E_NOMEM, "hipMalloc failed for %d workgroup entries", L.n_tiles);
        if (L.bytes) HIPCHK(hipMemcpyAsync(d_in, c->h_pcm_align.data(), L.bytes, hipMemcpyHostToDevice, c->stream));
        return (int)MP3S_OK;
    });
    if (rc) return rc;
    const int e = launch_pcm_align(c->stream, d_pcm, nch, d_runs, n_pairs, max_lag, search_rows, h_lags ? (const int32_t *)(d_in + L.o_lags) : nullptr,
                                   (const PcmTile *)(d_in + L.o_tiles), L.n_tiles, d_scores, d_lags, (mp3s_pcm_pair *)(d_in + o_geo), d_frames, d_out);
    if (e) return fail(MP3S_E_HIP, "pcm align launch: %s", hipGetErrorString((hipError_t)e));
    return MP3S_OK;
}

int mp3s_pcm_alignment_files(mp3s_ctx *c, const uint8_t *const *a, const size_t *a_lens, const uint8_t *const *b, const size_t *b_lens, int n_pairs,
                             int max_lag, int search_rows, const int32_t *lags, int want_profile, mp3s_buf **owner, mp3s_pcm_alignment *out, int32_t *status)
{
    if (!c || !a || !a_lens || !b || !b_lens || !owner || !out || n_pairs <= 0) return fail(MP3S_E_ARG, "bad argument");
    if (n_pairs > 0x3fffffff) return fail(MP3S_E_ARG, "n_pairs=%d", n_pairs);
    if (const int rc = check_search(n_pairs, 2, max_lag, search_rows, lags)) return rc;
    const mp3s_pcm_pair_diff nothing = {0, 0, 0, -1, 0, 0};
    return pcm_pairs_call(c, a, a_lens, b, b_lens, n_pairs, out, sizeof *out, owner, status,
                          // a stream without a frame: nothing to search; with a given lag the record of an empty overlap
                          [&](const mp3s_multi &m, int i) {
                              distortion_from_record(nothing, m.parsed[i], m.parsed[n_pairs + i], 0, 0, nullptr, &out[i].at_lag);
                              out[i].lag.lag = lags[i];
                          },
                          // a pair too short for the search is refused; the others are unaffected
                          [&](const mp3s_multi &m, FileStatus &fs, int i) {
                              const int64_t ra = 1152 * pcm_frames(m.parsed[i]), rb = 1152 * pcm_frames(m.parsed[n_pairs + i]);
                              if (lags || search_room(ra, rb, max_lag) >= 1) return false;
                              fs.set(i, fail(MP3S_E_UNSUPPORTED, "pair %d: %lld rows against %lld are too few to search lags up to max_lag = %d (more than %d rows are needed)", i,
                                             (long long)ra, (long long)rb, max_lag, 2 * max_lag));
                              return true;
                          },
                          [&](mp3s_multi &m, const std::vector<int> &idx, int nch, mp3s_buf *top) {
                              return align_group(c, m, n_pairs, idx, nch, max_lag, search_rows, lags, want_profile != 0, top, out);
                          });
}

}  // extern "C"
