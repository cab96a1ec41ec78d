// C-ABI of the library (include/mp3s.h), part 3e: does a file carry a payload, and how much -- the table audit of a list of MP3 files,
// on the frame of the list-of-files calls (mp3s_internal.h).  The files go the way of mp3s_decode_streams up to the Huffman decode
// (decode_front: no transform runs, no PCM exists); k_table_audit_units and k_table_audit_streams (k_table_audit.hpp) classify the
// regions there, and a record per file comes down, with the per-frame profile when it is asked for.
#include "mp3s_internal.h"

namespace {

void no_frames(const ParsedStream &p, mp3s_table_audit *out)
{
    std::memset(out, 0, sizeof *out);
    out->first_forced = out->last_forced = -1;
    out->channels = p.nch; out->sampling_rate = p.sampling_rate; out->kbps = p.bit_rate / 1000;
}

// The streams `idx` of m (one channel count, every one with a frame) as one batch; out[idx[k]] = stream k.  What the results point into
// (the profile) is kept in a new part of `top`.
int audit_group(mp3s_ctx *c, mp3s_multi &m, const std::vector<int> &idx, int nch, bool want_profile, mp3s_buf *top, mp3s_table_audit *out)
{
    DecodeFront F;
    int rc = decode_front(c, m, idx, nch, 0, F);
    if (rc) return rc;
    const long n = F.n;
    if (n <= 0) return fail(MP3S_E_ARG, "a batch without frames");
    // the side records of streams the host parsed from the start: the decode batch has zeros there, the scan has them
    for (size_t k = 0; k < idx.size(); k++) {
        const ScannedStream &sc = m.scanned[idx[k]];
        const long nf = m.parsed[idx[k]].n_frames;
        if ((long)sc.side.size() != nf)
            return fail(MP3S_E_UNSUPPORTED, "file %d: the scan kept no side records for its %ld frame(s)", idx[k], nf);
        if (!sc.host_parsed) continue;
        // (a stream that became host-parsed inside decode_front had its records uploaded there; writing them again changes nothing)
        rc = mp3s_dev_upload(c, (mp3s_frame_side *)F.d_side + F.first_of[k], sc.side.data(), (size_t)nf * sizeof(mp3s_frame_side));
        if (rc) return rc;
    }
    const size_t ns = idx.size();
    std::vector<mp3s_table_audit_seg> segs(ns);
    for (size_t k = 0; k < ns; k++) segs[k] = {(int32_t)F.first_of[k], (int32_t)m.parsed[idx[k]].n_frames};
    const size_t o_prof = up16(ns * sizeof(mp3s_table_audit)), res_bytes = o_prof + (want_profile ? (size_t)n * 4 : 0);
    // (the unit records lie where other calls keep PCM: the audit decodes none -- PoolSlot, mp3s_internal.h)
    void *d_units = c->grab(kPoolPcm0, (size_t)n * 4 * sizeof(mp3s_table_audit_unit)), *d_segs = c->grab(kPoolInputs, ns * sizeof(mp3s_table_audit_seg)),
         *d_res = c->grab(kPoolSmall, res_bytes);
    if (!d_units || !d_segs || !d_res) return fail(MP3S_E_NOMEM, "hipMalloc failed for the audit of %ld frames", n);
    std::unique_ptr<mp3s_buf> part(new mp3s_buf());
    if (!part->big[2].reserve(res_bytes)) return fail(MP3S_E_NOMEM, "hipHostMalloc failed for %zu bytes of audit results", res_bytes);
    rc = mp3s_dev_upload(c, d_segs, segs.data(), ns * sizeof(mp3s_table_audit_seg));
    if (rc) return rc;
    const int e = launch_table_audit(c->stream, (const int16_t *)F.d_is, (const mp3s_frame_side *)F.d_side, (int)n, nch, (const mp3s_table_audit_seg *)d_segs,
                                     (int)ns, (mp3s_table_audit_unit *)d_units, (mp3s_table_audit *)d_res,
                                     want_profile ? (uint32_t *)((uint8_t *)d_res + o_prof) : nullptr);
    if (e) return fail(MP3S_E_HIP, "table audit launch: %s", hipGetErrorString((hipError_t)e));
    rc = mp3s_dev_download(c, part->big[2].data(), d_res, res_bytes);
    if (rc) return rc;
    if (trace_on()) fprintf(stderr, "mp3s:   table audit: %zu stream(s), %ld frames, %zu bytes down\n", ns, n, res_bytes);
    const mp3s_table_audit *rec = (const mp3s_table_audit *)part->big[2].data();
    const uint32_t *profile = want_profile ? (const uint32_t *)(part->big[2].data() + o_prof) : nullptr;
    for (size_t k = 0; k < ns; k++) {
        const ParsedStream &p = m.parsed[idx[k]];
        mp3s_table_audit &o = out[idx[k]];
        o = rec[k];
        o.sampling_rate = p.sampling_rate; o.kbps = p.bit_rate / 1000;
        o.profile = profile ? profile + F.first_of[k] : nullptr;
    }
    top->parts.push_back(std::move(part));
    return MP3S_OK;
}

}  // namespace

extern "C" {

int mp3s_table_audit_dev(mp3s_ctx *c, const int16_t *d_is, const mp3s_frame_side *d_side, int n_frames, int nch, const mp3s_table_audit_seg *d_segs,
                         int n_segs, mp3s_table_audit_unit *d_units, mp3s_table_audit *d_out, uint32_t *d_profile)
{
    if (!c || !d_is || !d_side || !d_segs || !d_out) return fail(MP3S_E_ARG, "null pointer");
    if (n_frames <= 0 || n_segs <= 0) return fail(MP3S_E_ARG, "n_frames=%d, n_segs=%d", n_frames, n_segs);
    if (nch != 1 && nch != 2) return fail(MP3S_E_ARG, "nch=%d", nch);
    if (((uintptr_t)d_is & 3) || ((uintptr_t)d_units & 15)) return fail(MP3S_E_ARG, "d_is must be 4-byte, d_units 16-byte aligned");
    if (!d_units) {
        d_units = (mp3s_table_audit_unit *)c->grab(kPoolPcm0, (size_t)n_frames * 4 * sizeof(mp3s_table_audit_unit));
        if (!d_units) return fail(MP3S_E_NOMEM, "hipMalloc failed for the unit records of %d frames", n_frames);
    }
    const int e = launch_table_audit(c->stream, d_is, d_side, n_frames, nch, d_segs, n_segs, d_units, d_out, d_profile);
    if (e) return fail(MP3S_E_HIP, "table audit launch: %s", hipGetErrorString((hipError_t)e));
    return MP3S_OK;
}

int mp3s_table_audit_files(mp3s_ctx *c, const uint8_t *const *mp3s, const size_t *lens, int n_files, int want_profile, mp3s_buf **owner,
                           mp3s_table_audit *out, int32_t *status)
{
    if (!c || !mp3s || !lens || !owner || !out || n_files <= 0) return fail(MP3S_E_ARG, "bad argument");
    std::unique_ptr<mp3s_buf> top(new mp3s_buf());
    top->multi.reset(new mp3s_multi());
    mp3s_multi &m = *top->multi;
    FileStatus fs(n_files);
    FileGroups groups;                       // by channel count
    for (int i = 0; i < n_files; i++) std::memset(&out[i], 0, sizeof out[i]);
    const std::vector<int32_t> front = mp3_list_front(c, m, n_files, [&](int i) { return std::pair<const uint8_t *, size_t>(mp3s[i], lens[i]); });
    for (int i = 0; i < n_files; i++) {
        if (front[(size_t)i]) { fs.set(i, front_end_failed(front[(size_t)i], i)); continue; }
        const ParsedStream &p = m.parsed[i];
        if (p.n_frames <= 0) { no_frames(p, &out[i]); continue; }
        if (p.nch < 1 || p.nch > 2) { fs.set(i, fail(MP3S_E_MALFORMED, "file %d: channel count %d", i, p.nch)); continue; }
        groups.add(p.nch, 0, i);
    }
    run_groups(groups, [&](int nch, int, const std::vector<int> &idx) {
        const int rc = audit_group(c, m, idx, nch, want_profile != 0, top.get(), out);
        if (rc) for (int i : idx) std::memset(&out[i], 0, sizeof out[i]);
        return rc;
    }, fs, [] {});
    mp3_list_done(c, m);
    return finish_list(fs, status, top, owner);
}

}  // extern "C"
