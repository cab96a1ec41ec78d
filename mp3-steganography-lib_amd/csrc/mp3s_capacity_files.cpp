// C-ABI of the library (include/mp3s.h), part 3d: how much fits -- the message capacity of a list of MP3 or WAV files, on the frame of
// the list-of-files calls (mp3s_internal.h).  The files go the way of mp3s_hide_messages / mp3s_encode_files up to the chain check of
// their (sampling rate, bitrate) group's encode batch; there the job stops (capacity_batch: no bit packing, no MP3 bytes) and k_capacity
// (k_capacity.hpp) counts the table indices the message cursor would advance by.  A few bytes per stream come down, and the profile
// when it is asked for.  A group whose verdict says that the guesses of the first pass did not hold goes through the full encode
// (encode_batch with the records) and is counted here on the host.
#include "mp3s_internal.h"

namespace {

// out = stream `seg` of a counted batch: the ONE place an EncSeg becomes an mp3s_capacity
void capacity_from_seg(const EncSeg &seg, int kbps, int rate, int64_t bits, int32_t active_units, const uint32_t *profile, int fallback, mp3s_capacity *out)
{
    std::memset(out, 0, sizeof *out);
    out->bits = bits; out->hide_offset = seg.hide_offset; out->text_bytes = mp3s_capacity_text_bytes(bits);
    out->too_long = seg.hide_offset < (int64_t)seg.n_hide - 1 ? 1 : 0;   // (file_from_seg's rule; there are no bytes to point at here)
    out->n_frames = seg.n_frames; out->kbps = kbps; out->sampling_rate = rate; out->channels = 2;
    out->active_units = active_units; out->fallback = fallback; out->profile = profile;
}

// The streams `segs` of one (sampling rate, bitrate), their PCM in HBM at d_pcm, counted as one batch; out[idx[k]] = stream k.  What the
// results point into (the profile) is kept in a new part of `top`.
int count_group(mp3s_ctx *c, const int16_t *d_pcm, std::vector<EncSeg> &segs, const std::vector<int> &idx, int samplerate, int kbps, bool want_profile,
                mp3s_buf *top, mp3s_capacity *out)
{
    std::unique_ptr<mp3s_buf> part(new mp3s_buf());
    CapacityBatch cb;
    int rc = capacity_batch(c, d_pcm, segs, samplerate, kbps, want_profile, part.get(), &cb);
    if (rc) return rc;
    if (cb.counted) {
        if (trace_on()) fprintf(stderr, "mp3s:   capacity: %zu stream(s) counted by k_capacity, %zu bytes down\n", idx.size(), cb.down_bytes);
        for (size_t k = 0; k < idx.size(); k++)
            capacity_from_seg(segs[k], kbps, samplerate, cb.seg[k].bits, cb.seg[k].active_units, cb.profile ? cb.profile + segs[k].first : nullptr, 0, &out[idx[k]]);
        top->parts.push_back(std::move(part));
        return MP3S_OK;
    }
    // the guesses did not hold: the full path resolves the chains (the PCM is still in HBM), the final records are counted here
    int passes = 0;
    rc = encode_batch(c, nullptr, d_pcm, segs, samplerate, kbps, part.get(), &passes, true);
    if (rc) return rc;
    size_t n_all = 0;
    for (const EncSeg &s : segs) n_all += (size_t)s.n_frames;
    part->lists.resize(1);
    if (want_profile) part->lists[0].resize(n_all * 4);
    uint32_t *const profile = want_profile ? reinterpret_cast<uint32_t *>(part->lists[0].data()) : nullptr;
    for (size_t k = 0; k < idx.size(); k++) {
        const EncSeg &s = segs[k];
        int64_t bits = 0;
        int32_t active = 0;
        for (int f = 0; f < s.n_frames; f++) {
            for (int u = 0; u < 4; u++) {
                const mp3s_gr_out &g = part->gr_out[((size_t)s.first + f) * 4 + u];
                if (g.flags & MP3S_RF_ACTIVE) { bits += g.n_tables; active++; }
            }
            if (profile) profile[(size_t)s.first + f] = (uint32_t)bits;
        }
        capacity_from_seg(s, kbps, samplerate, bits, active, profile ? profile + s.first : nullptr, 1, &out[idx[k]]);
    }
    top->parts.push_back(std::move(part));
    return MP3S_OK;
}

}  // namespace

extern "C" {

int64_t mp3s_capacity_text_bytes(int64_t bits)
{
    // n_hide = 8 * (digits(n) + 1 + n), and n_hide - 1 <= bits: n + digits(n) + 1 <= room, in bytes
    const int64_t room = bits < 0 ? 0 : (bits + 1) / 8;
    auto framed = [](int64_t n) { int64_t d = 1; for (int64_t t = n; t >= 10; t /= 10) d++; return n + d + 1; };
    int64_t n = std::max<int64_t>(room - 2, 0);          // (one digit; every further digit takes one byte of text away)
    while (n > 0 && framed(n) > room) n--;
    return n;
}

int mp3s_capacity_dev(mp3s_ctx *c, const mp3s_gr_out *d_gr, const mp3s_chain_seg *d_segs, int n_segs, mp3s_capacity_seg *d_out, uint32_t *d_profile)
{
    if (!c || !d_gr || !d_segs || !d_out) return fail(MP3S_E_ARG, "null pointer");
    if (n_segs <= 0) return fail(MP3S_E_ARG, "n_segs=%d", n_segs);
    const int e = launch_capacity(c->stream, d_gr, d_segs, n_segs, d_out, d_profile);
    if (e) return fail(MP3S_E_HIP, "capacity launch: %s", hipGetErrorString((hipError_t)e));
    return MP3S_OK;
}

int mp3s_capacity_files(mp3s_ctx *c, const uint8_t *const *mp3s, const size_t *lens, int n_files, const uint8_t *const *msgs,
                        const size_t *msg_lens, int want_profile, mp3s_buf **owner, mp3s_capacity *out, int32_t *status)
{
    if (!c || !mp3s || !lens || !owner || !out || n_files <= 0 || (msgs && !msg_lens)) return fail(MP3S_E_ARG, "bad argument");
    // ---- the front of the re-encoding calls (file_lists.cpp): scan, the reference's checks, messages, groups
    std::unique_ptr<mp3s_buf> top(new mp3s_buf());
    top->multi.reset(new mp3s_multi());
    mp3s_multi &m = *top->multi;
    std::vector<std::vector<uint8_t>> bits;
    FileStatus fs(n_files);
    FileGroups groups;                       // by (sampling rate, kbps)
    for (int i = 0; i < n_files; i++) std::memset(&out[i], 0, sizeof out[i]);
    reencode_list_front(c, m, mp3s, lens, n_files, msgs, msg_lens, fs, bits, groups);
    // ---- per group: decode into HBM as reencode_group does, then the encode without its tail
    run_groups(groups, [&](int rate, int kbps, const std::vector<int> &idx) {
        std::vector<EncSeg> segs;
        std::vector<std::vector<uint8_t>> guess;
        void *d_keep = nullptr;
        int64_t rows_frames = 0;
        int rc = reencode_decode(c, m, idx, bits, segs, guess, &d_keep, &rows_frames);
        if (!rc) rc = count_group(c, (const int16_t *)d_keep, segs, idx, rate, kbps, want_profile != 0, top.get(), out);
        if (rc) for (int i : idx) std::memset(&out[i], 0, sizeof out[i]);
        return rc;
    }, fs, [] {});
    mp3_list_done(c, m);
    return finish_list(fs, status, top, owner);
}

int mp3s_capacity_wavs(mp3s_ctx *c, const uint8_t *const *wavs, const size_t *lens, int n_files, const int32_t *bitrate_kbps,
                       const uint8_t *const *hide_bits, const int32_t *n_hide, int want_profile, mp3s_buf **owner, mp3s_capacity *out,
                       int32_t *status)
{
    if (!c || !wavs || !lens || !bitrate_kbps || !owner || !out || n_files <= 0 || (hide_bits && !n_hide)) return fail(MP3S_E_ARG, "bad argument");
    const WavRead how = wav_read_of(c);
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
        std::vector<EncSeg> segs;
        WavBatch wb;
        void *d_pcm = nullptr;
        int rc = wav_to_device(c, in, idx, segs, wb, &d_pcm);
        if (!rc) rc = count_group(c, (const int16_t *)d_pcm, segs, idx, rate, kbps, want_profile != 0, top.get(), out);
        if (rc) {
            (void)hipStreamSynchronize(c->stream);   // (the batch's records are the source of copies that may still be in flight)
            for (int i : idx) std::memset(&out[i], 0, sizeof out[i]);
        }
        return rc;
    }, fs, [&] { (void)hipStreamSynchronize(c->stream); });
    return finish_list(fs, status, top, owner);
}

}  // extern "C"
