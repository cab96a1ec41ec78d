// The frame of the list-of-files calls (mp3s_internal.h): the pieces of it that are no templates.
#include "mp3s_internal.h"

long walk_whole(const uint8_t *file, size_t len, std::vector<FrameRef> &refs, FrameWalker &w, std::vector<uint8_t> *tables, long tables_wanted)
{
    const int rc = w.open(file, len);
    if (rc) { w.error = rc; return -1; }
    w.tables_wanted = tables_wanted;
    refs.resize(std::max(refs.size(), len / 96 + 64));
    for (size_t n = 0;;) {
        if (tables && tables->size() < refs.size() * 4) tables->resize(refs.size() * 4);
        if (w.ended || w.irregular) return w.irregular || n == 0 ? -1 : (long)n;
        n += (size_t)w.next(refs.data() + n, (long)(refs.size() - n), tables ? tables->data() + n * 4 : nullptr, 0, 0);
        if (n == refs.size()) refs.resize(2 * n);
    }
}

void file_from_seg(const EncSeg &seg, const uint8_t *mp3_base, int kbps, int rate, int64_t hide_offset, mp3s_file *out)
{
    std::memset(out, 0, sizeof *out);
    out->data = mp3_base + seg.mp3_off; out->len = seg.mp3_len;
    out->kbps = kbps; out->sampling_rate = rate; out->channels = 2; out->n_frames = seg.n_frames;
    out->hide_offset = hide_offset;
    out->too_long = hide_offset < (int64_t)seg.n_hide - 1 ? 1 : 0;
}

std::vector<int32_t> mp3_list_front(mp3s_ctx *c, mp3s_multi &m, int n_files, const std::function<std::pair<const uint8_t *, size_t>(int)> &file_of)
{
    m.parsed.resize(n_files); m.scanned.resize(n_files); m.pcm.assign(n_files, nullptr); m.files.resize(n_files);
    std::vector<int32_t> st((size_t)n_files, MP3S_OK);
    size_t total = 0;
    for (int i = 0; i < n_files; i++) {
        const std::pair<const uint8_t *, size_t> f = file_of(i);
        if (!f.first) { st[(size_t)i] = MP3S_E_ARG; continue; }
        m.files[i] = f;
        total += f.second;
    }
    if (n_files == 1) m.scanned[0] = std::move(c->spare_scan);   // its capacity: no fresh pages for the blob of a long file
    parallel_files(file_workers(n_files, total, host_threads16()), n_files, [&](int, int i) { if (!st[(size_t)i]) st[(size_t)i] = front_end(m, i); });
    return st;
}

void mp3_list_done(mp3s_ctx *c, mp3s_multi &m)
{
    if (m.files.size() == 1) c->spare_scan = std::move(m.scanned[0]);
    m.files.clear();   // borrowed pointers
}

void reencode_list_front(mp3s_ctx *c, mp3s_multi &m, const uint8_t *const *mp3s, const size_t *lens, int n_files, const uint8_t *const *msgs,
                         const size_t *msg_lens, FileStatus &fs, std::vector<std::vector<uint8_t>> &bits, FileGroups &groups, double *t_scanned)
{
    const std::vector<int32_t> front = mp3_list_front(c, m, n_files, [&](int i) {
        const bool bad = !mp3s[i] || (msgs && msgs[i] == nullptr && msg_lens[i]);
        return std::pair<const uint8_t *, size_t>(bad ? nullptr : mp3s[i], lens[i]);
    });
    if (t_scanned) *t_scanned = now_ms();
    bits.resize((size_t)n_files);
    for (int i = 0; i < n_files; i++) {
        int kbps = 0;
        if (front[(size_t)i]) { fs.set(i, front_end_failed(front[(size_t)i], i)); continue; }
        fs.set(i, reencode_check(m.parsed[i], &kbps));
        if (fs.st[(size_t)i]) continue;
        if (msgs && msgs[i]) message_frame(msgs[i], msg_lens[i], bits[(size_t)i]);
        groups.add(m.parsed[i].sampling_rate, kbps, i);
    }
}

int front_end_failed(int code, int i)
{
    return fail(code, code == MP3S_E_ARG ? "file %d: null pointer" : "file %d: malformed or unsupported MP3 stream", i);
}

int finish_files(const FileStatus &fs, int32_t *status)
{
    int first_bad = MP3S_OK;
    for (size_t i = 0; i < fs.st.size(); i++) {
        if (status) status[i] = fs.st[i];
        if (fs.st[i] && !first_bad) first_bad = fail(fs.st[i], "%s", fs.why[i].c_str());
    }
    return first_bad;
}

int finish_list(const FileStatus &fs, int32_t *status, std::unique_ptr<mp3s_buf> &top, mp3s_buf **owner)
{
    const int first_bad = finish_files(fs, status);
    if (!status && first_bad) return first_bad;
    *owner = top.release();
    return MP3S_OK;
}
