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
