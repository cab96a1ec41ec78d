// C-ABI of the library (include/mp3s.h), part 3c: a list of MP3 files in, their hidden messages out -- the counterpart of
// mp3s_hide_messages.  The host walks every file from header to header (FrameWalker, on the context's scan threads); the files the
// walk calls regular go up as they are, one image for the batch, and k_reveal (k_reveal.hpp) reads the stego bits out of their
// side info, one workgroup per stream; packed bits and counts come down in one copy.  Every other file takes the byte-level scan
// on the host.  Nothing here depends on a stream's sampling rate, bitrate or channel count: a mixed list is ONE batch.
#include "mp3s_internal.h"

namespace {

constexpr size_t kRevealMaxImage = 0xfffffff0u;   // offsets into the image are 32 bits wide

struct RevFile {
    bool dev = false;                       // the walk vouches for the stream: its bits come from the device
    std::vector<FrameRef> refs;             // ... its frames, counted from the start of the file
    int32_t n_frames = 0, nch = 0, sampling_rate = 0, bit_rate = 0;
};
struct HostScan { ParsedStream p; ScannedStream sc; };   // one per scan thread: the vectors keep their room from file to file

// the byte-level scan (what mp3s_scan_stream and mp3s_reveal_message run) for a file the device does not take
int host_reveal(const uint8_t *file, size_t len, HostScan &h, RevFile &r, std::vector<uint8_t> &bits, std::vector<uint8_t> &text)
{
    r.dev = false; r.refs.clear(); r.refs.shrink_to_fit();
    const int rc = parse_stream(file, len, h.p, &h.sc);
    if (rc) return rc;
    r.n_frames = h.p.n_frames; r.nch = h.p.nch; r.sampling_rate = h.p.sampling_rate; r.bit_rate = h.p.bit_rate;
    bits.assign(h.p.bits.begin(), h.p.bits.end());
    message_reveal(bits.data(), bits.size(), text);
    return MP3S_OK;
}

// the files `idx` (in image order) through k_reveal: bits[i] (0/1 bytes) and dev_status[i] for each
int reveal_launch(mp3s_ctx *c, const uint8_t *const *mp3s, const size_t *lens, std::vector<RevFile> &rf, const std::vector<int> &idx,
                  std::vector<std::vector<uint8_t>> &lists)
{
    const size_t ns = idx.size();
    std::vector<Upload> files;
    std::vector<size_t> place(ns);
    size_t img = 0;
    uint64_t nf = 0, packed = 0;
    for (size_t k = 0; k < ns; k++) {
        place[k] = up16(img);
        img = place[k] + lens[idx[k]];
        files.push_back({place[k], mp3s[idx[k]], lens[idx[k]]});
        nf += (uint64_t)rf[(size_t)idx[k]].n_frames;
        packed += reveal_packed_bytes((uint64_t)rf[(size_t)idx[k]].n_frames);
    }
    if (img > kRevealMaxImage || nf > 0xffffffffull || packed > 0xffffffffull) return fail(MP3S_E_ARG, "reveal batch too large");
    // what goes up: [image | frame refs | stream refs | output offsets]; what comes down: [bit counts | status words | packed bits]
    const size_t o_refs = up16(img), o_streams = o_refs + (size_t)nf * sizeof(FrameRef), o_off = up16(o_streams + ns * sizeof(StreamRef)),
                 in_end = up16(o_off + ns * 4);
    const size_t o_st = ns * 4, o_pk = up16(2 * ns * 4), out_bytes = o_pk + (size_t)packed;
    std::vector<uint8_t> rec(in_end - o_refs, 0);
    FrameRef *refs = reinterpret_cast<FrameRef *>(rec.data());
    StreamRef *streams = reinterpret_cast<StreamRef *>(rec.data() + (o_streams - o_refs));
    uint32_t *out_off = reinterpret_cast<uint32_t *>(rec.data() + (o_off - o_refs));
    uint32_t first = 0, pk = 0;
    for (size_t k = 0; k < ns; k++) {
        const RevFile &r = rf[(size_t)idx[k]];
        const uint32_t n = (uint32_t)r.n_frames;
        for (uint32_t f = 0; f < n; f++) {
            FrameRef x = r.refs[f];
            x.file_off += (uint32_t)place[k]; x.stream = (uint16_t)k;
            refs[first + f] = x;
        }
        StreamRef &s = streams[k];
        s.base = (uint32_t)place[k]; s.end = (uint32_t)(place[k] + lens[idx[k]]); s.first_frame = first; s.n_frames = n;
        FrameWalker::history(r.refs.data(), 0, s.prev_size);
        out_off[k] = pk;
        first += n; pk += (uint32_t)reveal_packed_bytes(n);
    }
    files.push_back({o_refs, rec.data(), rec.size()});
    HIPCHK(hipSetDevice(c->device));
    uint8_t *d_in = (uint8_t *)c->grab(kPoolReveal, in_end + out_bytes);
    PinnedBlock down;
    if (!d_in || !down.reserve(out_bytes)) return fail(MP3S_E_NOMEM, "no memory for a reveal batch of %zu bytes", in_end + out_bytes);
    uint8_t *d_out = d_in + in_end;
    std::vector<Upload> ups;
    if (!plan_uploads(files, [&](size_t extent) { if (c->h_blob.size() < extent) c->h_blob.resize(extent); return c->h_blob.data(); }, ups))
        return fail(MP3S_E_NOMEM, "no staging for a reveal batch");
    const double t0 = trace_on() ? now_ms() : 0;
    int rc = MP3S_OK;
    for (const Upload &u : ups)
        if (hipMemcpyAsync(d_in + u.dst, u.src, u.bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) { rc = fail(MP3S_E_HIP, "upload of a reveal batch failed"); break; }
    if (!rc) {
        const int e = launch_reveal(c->stream, d_in, 0, (const FrameRef *)(d_in + o_refs), (const StreamRef *)(d_in + o_streams), (int)ns,
                                    (const uint32_t *)(d_in + o_off), d_out + o_pk, (int32_t *)d_out, (int32_t *)(d_out + o_st));
        if (e) rc = fail(MP3S_E_HIP, "reveal launch: %s", hipGetErrorString((hipError_t)e));
    }
    if (!rc && hipMemcpyAsync(down.data(), d_out, out_bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) rc = fail(MP3S_E_HIP, "download of a reveal batch failed");
    const hipError_t es = hipStreamSynchronize(c->stream);   // (also after a failure: copies in flight read the callers' bytes and the staging)
    if (rc) return rc;
    if (es != hipSuccess) return fail(MP3S_E_HIP, "reveal batch: %s", hipGetErrorString(es));
    if (trace_on()) fprintf(stderr, "mp3s:   reveal_messages: %zu stream(s), %llu frames, %zu bytes up in %zu copies: %.3f ms\n", ns, (unsigned long long)nf, in_end, ups.size(), now_ms() - t0);
    const int32_t *nb = (const int32_t *)down.data(), *dst = (const int32_t *)(down.data() + o_st);
    for (size_t k = 0; k < ns; k++) {
        RevFile &r = rf[(size_t)idx[k]];
        const int64_t n = nb[k];
        if (dst[k] != 0 || n < 0 || n > (int64_t)r.n_frames * 12) { r.dev = false; continue; }   // (the caller sends it through the host scan)
        std::vector<uint8_t> &bits = lists[2 * (size_t)idx[k] + 1];
        bits.resize((size_t)n);
        const uint8_t *p = down.data() + o_pk + out_off[k];
        for (int64_t b = 0; b < n; b++) bits[(size_t)b] = (p[b >> 3] >> (7 - (b & 7))) & 1;
        message_reveal(bits.data(), bits.size(), lists[2 * (size_t)idx[k]]);
    }
    return MP3S_OK;
}

}  // namespace

// mp3s_reveal_messages with the limits of a launch named by the caller (the test aid mp3s_debug_reveal_messages)
static int reveal_files(mp3s_ctx *c, const uint8_t *const *mp3s, const size_t *lens, int n_files, int max_streams, size_t max_image,
                 mp3s_buf **owner, mp3s_file *out, int32_t *status)
{
    if (!c || !mp3s || !lens || !owner || !out || n_files <= 0) return fail(MP3S_E_ARG, "bad argument");
    if (max_streams < 1 || max_streams > kRevealMaxStreams || max_image < 1 || max_image > kRevealMaxImage) return fail(MP3S_E_ARG, "bad launch limits");
    std::unique_ptr<mp3s_buf> top(new mp3s_buf());
    top->lists.resize(2 * (size_t)n_files);   // per file: the text, the 0/1 bits
    std::vector<RevFile> rf((size_t)n_files);
    FileStatus fs(n_files);
    std::vector<int32_t> &st = fs.st;
    size_t total = 0;
    for (int i = 0; i < n_files; i++) {
        std::memset(&out[i], 0, sizeof out[i]);
        if (!mp3s[i]) st[(size_t)i] = MP3S_E_ARG;
        else total += lens[i];
    }
    // ---- front end: the walk, and the byte-level scan for what the walk does not take
    const int workers = file_workers(n_files, total, default_scan_threads(c));
    std::vector<HostScan> scratch((size_t)std::max(workers, 1));
    const double t0 = trace_on() ? now_ms() : 0;
    parallel_files(workers, n_files, [&](int w, int i) {
        RevFile &r = rf[(size_t)i];
        if (st[(size_t)i]) return;
        FrameWalker fw;
        const long n = lens[i] <= max_image ? walk_whole(mp3s[i], lens[i], r.refs, fw) : -1;
        if (n > 0 && n <= 0x7fffffff / 12) {
            r.dev = true;
            r.n_frames = (int32_t)n; r.nch = fw.nch; r.sampling_rate = fw.sampling_rate; r.bit_rate = fw.bit_rate;
            return;
        }
        st[(size_t)i] = host_reveal(mp3s[i], lens[i], scratch[(size_t)w], r, top->lists[2 * (size_t)i + 1], top->lists[2 * (size_t)i]);
    });
    const double t1 = trace_on() ? now_ms() : 0;
    // ---- the device's share, in launches of at most max_streams streams and max_image bytes of image
    std::vector<int> idx;
    size_t img = 0;
    int n_launches = 0, rc = MP3S_OK;
    auto flush = [&]() {
        if (idx.empty() || rc) return;
        rc = reveal_launch(c, mp3s, lens, rf, idx, top->lists);
        n_launches++;
        idx.clear(); img = 0;
    };
    for (int i = 0; i < n_files && !rc; i++) {
        if (!rf[(size_t)i].dev) continue;
        size_t at = up16(img);
        if ((int)idx.size() == max_streams || at + lens[i] > max_image) { flush(); at = 0; }
        idx.push_back(i);
        img = at + lens[i];
    }
    flush();
    if (rc) return rc;
    // a stream the kernel flagged (a reference it would not follow): the host scan decides
    for (int i = 0; i < n_files; i++) {
        RevFile &r = rf[(size_t)i];
        if (st[(size_t)i] || r.dev || !r.refs.size()) continue;
        st[(size_t)i] = host_reveal(mp3s[i], lens[i], scratch[0], r, top->lists[2 * (size_t)i + 1], top->lists[2 * (size_t)i]);
    }
    if (trace_on()) fprintf(stderr, "mp3s: reveal_messages, %d file(s): front end %.3f ms on %d thread(s), %d launch(es) %.3f ms\n", n_files, t1 - t0, workers, n_launches, now_ms() - t1);
    for (int i = 0; i < n_files; i++) {
        const RevFile &r = rf[(size_t)i];
        if (st[(size_t)i]) { fs.set(i, front_end_failed(st[(size_t)i], i)); continue; }
        const std::vector<uint8_t> &text = top->lists[2 * (size_t)i], &bits = top->lists[2 * (size_t)i + 1];
        mp3s_file &o = out[i];
        o.data = text.data(); o.len = text.size();
        o.kbps = r.bit_rate / 1000; o.sampling_rate = r.sampling_rate; o.channels = r.nch; o.n_frames = r.n_frames;
        o.n_bits = (int32_t)bits.size(); o.bits = bits.data();
    }
    return finish_list(fs, status, top, owner);
}

extern "C" {

int mp3s_reveal_bits_dev(mp3s_ctx *c, const uint8_t *d_image, uint32_t image_base, const mp3s_frame_ref *d_refs, const mp3s_stream_ref *d_streams,
                         int n_streams, const uint32_t *d_out_off, uint8_t *d_packed, int32_t *d_n_bits, int32_t *d_status)
{
    if (!c || !d_image || !d_refs || !d_streams || !d_out_off || !d_packed || !d_n_bits || !d_status) return fail(MP3S_E_ARG, "null pointer");
    if (n_streams <= 0 || n_streams > kRevealMaxStreams) return fail(MP3S_E_ARG, "n_streams=%d (1 .. %d a launch)", n_streams, kRevealMaxStreams);
    const int e = launch_reveal(c->stream, d_image, image_base, d_refs, d_streams, n_streams, d_out_off, d_packed, d_n_bits, d_status);
    if (e) return fail(MP3S_E_HIP, "reveal launch: %s", hipGetErrorString((hipError_t)e));
    return MP3S_OK;
}

int mp3s_reveal_messages(mp3s_ctx *c, const uint8_t *const *mp3s, const size_t *lens, int n_files, mp3s_buf **owner, mp3s_file *out, int32_t *status)
{
    return reveal_files(c, mp3s, lens, n_files, kRevealMaxStreams, kRevealMaxImage, owner, out, status);
}

int mp3s_debug_reveal_messages(mp3s_ctx *c, const uint8_t *const *mp3s, const size_t *lens, int n_files, int max_streams, mp3s_buf **owner,
                               mp3s_file *out, int32_t *status)
{
    return reveal_files(c, mp3s, lens, n_files, max_streams, kRevealMaxImage, owner, out, status);
}

}  // extern "C"
