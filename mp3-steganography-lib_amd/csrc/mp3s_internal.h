// Shared by the translation units behind include/mp3s.h (mp3s_api.cpp, mp3s_decode_pipeline.cpp,
// mp3s_encode_pipeline.cpp): the context, result owners, page-locked blocks and the pipeline helpers.  Nothing here is
// part of the C-ABI.
#pragma once
#include <hip/hip_runtime_api.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/mp3s.h"
#include "mp3s_device.h"
#include "mp3s_host.h"

namespace mp3s {
// records the text mp3s_last_error() returns on this thread; returns `code`
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
}  // namespace mp3s

using namespace mp3s;

#define HIPCHK(call)                                                                                 \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) return fail(MP3S_E_HIP, "%s: %s", #call, hipGetErrorString(e_));       \
    } while (0)

// The device buffers a context keeps between calls (mp3s_ctx::grab), one name per buffer.  A buffer with several users is shared on purpose;
// what keeps them apart is said here, and a new user says it here too.
//   One call at a time per context covers most of it: a list call, a one-file call or an encode has synchronised the context's stream when
//   it returns, and within a call the users below follow each other on that stream.
//   A pipe owns its context while it exists (mp3s.h): no other call runs beside its jobs.  They alternate between two sets of {Is, Si, Pcm}
//   -- job k + 1 fills the other set while job k's is read -- and a set is written again only behind the events of the job that had it
//   (e_dec, e_enc, e_down: pipe_jobs.cpp).  ChainAgg and the Var* buffers are one per context: the jobs' rate loops, selections and chain
//   checks follow each other on the compute and tail streams (tail_from, ev_sel).
//   The _dev calls (test aids on the caller's device arrays, nothing waited for) queue on the context's stream: what a later call writes
//   to a buffer they share lies behind their reads, and a regrow synchronises that stream first.  ChainDev is theirs alone.
enum PoolSlot : int {
    kPoolIs0, kPoolSi0,     // Huffman output of a decode batch (decode_front) or of set 0 of a pipe: samples [frames][2][2][576] int16, granule records
    kPoolFrameHdr, kPoolPcmChunk, kPoolHufStatus, kPoolMainData, kPoolSideInfo,   // decode_front: headers, a chunk of PCM on its way down, Huffman status, main data, side records
    kPoolPcm0,              // int16 PCM that stays on the device: reencode_decode, the pair calls, wav_to_device, the PCM batch calls (mp3s_pcm_batch.cpp), set 0 of a pipe; the table audit, which decodes no PCM, keeps its unit records here
    kPoolPcmUp,             // the PCM an encode brings from the host (encode_batch without pcm_dev)
    kPoolInputs,            // the host-made input block of the call: the encoder's (EncLayout), the pair calls', the audit's stream table, the workgroup tables of mp3s_pcm_diff_dev / mp3s_pcm_align_dev, [items | workgroup table] of the PCM batch launches, [streams or items | workgroup table] of the QMDCT launches (mp3s_qmdct_files.cpp)
    kPoolMdct,              // encode_batch, capacity_batch: MDCT lines [n_all][2][2][576]
    kPoolRedo,              // enc_resolve: entries of the exact re-runs
    kPoolIx, kPoolGrOut, kPoolEnergy,   // encode_batch, capacity_batch: quantised lines, GrInfo records, band energies
    kPoolChainAgg,          // chain_agg_bytes(n) of the chain check: encode_batch, capacity_batch, every job of a pipe
    kPoolMp3, kPoolScfsi,   // encode_batch: the packed bytes, the scalefactor selection (capacity_batch packs nothing and takes neither)
    kPoolSmall,             // the small results one copy brings down: of an encode (small_bytes; capacity_batch: + capacity records and profile), of the pair calls, of the audit, the QMDCT feature records
    kPoolVarEntries, kPoolVarIx, kPoolVarOut, kPoolVarEnergy, kPoolVarPairs,   // message variants: enc_resolve's launches take all five, the entries inside the first rate-loop launch
                            // (enc_variant_buffers) Ix, Out and Energy -- their selection is through before a resolve begins
    kPoolIs1, kPoolSi1, kPoolPcm1,      // set 1 of a pipe
    kPoolWavImage, kPoolResampleRows,   // wav_to_device: the files' bytes with the kernels' records behind them; PCM at the source rate for the resampler (k_wav_resample's input: wav_to_device's imported files, and the frames k_pcm_unbatch makes for mp3s_pcm_batch_encode_at)
    kPoolSelectDev,         // scratch of select_step, grown behind a synchronise of the stream the step was given alone: its users all run on one stream at a time -- the
                            // context's, or for the jobs of a pipe with a tail stream that tail (from pipe_create, which drains the context's stream, to pipe_quiesce, which drains the pipe's)
    kPoolChainDev,          // scratch of mp3s_chain_resolve_dev and mp3s_chain_redo_dev
    kPoolReveal,            // mp3s_reveal_messages: a batch's [files | records | packed bits out]
    kPoolSlotCount
};
constexpr PoolSlot kPoolIs[2] = {kPoolIs0, kPoolIs1}, kPoolSi[2] = {kPoolSi0, kPoolSi1}, kPoolPcm[2] = {kPoolPcm0, kPoolPcm1};   // by Job::set

struct mp3s_pipe;
struct ChainResolver;
struct mp3s_ctx {
    int device = 0;
    int64_t opt[MP3S_OPT_COUNT] = {0};   // MP3S_OPT_*: defaults from the environment at creation, then mp3s_ctx_set_option
    mp3s_run_stats run_stats = {0, 0, 0, 0, 0};
    mp3s_pipe *own_pipe = nullptr;       // the overlapped stages the one-file calls run their chunks through (made on first use)
    std::vector<mp3s_pipe *> parked_pipes;   // own pipes that became too small (a file with larger frames came): quiet, kept until the context goes (run_file.cpp)
    int sink_fd = -1; size_t sink_done = 0, sink_base = 0; bool sink_early = false;   // (sink_early: the file was empty when the call began -- only then do chunks go to it before the call has succeeded)
   // mp3s_*_fd: the file the result goes to, how many of its bytes (behind sink_base: the WAV header's place) run_file has written already
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_order = nullptr;
    hipEvent_t ev_sel = nullptr; bool sel_pending = false;   // a selection on another stream than the context's has read the variant buffers (select_step; rate_step waits)
    int32_t *d_sync = nullptr;        // 64-bit word {finished workgroups | error bits} of the pack kernel in flight (k_sync.hpp): self-clearing;
                                      // [2] counts the samples the fast synthesis computed again in the exact order
    double synth_eps_scale = 1.0;     // int16 decode: scale of the fast synthesis guard (0 = always the exact kernel)
    GuardProbe guard_probe = {nullptr, nullptr, 0, 0};   // mp3s_debug_guard_margin
    void *scratch = nullptr, *scratch_enc = nullptr; size_t scratch_bytes = 0, scratch_enc_bytes = 0;   // of the decode, of the encode transforms
    Profiler prof;
    // device buffers of the stream pipelines, kept between calls (hipMalloc/hipFree cost more than a small file's work)
    static constexpr int kPoolSlots = 32;
    // the packed tap tables of the resampler (MP3S_OPT_WAV_RESAMPLE), one per ratio the context has met (mp3s_encode_files.cpp)
    struct ResampleTaps { int L, M, T; uint32_t *d; };
    std::vector<ResampleTaps> res_taps;
    void *pool[kPoolSlots] = {nullptr};
    size_t pool_bytes[kPoolSlots] = {0};
    void *grab(PoolSlot slot, size_t bytes, hipStream_t user = nullptr /* the stream the buffer's users run on; null: the context's */)
    {
        if (slot < 0 || slot >= kPoolSlots) return nullptr;   // (callers answer MP3S_E_NOMEM)
        if (bytes < 16) bytes = 16;
        if (pool_bytes[slot] >= bytes) return pool[slot];
        if (pool[slot]) { hipStreamSynchronize(user ? user : stream); hipFree(pool[slot]); pool[slot] = nullptr; pool_bytes[slot] = 0; }
        const size_t want = bytes + bytes / 4;   // head room: similar-sized files reuse the buffer
        if (hipMalloc(&pool[slot], want) != hipSuccess) { pool[slot] = nullptr; return nullptr; }
        pool_bytes[slot] = want;
        return pool[slot];
    }
    // host-side work arrays of the encoder, kept between calls: beyond a few MB a fresh vector means fresh pages from
    // the kernel on every call (page faults cost more than the work done in them).  Those of the host's chain resolver are its own
    // (chain_resolve.h, which needs the encoder's types below: made and freed with the context, mp3s_api.cpp)
    ChainResolver *chain = nullptr;
    std::vector<uint8_t> h_in;
    // ... and of the decoder: the concatenated batch
    std::vector<mp3s_frame_hdr> h_hdr;
    std::vector<mp3s_frame_side> h_side;
    std::vector<uint8_t> h_blob;
    // ... and the scan result of the last single-file call, lent to the next one for its capacity
    ScannedStream spare_scan;
    // ... and the frame table / table counts of the file run_file is working on
    std::vector<FrameRef> h_refs;
    std::vector<uint8_t> h_tables;
    // ... and the workgroup table of the last mp3s_pcm_diff_dev, which travels on the stream behind the call: ev_pcm_tiles (made on first
    // use) is recorded behind its copy, the next call waits for it before it writes the table again
    std::vector<PcmTile> h_pcm_tiles;
    hipEvent_t ev_pcm_tiles = nullptr;
    // ... and the block [workgroup table | given lags] of the last mp3s_pcm_align_dev, by the same rule and behind the same event
    std::vector<uint8_t> h_pcm_align;
    // ... and the block [items | workgroup table] of the last PCM batch launch (mp3s_pcm_batch.cpp) or QMDCT launch (mp3s_qmdct_files.cpp), by the same rule and behind the same event
    std::vector<uint8_t> h_pcm_batch;
    static int ensure(void *&buf, size_t &have, size_t bytes)
    {
        if (bytes <= have) return 0;
        if (buf) { hipFree(buf); buf = nullptr; have = 0; }
        hipError_t e = hipMalloc(&buf, bytes);
        if (e != hipSuccess) return fail(MP3S_E_NOMEM, "hipMalloc(%zu) for scratch: %s", bytes, hipGetErrorString(e));
        have = bytes;
        return 0;
    }
    int ensure_scratch(size_t bytes) { return ensure(scratch, scratch_bytes, bytes); }
    // the encode transforms' scratch (subband samples between analysis and MDCT) is a buffer of its own: in the pipe the decode
    // transforms of the next job run on another stream beside them
    int ensure_scratch_enc(size_t bytes) { return ensure(scratch_enc, scratch_enc_bytes, bytes); }
};
static_assert(kPoolSlotCount <= mp3s_ctx::kPoolSlots, "every PoolSlot needs a place in mp3s_ctx::pool");

// Page-locked host memory for large results (decoded PCM): the device writes it at PCIe speed, no bounce buffer, no
// page faults.  Pinning costs more than the copy it saves, so blocks are kept and reused: process-wide, because a
// result may outlive the context that produced it.  (Blocks still cached at exit are left to the OS.)
// mp3s_debug_guard_margin's probe is an instantiation of the stream kernel: an int16 decode that would take another route while the probe is set
// (MP3S_OPT_FUSED_DECODE or MP3S_OPT_FAST_IMDCT off, the guard switched off) is refused -- it would leave the probe's arrays as they were.
// (Float formats never fill them and pass.)
inline int guard_probe_usable(const mp3s_ctx *c, int out_format)
{
    if (!c->guard_probe.x || out_format != MP3S_PCM_I16) return MP3S_OK;
    if (c->opt[MP3S_OPT_FUSED_DECODE] && c->opt[MP3S_OPT_FAST_IMDCT] && c->synth_eps_scale > 0 && c->d_sync) return MP3S_OK;
    return fail(MP3S_E_ARG, "the guard probe is set (mp3s_debug_guard_margin) and this int16 decode would not run the stream kernel that fills it "
                            "(MP3S_OPT_FUSED_DECODE / MP3S_OPT_FAST_IMDCT off, or the guard's scale is 0)");
}

// How this context decodes (DecodeHow, mp3s_device.h): its options, its guard scale and its counters.  The caller's: sf_base, the event the
// transforms complete, and where the launch's first sample lies in the guard probe's arrays (a batch's chunks fill them side by side).
inline DecodeHow decode_how(mp3s_ctx *c, int sf_base, hipEvent_t done, int64_t probe_base)
{
    if (c->guard_probe.x) c->guard_probe.base = probe_base;
    return {sf_base, c->synth_eps_scale, c->d_sync, c->opt[MP3S_OPT_FAST_IMDCT] != 0, c->opt[MP3S_OPT_FLOAT_FAST] != 0, c->opt[MP3S_OPT_FUSED_DECODE] != 0,
            done, c->guard_probe.x ? &c->guard_probe : nullptr};
}

int local_world_size();   // mp3s_hostinfo.cpp: LOCAL_WORLD_SIZE of the launcher (1 without one)

class PinnedBlock {
public:
    PinnedBlock() = default;
    PinnedBlock(const PinnedBlock &) = delete;
    PinnedBlock &operator=(const PinnedBlock &) = delete;
    ~PinnedBlock() { release(); }
    bool reserve(size_t bytes)
    {
        if (bytes <= cap_) return true;
        release();
        if (bytes > kMaxPinned) {   // hours of audio in one call: pinning gigabytes costs seconds, ordinary memory then
            p_ = (uint8_t *)std::malloc(bytes);
            if (!p_) return false;
            cap_ = bytes; pinned_ = false;
            return true;
        }
        pinned_ = true;
        {
            std::lock_guard<std::mutex> g(mu());
            auto &fl = free_list();
            size_t best = fl.size();
            // best fit, but a small request does not take a large block away from the next large request (which would
            // then have to pin fresh pages: about a millisecond per 4 MB)
            const size_t too_big = std::max(4 * bytes, bytes + ((size_t)1 << 20));
            for (size_t i = 0; i < fl.size(); i++)
                if (fl[i].second >= bytes && fl[i].second <= too_big && (best == fl.size() || fl[i].second < fl[best].second)) best = i;
            if (best < fl.size()) { p_ = fl[best].first; cap_ = fl[best].second; fl.erase(fl.begin() + best); return true; }
        }
        const size_t want = bytes + bytes / 8 + (1 << 16);
        void *q = nullptr;
        if (hipHostMalloc(&q, want, hipHostMallocDefault) != hipSuccess) return false;
        p_ = (uint8_t *)q; cap_ = want;
        return true;
    }
    uint8_t *data() const { return p_; }
    // what the process keeps pooled right now, and the cap (mp3s_ctx_host_share)
    static void pool_state(size_t *held, size_t *cap)
    {
        std::lock_guard<std::mutex> g(mu());
        size_t h = 0;
        for (auto &e : free_list()) h += e.second;
        *held = h; *cap = pool_cap();
    }

private:
    void release()
    {
        if (!p_) return;
        if (!pinned_) { std::free(p_); p_ = nullptr; cap_ = 0; return; }
        std::lock_guard<std::mutex> g(mu());
        auto &fl = free_list();
        size_t held = 0;
        for (auto &e : fl) held += e.second;
        if (fl.size() < 48 && held + cap_ <= pool_cap()) fl.emplace_back(p_, cap_);
        else hipHostFree(p_);
        p_ = nullptr; cap_ = 0;
    }
    static std::mutex &mu() { static std::mutex *m = new std::mutex(); return *m; }
    static std::vector<std::pair<uint8_t *, size_t>> &free_list()
    {
        static auto *v = new std::vector<std::pair<uint8_t *, size_t>>();
        return *v;
    }
    static constexpr size_t kMaxPinned = (size_t)4 << 30;   // (a 100 000-frame file decodes to 460 MB of PCM: two such results and the MP3 results beside them stay pooled)
    // what stays pooled between calls: the ranks of one host share its page-locked memory (memlock / cgroup limits), so eight ranks
    // keep 1 GB each where a lone process keeps 4; a block that does not fit goes back to the system when it is released
    static size_t pool_cap()
    {
        static const size_t cap = std::max<size_t>((size_t)1 << 30, kMaxPinned / (size_t)local_world_size());
        return cap;
    }
    uint8_t *p_ = nullptr;
    size_t cap_ = 0;
    bool pinned_ = true;
};

struct mp3s_multi {     // owner payload of mp3s_decode_streams
    std::vector<std::pair<const uint8_t *, size_t>> files;   // borrowed for the duration of the call
    std::vector<ParsedStream> parsed;
    std::vector<ScannedStream> scanned;
    PinnedBlock arena[3];                 // PCM of all mono / all stereo streams, index = channel count
    size_t head_room = 0;                 // bytes kept free in front of the PCM (mp3s_decode_file puts the WAV header there)
    std::vector<const uint8_t *> pcm;     // per stream, into its arena
    // blocks of a stream: only frames [first, first + count) of stream i are kept after parsing (absent: all of them);
    // keep_dup = the frame the reference repeats after a bad header (D12) still belongs to a window that ends the stream
    struct Window { long first, count; bool keep_dup; };
    std::vector<Window> window;
    std::vector<std::vector<uint8_t>> all_bits;   // ... and the stego bits of the whole stream
    // an index of the (single) stream: its window is scanned on its own, from the resume point in front of it, instead of
    // the whole file (then all_bits holds the bits of the window's frames only)
    const StreamIndex *index = nullptr;
};

struct mp3s_buf {
    std::shared_ptr<mp3s_multi> multi;
    ParsedStream parsed;
    ScannedStream scanned;
    std::vector<uint8_t> bytes;      // generic payload (pcm / mp3)
    std::vector<uint8_t> bits;
    std::vector<FrameRef> refs;      // mp3s_walk_stream: the frames (their table counts in bits)
    std::vector<int32_t> scfsi;
    std::vector<std::unique_ptr<mp3s_buf>> parts;   // results of the batches of a multi-file call
    std::vector<std::vector<uint8_t>> lists;        // mp3s_reveal_messages: per file its text and its stego bits
    // encoder results: MP3 bytes and GrInfo records land in page-locked blocks and are handed out from there
    PinnedBlock big[3];              // MP3 bytes, GrInfo records, the small results (verdict, per-stream chain ends)
    uint8_t *mp3 = nullptr;
    mp3s_gr_out *gr_out = nullptr;
};

// a result owner with the batch record of ONE borrowed stream (the block calls): b.multi made, stream 0 = (file, len), nothing parsed yet
inline mp3s_multi &one_stream_multi(mp3s_buf &b, const uint8_t *file, size_t len)
{
    b.multi.reset(new mp3s_multi());
    mp3s_multi &m = *b.multi;
    m.parsed.resize(1); m.scanned.resize(1); m.pcm.assign(1, nullptr); m.files.assign(1, {file, len});
    return m;
}

// MP3S_TRACE=1: phase timings of the file pipelines on stderr
inline bool trace_on() { static const bool on = getenv("MP3S_TRACE") != nullptr; return on; }
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// (mp3s_*_fd) pwrite until the n bytes of `src` stand in the file from `at` on, or a write fails: the bytes written.  A count below n is for the
// caller to react to; errno is the failed write's.
inline size_t pwrite_all(int fd, const uint8_t *src, size_t n, size_t at)
{
    size_t done = 0;
    while (done < n) {
        const ssize_t w = pwrite(fd, src + done, n - done, (off_t)(at + done));
        if (w <= 0) break;
        done += (size_t)w;
    }
    return done;
}
// (mp3s_*_fd) arm the context's sink: the result goes to fd, behind `base` bytes the caller writes itself (the WAV header's place); nothing is
// written yet.  Chunks go to the file before the call has succeeded only if it is empty now.
inline void sink_begin(mp3s_ctx *c, int fd, size_t base)
{
    struct stat st;
    c->sink_fd = fd; c->sink_done = 0; c->sink_base = base; c->sink_early = fstat(fd, &st) == 0 && st.st_size == 0;
}

// ---------------------------------------------------------------- the frame of the list-of-files calls (file_lists.cpp)
// mp3s_decode_streams, mp3s_hide_messages, mp3s_encode_files, mp3s_reveal_messages and mp3s_pipe_collect answer per file by ONE
// rule, made of the pieces below: out[i] zeroed, a code and a text per file, front ends on a few host threads, one device batch
// per group of files, a failed batch run again file by file, the codes into status[] -- or, without one, the first failing
// file's code as the call's -- and that file's text into mp3s_last_error().

// x rounded up to a multiple of 16: where every part of a host-made block and every file of a device image begins
inline size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }

// Host threads for the front ends of n files of total_bytes, at most max_threads: small lists (by bytes) stay on the calling
// thread -- starting a thread costs about what scanning 100 KB does.  host_threads16(): the max_threads of the calls that have
// no context option to ask (MP3S_OPT_SCAN_THREADS: default_scan_threads).
inline int file_workers(int n, size_t total_bytes, int max_threads)
{
    return (int)std::min<size_t>({(size_t)n, (size_t)max_threads, total_bytes / (256u << 10) + 1});
}
inline int host_threads16() { const unsigned hw = std::thread::hardware_concurrency(); return (int)std::min(hw ? hw : 1u, 16u); }
// f(worker, i) for i in [0, n) on `workers` threads, the calling one (worker 0) included: the front ends of the files of a list
// are independent.  The files are handed out one by one, in order; f(w, ...) runs on one thread at a time for every w.
template <class F>
void parallel_files(int workers, int n, F f)
{
    if (workers <= 1) {
        for (int i = 0; i < n; i++) f(0, i);
        return;
    }
    std::atomic<int> next{0};
    auto run = [&](int w) { for (int i; (i = next.fetch_add(1)) < n;) f(w, i); };
    std::vector<std::thread> pool;
    for (int w = 1; w < workers; w++) pool.emplace_back(run, w);
    run(0);
    for (auto &t : pool) t.join();
}

// A whole file through the FrameWalker: open, walk to the end into refs (which grows; refs.size() >= the count afterwards), with
// `tables` ([frames][4], grown beside refs) the code-book counts for as long as tables_wanted says.  Returns the frame count, or
// -1 when the file is not for the walk; the walker, which stays with the caller for what else it knows of the stream, tells why:
// irregular, or ended without a frame, or neither -- open() failed, and w.error is its code.
long walk_whole(const uint8_t *file, size_t len, std::vector<FrameRef> &refs, FrameWalker &w, std::vector<uint8_t> *tables = nullptr,
                long tables_wanted = 0);

// out = stream `seg` of a finished encode batch whose bytes lie at mp3_base: the ONE place an EncSeg becomes an mp3s_file.  The
// caller says how many message bits the stream took (the host's count, or the device's cursor).
struct EncSeg;
void file_from_seg(const EncSeg &seg, const uint8_t *mp3_base, int kbps, int rate, int64_t hide_offset, mp3s_file *out);

// The files of a list by a pair of keys ((sampling rate, kbps)), groups and members in arrival order: a group is one device batch,
// and the order of the batches decides where the results lie in the owner.
struct FileGroups {
    struct Group { int a, b; std::vector<int> idx; };
    std::vector<Group> groups;
    void add(int a, int b, int i)
    {
        size_t g = 0;
        while (g < groups.size() && (groups[g].a != a || groups[g].b != b)) g++;
        if (g == groups.size()) groups.push_back({a, b, {}});
        groups[g].idx.push_back(i);
    }
};

// Code and text per file of a list call.  Whoever finds a file failing records both at that moment: set(i, code) keeps what
// mp3s_last_error() says then (the text of the fail() that made the code) -- on the calling thread, that is: a front end on
// another thread leaves its code in st[i] and the caller composes the text after the join (front_end_failed for the two texts
// hide and reveal share).
struct FileStatus {
    std::vector<int32_t> st;
    std::vector<std::string> why;
    explicit FileStatus(int n) : st((size_t)n, MP3S_OK), why((size_t)n) {}
    void set(int i, int code) { st[(size_t)i] = code; if (code) why[(size_t)i] = mp3s_last_error(); }
};
int front_end_failed(int code, int i);   // fail(code, "file %d: null pointer" for MP3S_E_ARG, "file %d: malformed or unsupported MP3 stream" otherwise)
// The tail of every list call: the codes into status[] (when given) and the FIRST failing file's text into mp3s_last_error().
// Returns that file's code (MP3S_OK: none failed), which fails the call when status == NULL.
int finish_files(const FileStatus &fs, int32_t *status);
// ... and the call's end behind it: the first failing file's code when there is no status[], else the results' owner to the caller
int finish_list(const FileStatus &fs, int32_t *status, std::unique_ptr<mp3s_buf> &top, mp3s_buf **owner);

// The front of the calls that take a list of MP3 files: m sized for n_files, file i = file_of(i) borrowed into m.files (a null pointer:
// MP3S_E_ARG, the file is not looked at), the context's spare scan lent to a list of one, front_end(m, i) of every file on the host
// threads.  Returns the per-file codes; their texts are the caller's.  mp3_list_done, after the last use of m.files and m.scanned:
// the borrowed pointers dropped, the spare scan handed back.
struct mp3s_multi;
std::vector<int32_t> mp3_list_front(mp3s_ctx *c, mp3s_multi &m, int n_files, const std::function<std::pair<const uint8_t *, size_t>(int)> &file_of);
void mp3_list_done(mp3s_ctx *c, mp3s_multi &m);
// ... of the re-encoding calls (mp3s_hide_messages, mp3s_capacity_files), where a message without bytes but with a length is a null
// file too: then per file the front end's text or the reference's checks (reencode_check), its framed message into bits[i], its
// (sampling rate, kbps) group.  *t_scanned (when given): now_ms() between the front ends and the rest
void reencode_list_front(mp3s_ctx *c, mp3s_multi &m, const uint8_t *const *mp3s, const size_t *lens, int n_files, const uint8_t *const *msgs,
                         const size_t *msg_lens, FileStatus &fs, std::vector<std::vector<uint8_t>> &bits, FileGroups &groups, double *t_scanned = nullptr);

// run(a, b, idx) -> code, for every group in order.  One file spoils its batch (main data the host parser rejects, a quantizer
// step that leaves the table ...): a failed group of one fails its file, a larger one is run again file by file, run(a, b, {i}),
// to name the file -- fs gets each file's code and text.  after_failure() runs between a failed batch and what follows it (the
// caller that has copies in flight from its callers' bytes waits for them there).
template <class Run, class After>
void run_groups(const FileGroups &groups, Run run, FileStatus &fs, After after_failure)
{
    for (const FileGroups::Group &g : groups.groups) {
        const int rc = run(g.a, g.b, g.idx);
        if (!rc) continue;
        if (g.idx.size() == 1) fs.set(g.idx[0], rc);
        after_failure();
        if (g.idx.size() > 1)
            for (int i : g.idx) fs.set(i, run(g.a, g.b, std::vector<int>{i}));
    }
}

// ---------------------------------------------------------------- decode pipeline (mp3s_decode_pipeline.cpp)
constexpr int kDecodeChunk = 16384;   // frames per decode launch group (scratch ~0.6 GB); chunks overlap by a 1-frame halo
inline size_t pcm_elem(int fmt) { return fmt == MP3S_PCM_I16 ? 2 : (fmt == MP3S_PCM_F32 ? 4 : 8); }
int max_part2_3(const mp3s_frame_side *side, long n);
// keep frames [first, first + count) of a parsed stream (its main data, side records, samples)
void cut_window(ParsedStream &p, ScannedStream &sc, long first, long count);
// host front end of stream i of m (scan; full host parse where the device cannot decode), cut to the stream's window
int front_end(mp3s_multi &m, int i);
int decode_transform_chunk(mp3s_ctx *c, const int16_t *d_is, const mp3s_granule_si *d_si, const mp3s_frame_hdr *d_hdr, long first, int cnt,
                           int nch, int halo, int out_format, void *d_pcm, hipStream_t stream = nullptr /* null: the context's */,
                           hipEvent_t done = nullptr /* recorded behind the chunk's transforms (launch_decode) */);
// The front half of a decode batch, for decode_group and the table audit (mp3s_table_audit_files.cpp) alike: the streams `idx` of m (one
// channel count) laid end to end -- frame headers into the context's h_hdr, side records, main data --, uploaded, launch_huffman, the
// frames the kernel flags decided by the host parser, host-parsed streams placed.  Afterwards d_is / d_si hold every frame's samples
// and granule records; d_side holds the side records of the device-decoded streams and zeros for streams that were host-parsed when
// the call began.  Pool buffers kPoolIs0 .. kPoolSideInfo; d_pcm gets room for a chunk of frames of frame_bytes each (0: none is wanted).  n == 0: nothing
// was done.  d_is == nullptr behind a failure: it happened in front of the allocations.
struct DecodeFront {
    long n = 0;                       // frames of the batch
    std::vector<long> first_of;       // per stream of idx: its first frame in the batch
    void *d_is = nullptr, *d_si = nullptr, *d_hdr = nullptr, *d_pcm = nullptr, *d_st = nullptr, *d_blob = nullptr, *d_side = nullptr;
};
int decode_front(mp3s_ctx *c, mp3s_multi &m, const std::vector<int> &idx, int nch, size_t frame_bytes, DecodeFront &F);
// decode the streams `idx` of m (one channel count) as one batch; d_keep: int16 PCM stays on the device there
int decode_group(mp3s_ctx *c, mp3s_multi &m, const std::vector<int> &idx, int nch, int out_format, void *d_keep = nullptr);

// ---------------------------------------------------------------- pairs of MP3 files compared on the device (pcm_pairs.cpp)
// frames of a stream's PCM, the frame the decoder repeats after a bad header (D12) included: what mp3s_decoded.n_rows counts, / 1152
inline int64_t pcm_frames(const ParsedStream &p) { return (int64_t)p.n_frames + (p.dup_last_frame ? 1 : 0); }
// out = a pair's record and what the host knows of its two streams: the ONE place a mp3s_pcm_pair_diff becomes an mp3s_pcm_distortion
// (n_frames records of n_samples compared samples in all)
void distortion_from_record(const mp3s_pcm_pair_diff &r, const ParsedStream &a, const ParsedStream &b, int64_t n_frames, int64_t n_samples,
                            const mp3s_pcm_frame_diff *profile, mp3s_pcm_distortion *out);
// The pairs `idx` (file idx[k] against file n_pairs + idx[k] of m, one channel count, every stream with a frame) as one batch.
//   lay : the streams A, B of pair idx[0], A, B of pair idx[1], ... and where each lies in the PCM buffer (decode_group: frames back to
//         back, a repeated last frame behind its stream); max_frames: what the caller's kernels can address.
//   run : kPoolPcm0 (the PCM), kPoolInputs (in_bytes of `in`, made by the caller from the layout: the context's h_in) and kPoolSmall (res_bytes), the
//         decode, a check that it left the layout's frame counts, the upload, launch(d_pcm, d_in, d_res) -> code (its own text),
//         down_bytes of the results into part->big[2] = res, and the stream synchronised whatever happened.
struct PcmPairBatch {
    std::vector<int> streams;
    std::vector<int64_t> first, frames_a, frames_b;   // per pair: the first frame of A in the buffer (B follows), the frames of A and of B
    std::vector<int64_t> out_first;                   // ... and the whole frames both have (min) of the pairs in front: where its records begin
    int64_t rows_frames = 0, cmp_frames = 0;          // the sums: frames of the PCM buffer, frame records
    std::unique_ptr<mp3s_buf> part;
    const uint8_t *res = nullptr;
    int lay(const mp3s_multi &m, int n_pairs, const std::vector<int> &idx, int64_t max_frames);
    int run(mp3s_ctx *c, mp3s_multi &m, int nch, const uint8_t *in, size_t in_bytes, size_t res_bytes, size_t down_bytes,
            const std::function<int(const int16_t *d_pcm, const uint8_t *d_in, uint8_t *d_res)> &launch);
private:
    int n_pairs = 0;
    const std::vector<int> *idx = nullptr;
};
// The shell of the pair-list calls behind their own argument checks: all 2 n files as one list (file i = a[i], file n + i = b[i])
// through the MP3 list front, out[0 .. n_pairs) (elements of out_size bytes) zeroed, per pair its code and text ("pair %d: ..."), or
// empty(m, i) (a stream without a frame: nothing for a decode batch; it fills out[i]), or its channel count's group; refuse(m, fs, i)
// (may be empty) is asked first in both cases and sets the pair's code when it says true.  group(m, idx, nch, top) -> code runs a
// batch and keeps what its results point into in a part of top; the out[] of a failed batch is zeroed again.
int pcm_pairs_call(mp3s_ctx *c, const uint8_t *const *a, const size_t *a_lens, const uint8_t *const *b, const size_t *b_lens, int n_pairs, void *out,
                   size_t out_size, mp3s_buf **owner, int32_t *status, const std::function<void(const mp3s_multi &m, int i)> &empty,
                   const std::function<bool(const mp3s_multi &m, FileStatus &fs, int i)> &refuse,
                   const std::function<int(mp3s_multi &m, const std::vector<int> &idx, int nch, mp3s_buf *top)> &group);
// The host block of a _dev test aid (the context's h_pcm_tiles / h_pcm_align) travels on the stream behind the call: the block of the
// call before may still be on its way, and its copy reads the vector that is written next.  Waits for ev_pcm_tiles (made on first
// use), runs fill_and_copy() -> code, records the event behind its copy.
int pcm_dev_host_block(mp3s_ctx *c, const std::function<int()> &fill_and_copy);

// ---------------------------------------------------------------- encode pipeline (mp3s_encode_pipeline.cpp)
constexpr int kLongMessageBits = 1024;    // above: the first pass does not guess cursors at all
constexpr int32_t kNoCursor = MP3S_NO_CURSOR; // "behind every message": such a unit hides nothing
constexpr int kPatternBytes = 32;         // the eight 3-bit patterns, 4 bytes apart, in front of the messages
constexpr int kVariantEntries = 65536;    // (unit, pattern) entries per variant launch
constexpr size_t kFewUnits = 8;           // that few wrong cursors after the first pass: re-run them directly

struct EncSeg {             // one stream of an encode batch: frames back to back in the batch's PCM
    int n_frames = 0;
    const uint8_t *hide = nullptr;   // 0/1 bytes
    int n_hide = 0;
    // a block of a longer stream (mp3s_encode_block; only as the single stream of a batch)
    int lead = 0;                    // frames of PCM in front of the block: transformed for their state, then dropped
    int64_t first_frame = 0;         // index of the block's first frame in its stream (padding recurrence)
    bool last = true;                // the stream ends with this block (the reference drops the cached tail there: E14)
    const mp3s_carry *carry_in = nullptr;
    // The first pass of the rate loop runs every unit on a GUESSED message cursor: the tables the units in front of it will
    // take.  Without better knowledge that is three per unit.  A stream that is being re-encoded brings better knowledge:
    // the non-zero table indices of the SAME audio in the stream it was decoded from (side info of the input, unit order
    // frame / channel / granule; silence has none).  n_frames * 4 entries, or null.
    const uint8_t *tables_guess = nullptr;
    int n_guess = -1;                // units tables_guess covers (-1: all n_frames * 4); behind them the guess is 3 per unit
    int any_silent = -1;             // 1 / 0: some / no unit of the stream is without tables; -1: look into tables_guess
    // filled by encode_batch
    int first = 0, hide_base = 0;
    int reach = 0, first_entry = 0;  // the message cursor is decided on the device over the stream's first `reach` units (0: guessed)
    int64_t hide_offset = 0;         // message bits consumed (from the start of the stream)
    size_t mp3_off = 0, mp3_len = 0; // the stream's bytes inside the batch's output
    mp3s_carry carry_out = {};
    bool carry_used = false;         // the block's bytes depend on carry_in
};
// message bits the frames in front of a block have taken
inline int64_t cursor0(const EncSeg &s)
{
    return s.carry_in ? std::min<int64_t>(std::max<int64_t>(s.carry_in->cursor, 0), kNoCursor) : 0;
}
// The host-made inputs of an encode batch travel as ONE block (one copy):
//   [frame headers (n_all) | rate frames (n) | assumed cursors (units) | message bits | chain segments | frame offsets (n+1) | padding (n)
//    | selection spans (n_segs) | variant entries: units (n_entries), cursors (n_entries)]
struct EncLayout {
    int n = 0, n_all = 0, lead = 0, units = 0, n_hide = 0, n_segs = 0;
    int n_entries = 0, max_reach = 0;   // message variants run inside the first rate-loop launch (mp3s_rate_select_dev)
    bool redo = true;              // the chain check is issued with the device's re-runs behind it (launch_chain's `redo`)
    int sri = 0, bri = 0, whole = 0, samplerate = 0, kbps = 0;
    size_t o_rf = 0, o_cur = 0, o_hide = 0, o_segs = 0, o_off = 0, o_pad = 0, o_spans = 0, o_ent = 0, bytes = 0;   // (headers at offset 0)
    size_t mp3_bytes = 0;          // all frames of the batch
    int64_t bytes_before = 0;      // size of the frames in front of a block (E14: the tail cut depends on it)
};
// The parts of such a block at `base`, typed: B = uint8_t for enc_fill, which writes them, const uint8_t for everybody who reads them -- on the
// host (the copy enc_fill wrote) or as device addresses (EncDev::d_in).  hide = [patterns | message of stream 0 | message of stream 1 ...]
template <class B, class T> using BlockPart = typename std::conditional<std::is_const<B>::value, const T, T>::type;
template <class B>
struct EncBlock {
    BlockPart<B, mp3s_frame_hdr> *hdr; BlockPart<B, mp3s_rate_frame> *rf; BlockPart<B, int32_t> *cursor; B *hide; BlockPart<B, mp3s_chain_seg> *segs;
    BlockPart<B, uint32_t> *off; B *pad; BlockPart<B, mp3s_select_span> *spans; BlockPart<B, int32_t> *ent_unit, *ent_cursor;
};
template <class B>
inline EncBlock<B> enc_block(const EncLayout &L, B *base)
{
    BlockPart<B, int32_t> *const ent = (BlockPart<B, int32_t> *)(base + L.o_ent);
    return {(BlockPart<B, mp3s_frame_hdr> *)base, (BlockPart<B, mp3s_rate_frame> *)(base + L.o_rf), (BlockPart<B, int32_t> *)(base + L.o_cur), base + L.o_hide,
            (BlockPart<B, mp3s_chain_seg> *)(base + L.o_segs), (BlockPart<B, uint32_t> *)(base + L.o_off), base + L.o_pad, (BlockPart<B, mp3s_select_span> *)(base + L.o_spans),
            ent, ent + L.n_entries};
}
// small results of a batch, in one block: this head, then mp3s_chain_seg_out[n_segs].  Every word is zero when all went well; the kernels
// that own a word write or OR into it, the host only reads.
struct SmallHead {
    int32_t redo_units, step_range;                      // the chain check's verdict (mp3s_chain_resolve_dev: d_verdict[0], [1])
    int32_t pack_status, huffman_status, parse_status;   // the bit packer's, the Huffman decode's, the device-side parse's (MP3S_PS_*)
    int32_t spare[3];
    bool chains_settled() const { return redo_units == 0 && step_range == 0; }
    bool pack_clean() const { return pack_status == 0; }
    bool huffman_clean() const { return huffman_status == 0; }
    bool parse_clean() const { return (parse_status & kParseMismatch) == 0; }
    bool inherits_across_frames() const { return (parse_status & kParseInherits) != 0; }
    // final after the first pass: a decode job, a hide / clear / encode job (walked: the job's frames were parsed on the device)
    bool decode_final(bool walked) const { return (!walked || parse_clean()) && huffman_clean(); }
    bool encode_final(bool walked) const { return (!walked || parse_clean()) && chains_settled() && pack_clean() && huffman_clean(); }
    // only the cursor / address guesses failed: the host can resolve the chains on the job's own device buffers
    bool resolvable(bool walked) const { return (!walked || parse_clean()) && redo_units != 0 && step_range == 0 && huffman_clean(); }
    bool all_clean() const { return chains_settled() && pack_clean() && huffman_clean() && parse_clean(); }   // no word says anything, whatever the job is
};
static_assert(sizeof(SmallHead) == 32 && offsetof(SmallHead, redo_units) == 0 && offsetof(SmallHead, step_range) == 4 && offsetof(SmallHead, pack_status) == 8 &&
              offsetof(SmallHead, huffman_status) == 12 && offsetof(SmallHead, parse_status) == 16 && offsetof(SmallHead, spare) == 20, "the kernels are handed these words' addresses");
inline size_t small_bytes(int n_segs) { return sizeof(SmallHead) + (size_t)n_segs * sizeof(mp3s_chain_seg_out); }
inline mp3s_chain_seg_out *small_seg_out(SmallHead *head) { return reinterpret_cast<mp3s_chain_seg_out *>(head + 1); }   // (on the device: for the launchers)
struct SmallView {   // a block that has come down
    const uint8_t *block;
    const SmallHead &head() const { return *reinterpret_cast<const SmallHead *>(block); }
    const mp3s_chain_seg_out &seg_out(size_t i) const { return reinterpret_cast<const mp3s_chain_seg_out *>(block + sizeof(SmallHead))[i]; }
};
// How stream i of a batch ended: from the stream's record when the host resolved the chains (enc_resolve filled it), from the device's otherwise
struct SegEnd { mp3s_carry out; bool carry_used; int64_t hide_offset; };
inline SegEnd seg_end(const EncSeg &sg, const mp3s_chain_seg_out &so, bool resolved)
{
    if (resolved) return {sg.carry_out, sg.carry_used, sg.hide_offset};
    SegEnd e = {{so.cursor - sg.hide_base, {}}, so.carry_used != 0, so.cursor - sg.hide_base};
    std::memcpy(e.out.chain, so.chain, sizeof e.out.chain);
    return e;
}
// checks the streams and fills first / hide_base of each
int enc_layout(std::vector<EncSeg> &segs, int samplerate, int bitrate_kbps, EncLayout &L, bool select = true /* MP3S_OPT_SELECT */);
// writes the block (L.bytes at dst); *mp3_off_len: per stream {offset, length} of its bytes in the batch's output
int enc_fill(std::vector<EncSeg> &segs, EncLayout &L, uint8_t *dst);
struct EncDev {
    const int16_t *d_pcm = nullptr;      // [n_all][1152][2]
    const uint8_t *d_in = nullptr;       // the block above
    int32_t *d_mdct_all = nullptr;       // [n_all][2][2][576]
    int16_t *d_ix = nullptr; mp3s_gr_out *d_out = nullptr; int32_t *d_en = nullptr;
    void *d_agg = nullptr;               // chain_agg_bytes(n)
    uint8_t *d_mp3 = nullptr; int32_t *d_sc = nullptr;
    SmallHead *d_small = nullptr;        // small_bytes(n_segs)
    bool direct_status = false;          // d_small's status words were zeroed with the job's inputs: the kernels OR into them directly
    // the bit packer in two launches, frames [0, pack_split) and the rest, pack_half recorded between them (the last chunk of a
    // one-file call: its first half comes down while the second is packed); 0: one launch
    int pack_split = 0; hipEvent_t pack_half = nullptr;
    // results of the variant entries (L.n_entries of them; read by the selection right behind the rate loop)
    int16_t *d_ixv = nullptr; mp3s_gr_out *d_outv = nullptr; int32_t *d_env = nullptr;
    // a job without its tail (capacity_batch): with d_cap set the job ends behind the chain check -- k_capacity writes the streams' records
    // there (and the per-frame profile, when d_profile is given) and the bit packer is not launched: d_mp3, d_sc and the pack fields are unused
    mp3s_capacity_seg *d_cap = nullptr; uint32_t *d_profile = nullptr;
};
// d_mdct_all | d_ix | d_out | d_en (a multiple of 256 bytes) | d_sc of a batch in ONE allocation (a slot of a pipe): where each begins, the end
struct EncScratch { size_t o_mdct, o_ix, o_out, o_en, o_sc, bytes; };
inline EncScratch enc_scratch_layout(const EncLayout &L)
{
    const size_t o_ix = (size_t)L.n_all * 2304 * 4, o_out = o_ix + (size_t)L.n * 2304 * 2, o_en = o_out + (size_t)L.units * sizeof(mp3s_gr_out),
                 o_sc = o_en + (((size_t)L.units * 22 * 4 + 255) & ~(size_t)255);
    return {0, o_ix, o_out, o_en, o_sc, o_sc + (size_t)L.n * 8 * 4};
}
// the entries of a stream's first `reach` units (variant-major, the two "bits left" rows from MP3S_SELECT_TAIL_FIRST on: mp3s.h)
void select_entries(int first_unit, int reach, int first_entry, int hide_end, int64_t bits_left, int32_t *ent_unit, int32_t *ent_cursor);
// device buffers for L.n_entries variant entries from the context's pool (kPoolVarIx, kPoolVarOut, kPoolVarEnergy: the host's variants', free at that point)
bool enc_variant_buffers(mp3s_ctx *c, const EncLayout &L, EncDev &d);
// The device steps of an encode (mp3s_api.cpp), each queued on the stream its caller names, nothing waited for; MP3S_OK, or the code and text
// of the entry point of the same name (mp3s_*_dev), which is the step on the context's stream behind its argument checks.
int encode_transform_step(mp3s_ctx *c, hipStream_t stream, const int16_t *d_pcm, const mp3s_frame_hdr *d_hdr, int n_frames, int32_t *d_mdct);
// the variant entries of a rate loop and of the selection behind it, from the arrays the entry points take (the table counts lie behind the records)
inline RateVariantArgs variant_args(const int32_t *d_ent_unit, const int32_t *d_ent_cursor, int n_entries, int16_t *d_ixv, mp3s_gr_out *d_outv, int32_t *d_env)
{
    return {d_ent_unit, d_ent_cursor, n_entries, d_ixv, d_outv, d_env, (uint8_t *)(d_outv + n_entries)};
}
// the completion event of a rate loop whose caller has none of its own (MP3S_OPT_RATE_SIGNALS: the dispatch signals ev_order, mp3s_ctx_wait_last)
inline hipEvent_t rate_signal_default(const mp3s_ctx *c) { return c->opt[MP3S_OPT_RATE_SIGNALS] ? c->ev_order : nullptr; }
// done (may be null): the dispatch's own completion signal, no record packet.  With variants the launch writes the context's variant buffers: it waits for a selection that read them on another stream (sel_pending)
int rate_step(mp3s_ctx *c, hipStream_t stream, hipEvent_t done, const int32_t *d_mdct, const mp3s_rate_frame *d_frames, int n_frames, const uint8_t *d_hide,
              int n_hide, const int32_t *d_cursor, const int32_t *d_state, const int32_t *d_list, int n_list, int16_t *d_ix, mp3s_gr_out *d_out, int32_t *d_en,
              const RateVariantArgs *variants = nullptr);
// on another stream than the context's the step records ev_sel behind itself and sets sel_pending, for the next rate_step with variants
int select_step(mp3s_ctx *c, hipStream_t stream, const uint8_t *d_hide, int32_t *d_cursor, const mp3s_chain_seg *d_segs, const mp3s_select_span *d_spans,
                int n_segs, int max_reach, const RateVariantArgs &va, int16_t *d_ix, mp3s_gr_out *d_out, int32_t *d_en);
// the packer in one launch, through the context's sync words (one launch at a time)
int pack_step(mp3s_ctx *c, hipStream_t stream, const int16_t *d_ix, const mp3s_gr_out *d_gr, const int32_t *d_en, int n_frames, int sri, int bri, int whole,
              const uint32_t *d_frame_off, const uint8_t *d_padding, uint8_t *d_mp3, int32_t *d_scfsi, int32_t *d_status);
// transforms -> rate loop on the guessed cursors, on c->stream; selection -> chain check -> bit packing (with d.d_cap: k_capacity in its place) on `tail`, or on
// c->stream without one; nothing waited for.  The packed bytes (the capacity records) are final iff d_small->chains_settled().
int enc_issue(mp3s_ctx *c, const EncLayout &L, const EncDev &d, hipStream_t tail = nullptr /* ordered behind the rate loop through tail_from */,
              hipEvent_t tail_from = nullptr, hipEvent_t pcm_read = nullptr /* recorded behind the encode transforms: the PCM they read may be overwritten */);
// verdict != 0: the host resolves the chains on the first pass's device buffers (walk, message variants, exact re-runs,
// packing again); `in` = the host copy of the block.  Pool buffers of its own: kPoolRedo, kPoolVarEntries .. kPoolVarPairs.
int enc_resolve(mp3s_ctx *c, const EncLayout &L, std::vector<EncSeg> &segs, const uint8_t *in, const EncDev &d, mp3s_buf *b, bool have_gr,
                int *passes_out);
int encode_batch(mp3s_ctx *c, const int16_t *pcm, const int16_t *pcm_dev, std::vector<EncSeg> &segs, int samplerate, int bitrate_kbps,
                 mp3s_buf *b, int *passes_out, bool want_gr = true);
// encode_batch without its tail: the same inputs, transforms, rate loop (message variants, selection) and chain check with the device's
// re-runs, then k_capacity instead of the bit packer.  No MP3 buffer on either side; ONE copy brings down [verdict and chain ends |
// capacity records | profile (want_profile)] into b->big[2].  out.counted: the verdict was 0 -- out.seg[k] is stream k's record,
// out.profile the batch's profile (stream k's part begins at segs[k].first; null without want_profile), both inside b, and every
// segs[k].hide_offset is what encode_batch gives.  Not counted: the guesses did not hold and nothing else of `out` means anything -- the
// caller runs the batch through encode_batch (want_gr) and counts from the host copy of the records; the PCM is still where it was.
struct CapacityBatch { bool counted = false; const mp3s_capacity_seg *seg = nullptr; const uint32_t *profile = nullptr; size_t down_bytes = 0; };
int capacity_batch(mp3s_ctx *c, const int16_t *pcm_dev, std::vector<EncSeg> &segs, int samplerate, int bitrate_kbps, bool want_profile,
                   mp3s_buf *b, CapacityBatch *out);
// what the reference's WAV reader / encoder would say to the WAV its decoder writes for this stream: MP3S_OK with *kbps_out, or the code
// and text mp3s_hide_message / mp3s_clear_file fail with
int reencode_check(const ParsedStream &p, int *kbps_out);
// the front half of a re-encode batch: the streams `idx` of m (stereo, one sampling rate and bitrate) become segs (bits[i] = framed
// message of file i, empty: nothing hidden; guess keeps the table counts segs point into) and are decoded on the device into
// *d_keep_out, int16 PCM that stays in HBM (kPoolPcm0), *rows_frames frames back to back
int reencode_decode(mp3s_ctx *c, mp3s_multi &m, const std::vector<int> &idx, const std::vector<std::vector<uint8_t>> &bits,
                    std::vector<EncSeg> &segs, std::vector<std::vector<uint8_t>> &guess, void **d_keep_out, int64_t *rows_frames);
// non-zero table indices per unit of a scanned stream, in the encoder's unit order (frame, channel, granule): see
// EncSeg::tables_guess; `extra` more frames (the repeated last frame of a stream that ends in a bad header) repeat the last
// mp3s_select_plan with a lower limit for each stream's reach (nullptr: none)
int select_plan(const mp3s_chain_seg *segs, int n_segs, mp3s_select_span *spans, int32_t *ent_unit, int32_t *ent_cursor, int cap,
                const int32_t *min_reach);
void tables_guess_of(const mp3s_frame_side *side, long n_frames, int extra, std::vector<uint8_t> &out);

// ---------------------------------------------------------------- WAV files as device batches (mp3s_encode_files.cpp)
// what mp3s_encode_file checks of a file before the device sees it, in its order (header, frame count, message arguments);
// MP3S_OK with *w and *count (frames), or the code and text the one-file call fails with
int wav_encode_check(const uint8_t *wav, size_t len, int bitrate_kbps, const uint8_t *hide_bits, int n_hide, mp3s_wav_info *w, int64_t *count);
// ... and what the device is told about the file: by the reference's reader (import false: wav_encode_check; always for k_wav_gather)
// or by the rules of MP3S_OPT_WAV_IMPORT (wav_import_parse; k_wav_gather for 16-bit stereo of whole frames, k_wav_import otherwise)
struct WavPlan {
    int samplerate = 0, format = 0, channels = 0;
    int64_t data_offset = 0, count = 0 /* frames */, n_samples = 0 /* per channel */;
    size_t need = 0;      // bytes of the file that go into the image: everything up to the last sample taken
    bool gather = true;   // the frames are contiguous int16 stereo in the file
    // MP3S_OPT_WAV_RESAMPLE, a file whose rate is not the target's: samplerate and count are the output's, n_samples the input's
    bool resample = false;
    int L = 1, M = 1, T = 0;
    int64_t in_frames = 0 /* ceil(n_samples / 1152): what k_wav_import fills of the scratch */, n_out = 0;
};
// which reader a call or a pipe reads its WAV files with: made from the context's options in ONE place (a non-zero resample value
// implies the import reader); a pipe keeps the value of the day it was created
struct WavRead { bool import = false; int resample = 0; };
WavRead wav_read_of(const mp3s_ctx *c);
int wav_encode_plan(WavRead how, const uint8_t *wav, size_t len, int bitrate_kbps, const uint8_t *hide_bits, int n_hide, WavPlan *p);
// a WAV file of a list call: its bytes, its message, its plan
struct WavIn {
    const uint8_t *wav; size_t len;
    const uint8_t *hide; int n_hide;
    WavPlan p;
};
struct WavBatch;
// the files `idx` to the device: their images up, the batch's kernels (launch_wav_batch) queued on the context's stream -> *d_pcm_out =
// [b.n_all][1152][2] int16 in the context's PCM buffer, the streams back to back in the order of idx (segs[k] = stream k).  Nothing is
// waited for; the batch's records and the callers' bytes are read by copies in flight until the stream is synchronised.
// the packed tap table of the ratio L / M on the context's device (pairs of consecutive taps as int16 halves, [L][T / 2] dwords): made and
// uploaded when the context meets the ratio first, kept until it goes.  For wav_to_device and the PCM batch calls that take a rate
int resample_taps_dev(mp3s_ctx *c, int L, int M, const uint32_t **d_out);
int wav_to_device(mp3s_ctx *c, const std::vector<WavIn> &in, const std::vector<int> &idx, std::vector<EncSeg> &segs, WavBatch &b, void **d_pcm_out);
// mp3s_encode_files with the reader named by the caller
int encode_files_as(mp3s_ctx *c, WavRead how, const uint8_t *const *wavs, const size_t *lens, int n_files, const int32_t *bitrate_kbps,
                    const uint8_t *const *hide_bits, const int32_t *n_hide, mp3s_buf **owner, mp3s_file *out, int32_t *status);

// ---------------------------------------------------------------- files into a device image, WAV batches (wav_batch.cpp)
// `bytes` from `src` to byte `dst` of a device image
struct Upload { size_t dst; const uint8_t *src; size_t bytes; };
// The copies that bring `files` (in image order) up: a long file goes from where it lies, short ones are laid into page-locked or
// plain staging at their places in the image first, bytes as they are, and travel in runs -- one copy per run instead of one per
// file (a copy from ordinary memory costs its thread 10 us and more whatever its size).  Whose staging it is and how it grows is the
// caller's business: staging(extent) is asked once, when there is a short file, for room for bytes [0, extent) of the image.
// false: it returned nullptr.  A copy u of a run has u.src == the staging + u.dst.
bool plan_uploads(const std::vector<Upload> &files, const std::function<uint8_t *(size_t extent)> &staging, std::vector<Upload> &ups);

// The layout of a batch of WAV files (one sampling rate and bitrate) on the device, for mp3s_encode_files and the pipe's encode jobs
// alike: every file at a 16-byte aligned place of one byte image, the records of the kernels that make the batch's PCM buffer
// [n_all][1152][2] int16 out of it -- k_wav_gather (runs), k_wav_import (iruns), and for the streams of MP3S_OPT_WAV_RESAMPLE
// k_wav_import into a scratch of s_all frames at the source rate (sruns) and k_wav_resample from there (rruns) -- and the longest
// stream per kernel (the grid).  Filled file by file in batch order; only the buffers are the caller's.
struct WavBatch {
    std::vector<Upload> files;           // per file: its place in the image, its bytes, how many of them the image takes
    std::vector<uint32_t> first;         // ... and its first frame in the PCM buffer
    std::vector<WavRun> runs;
    std::vector<WavImportRun> iruns, sruns;
    std::vector<WavResampleRun> rruns;
    int64_t max_frames = 0, max_iframes = 0, max_sframes = 0, max_rframes = 0;
    int64_t n_all = 0, s_all = 0;        // frames of the PCM buffer, of the resampler's scratch
    size_t img = 0;                      // the image's end (kWavSlack readable bytes are needed behind it)
    size_t res_lds = 0;                  // dynamic LDS of the k_wav_resample launch
    // the record block [runs | iruns | sruns | rruns], every part 16-byte aligned: offsets from the start of the buffer that holds it
    size_t o_runs = 0, o_iruns = 0, o_sruns = 0, o_rruns = 0, rec_end = 0;
    struct Part { size_t at; const void *data; size_t bytes; };

    void clear();                        // (the vectors keep their room: a job of a pipe fills the batch of the job before it)
    // d_taps: the packed tap table of the stream's ratio on the device (a stream to resample only).  MP3S_OK, or the batch is too large
    int add(const WavPlan &p, const uint8_t *wav, const uint32_t *d_taps);
    void place_records(size_t base);     // the block at `base` (rounded up to 16) -> o_*, rec_end
    std::array<Part, 4> parts() const;   // where each part of the block goes and what it is made of
};
// what makes the PCM buffer out of the image, queued on `stream`: import into the scratch d_rows and the resampler (when the batch
// has such streams), the gather, the import.  d_records: the device buffer the batch's o_* count from
int launch_wav_batch(hipStream_t stream, const uint8_t *d_image, const uint8_t *d_records, const WavBatch &b, int16_t *d_pcm, int16_t *d_rows, Profiler *prof);

// ---------------------------------------------------------------- one file as chunks through the overlapped stages (run_file.cpp)
constexpr int kRunFallback = 1;          // run_file: not for this path -- the caller takes the synchronous one (same bytes)
constexpr int kRunHide = 0, kRunClear = 1, kRunDecode = 2;
struct RunResult {
    int64_t n_frames = 0, n_rows = 0;
    int nch = 0, sampling_rate = 0, bit_rate = 0, kbps = 0;
    const uint8_t *mp3 = nullptr; size_t mp3_len = 0;        // hide / clear
    int64_t hide_offset = 0; int too_long = 0;
    const uint8_t *pcm = nullptr;                            // decode: [n_rows][nch] in the format asked for, 64 bytes into its block
    const uint8_t *bits = nullptr; size_t n_bits = 0;
};
// mode: kRunHide (utf8 / n_msg = the message) / kRunClear / kRunDecode (out_format).  MP3S_OK, kRunFallback, or an error.
int run_file(mp3s_ctx *c, const uint8_t *mp3, size_t len, int mode, const uint8_t *utf8, size_t n_msg, int out_format, mp3s_buf **owner, RunResult *out);
void destroy_own_pipe(mp3s_ctx *c);
void pipe_quiesce(mp3s_pipe *P);     // pipe_jobs.cpp: threads ended, streams drained, nothing freed
void own_pipe_lanes(const mp3s_ctx *c, mp3s_run_stats *out);

// ---------------------------------------------------------------- what this process may use of the host (mp3s_hostinfo.cpp)
// CPUs the process may run on: sched_getaffinity, cut down to the cgroup's CPU quota
int host_cpus_allowed();
// ranks sharing this host: LOCAL_WORLD_SIZE of the launcher, 1 without one
int local_world_size();
// host threads a rank should scan / walk with: MP3S_OPT_SCAN_THREADS, or its share of the allowed CPUs (one is kept for the
// thread that issues and collects), between 1 and 3
int default_scan_threads(const mp3s_ctx *c);
// the CPUs of the GPU's NUMA node that this process may run on (sysfs numa_node of the PCI device); empty: unknown, no binding
std::vector<int> gpu_node_cpus(int device);
