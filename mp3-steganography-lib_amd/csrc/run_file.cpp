// ------------------------------------------------------------------------------------------------ one file as chunks
// The reference's call shape is one file per call (steganography.py:137-162: decode loop MP3_Parser.py:68-80, then encode
// loop MP3_Encoder.py:607-609).  run_file gives that call the overlap the pipe gives a stream of jobs: the calling thread
// walks the frame headers a chunk at a time and queues each chunk on the stages above -- walk(k+1) || upload || front end ||
// kernels(k) || download(k-1) -- and the chunks' bytes land side by side in ONE result block.  What crosses a chunk
// boundary is what crosses a block boundary of a sharded stream: a frame of decoder state and a frame of
// PCM in front of the chunk are recomputed and dropped; the padding recurrence is replayed from the frame index; the message
// cursor and the inherited addresses (17 integers) are GUESSED -- "the message is hidden, nothing is inherited" -- and every
// chunk reports whether it looked at them: only a chunk that did, on a guess that was wrong, is run again on the real carry.
#include "pipe_internal.h"
#include "run_plan.h"

int ensure_own_pipe(mp3s_ctx *c, size_t chunk_bytes, size_t chunk_frames)
{
    if (c->own_pipe && c->own_pipe->max_job_bytes >= chunk_bytes && c->own_pipe->max_frames >= chunk_frames) return MP3S_OK;
    if (c->own_pipe) {
        // A file with larger frames than any before it (a higher bit rate): the slots' byte buffers are too small.  The old pipe is PARKED, not
        // destroyed: handing its page-locked and device buffers back to the driver at this point made every copy of the next ten calls run at
        // half rate (r06, tools/repro_config5.py + rocprofv3 --memory-copy-trace: 28 instead of 56 GB/s down, the same sizes, agents and stream;
        // kept instead: the first call 9 instead of 20 ms, none slow behind it -- config 5's joint_ms_short_48k_192 at 1.6 or 2.5 ms by where the
        // seven timed calls fell).  Frame sizes are bounded (1 441 bytes), so at most a few pipes are ever parked; they go with the context.
        // (a whole-mode piece and growing files park more than "a few".  What is asked for here is RunPlan's pipe_bytes /
        // pipe_frames, run_plan.h: a bound on the parked pipes is a change to this function and that field.)
        pipe_quiesce(c->own_pipe);
        c->parked_pipes.push_back(c->own_pipe);
        c->own_pipe = nullptr;
    }
    const size_t want = std::max<size_t>(chunk_bytes + chunk_bytes / 4, (size_t)1 << 20);
    // (chunks are cut by frames: the slots' per-frame arrays are sized by what a chunk can hold, not by the 96-byte frames its bytes could be)
    return pipe_create(c, kRunDepth, want, 0, true, &c->own_pipe, std::max<size_t>(chunk_frames + chunk_frames / 4, 4096));
}

// how the streams of the context's own pipe were chosen (mp3s_ctx_run_stats)
void own_pipe_lanes(const mp3s_ctx *c, mp3s_run_stats *out)
{
    if (!c->own_pipe) return;
    const LaneReport &r = c->own_pipe->lanes;
    out->rehearsal_us = (int64_t)(r.rehearsal_ms * 1e3); out->rehearsals = r.rehearsals; out->lanes = r.lanes; out->queue_shared = r.queue_shared;
}

void destroy_own_pipe(mp3s_ctx *c)   // (the context is being destroyed)
{
    if (c->own_pipe) { mp3s_pipe_destroy(c->own_pipe); c->own_pipe = nullptr; }
    for (mp3s_pipe *p : c->parked_pipes) mp3s_pipe_destroy(p);
    c->parked_pipes.clear();
    forget_lanes(c);
}

namespace {

struct RunChunk {
    std::unique_ptr<Job> job;
    long first = 0, count = 0;
    bool last = false;
    mp3s_carry guess = {}, out = {};
    bool carry_used = false;
    int64_t out_off = 0, out_len = 0;
    bool done = false;
};

// (for the duration of the call the context computes on the stream its pipe rehearsed best with, if that is not its own)
struct StreamSwap {
    mp3s_ctx *c; hipStream_t keep;
    StreamSwap(mp3s_ctx *c_, hipStream_t s) : c(c_), keep(c_->stream) { if (s) c->stream = s; }
    ~StreamSwap() { if (c->stream != keep) { (void)hipStreamSynchronize(c->stream); c->stream = keep; } }
};
struct FileUpGuard { mp3s_pipe *P; ~FileUpGuard() { file_up_end(P); } };

// One call on one file, from the first chunk's walk to the result: what run_file_impl opened and planned (borrowed), the stream's frame
// table, the result block, the chunks and where the early sink stands.  run_file_impl drives it: step() chunk after chunk, the last issue_b,
// settle(), fill().
struct FileRun {
    mp3s_ctx *c; mp3s_pipe *P;
    const uint8_t *mp3; size_t len;
    const bool decode; const int out_format; const size_t esz;
    FrameWalker &w;
    const std::vector<uint8_t> &bits; const int64_t n_hide;   // the framed message
    const long fs0, n_est, cap_frames;
    const double t_call0;
    // ---- the stream's frame table, grown as the walk proceeds
    std::vector<FrameRef> &refs;
    std::vector<uint8_t> &tables;
    long n_walked = 0;
    std::unique_ptr<mp3s_buf> res;
    std::vector<RunChunk> chunks;
    PlaceEntry fix;                              // the stream's last frame, decoded here when the walk ends (E14)
    bool have_fix = false;
    int rate = 0, kbps = 0, nch = 0;
    size_t res_cap = 0;
    int64_t hide_offset = 0;
    // (mp3s_*_fd: a chunk's bytes go to the file as soon as they are final -- while the chunks behind it are still on the device.)
    // Only into a file that was EMPTY when the call began (sink_early): a stream that is refused late -- a damaged frame in the last chunk, found
    // on the device -- ends in an error, and the reference has not touched its output file at that point; a file that held something is written
    // at the end of a call that succeeded (the entry point does that), a fresh one is removed by the caller that created it.
    bool sink_on;
    size_t sink_next = 0;
    mp3s_carry sink_real = {};

    FileRun(mp3s_ctx *c_, const uint8_t *mp3_, size_t len_, bool decode_, int out_format_, FrameWalker &w_, const std::vector<uint8_t> &bits_, long fs0_, long n_est_,
            const RunPlan &plan, double t_call0_)
        : c(c_), P(c_->own_pipe), mp3(mp3_), len(len_), decode(decode_), out_format(out_format_), esz(pcm_elem(out_format_)), w(w_), bits(bits_),
          n_hide((int64_t)bits_.size()), fs0(fs0_), n_est(n_est_), cap_frames(plan.cap_frames), t_call0(t_call0_), refs(c_->h_refs), tables(c_->h_tables),
          res(new mp3s_buf()),
          sink_on(c_->sink_fd >= 0 && c_->sink_early && (!decode_ || out_format_ == MP3S_PCM_I16))   // (a decode's chunks have no carries: final when they are down)
    {
        if ((long)refs.size() < n_est + 64) refs.resize((size_t)n_est + 64);
        if (n_hide) { w.tables_wanted = (long)n_hide + (long)n_hide / 16 + 64; tables.resize((size_t)plan.first_chunk * 4 + 16); }
    }

    // EVERY way out of the call after the first chunk has been queued goes through here (another path takes the file, or a hard
    // error such as MP3S_E_HIP): nothing of this call may still be in flight when its result block, its jobs and the slots are
    // let go -- a queued download would otherwise write into page-locked memory the pool hands to the next call
    int fallback(const char *why, int code = kRunFallback)
    {
        if (trace_on()) fprintf(stderr, "mp3s: run_file: %s -> %s\n", why, code == kRunWhole ? "once more, in one piece" : code == kRunFallback ? "synchronous path" : "error");
        if (code == kRunFallback) c->run_stats.fallbacks++;
        pipe_release_slots(P, true);
        return code;
    }

    // retire chunk k: wait for its results, settle its verdict and its carry
    int retire(size_t k)
    {
        RunChunk &rc = chunks[k];
        if (rc.done) return MP3S_OK;
        Job *j = rc.job.get();
        Slot &s = P->slots[(size_t)j->slot];
        if (issue_down(P, *j, s)) return kRunFallback;
        if (hipEventSynchronize(s.e_down) != hipSuccess) return fail(MP3S_E_HIP, "waiting for a chunk's results failed");
        if (trace_on()) {
            float up = 0, huff = 0, rl = 0, comp = 0, down = 0;
            hipEvent_t e0 = P->slots[(size_t)chunks[0].job->slot].e_start;
            if (k >= (size_t)P->depth) e0 = s.e_start;
            (void)hipEventElapsedTime(&up, e0, s.e_up); (void)hipEventElapsedTime(&huff, e0, s.e_huff); (void)hipEventElapsedTime(&rl, e0, s.e_rate);
            (void)hipEventElapsedTime(&comp, e0, s.e_comp); (void)hipEventElapsedTime(&down, e0, s.e_down);
            (void)hipGetLastError();
            fprintf(stderr, "mp3s: run_file: chunk %zu's results are here %.3f ms after the call's start; on the device, from the first chunk's start: inputs up %.3f, "
                            "front end done %.3f, rate loop done %.3f, tail done %.3f, results down %.3f ms\n", k, now_ms() - t_call0, up, huff, rl, comp, down);
        }
        bool resolved = false;
        const bool ok = finish_fast(P, j, s, &resolved);
        if (!ok && !resolved) return kRunFallback;
        if (resolved) c->run_stats.resolved++;
        const SmallView small{j->res->big[2].data()};
        // scalefactors inherited across frames: the Huffman kernel walks back to the granule that wrote them.  With the
        // file's side records and main data in file-wide arrays it finds them across chunk boundaries (round 4); without them
        // (a file above 1 GB, no memory) the stream goes through the stages once more, in one piece
        if (j->walked && !j->file_wide && small.head().inherits_across_frames() && chunks.size() + (w.ended ? 0 : 1) > 1) return kRunWhole;
        if (!decode) {
            const EncSeg &sg = j->segs[0];
            if (resolved) std::memcpy(j->ck.dst, j->res->mp3 + sg.mp3_off, sg.mp3_len);
            const SegEnd e = seg_end(sg, small.seg_out(0), resolved);
            rc.out = e.out; rc.carry_used = e.carry_used;
            rc.out_len = (int64_t)sg.mp3_len;
        }
        rc.done = true;
        return MP3S_OK;
    }

    // The early sink (see sink_on), chunks 0 .. k having been retired.  Final = the chunk will not be run again on its real carry: the test
    // settle() makes at the end (carry_settles, run_plan.h), here on a copy of the carries, nothing settled.
    void sink_upto(size_t k)
    {
        for (; sink_on && sink_next <= k && sink_next < chunks.size(); sink_next++) {
            const RunChunk &rc = chunks[sink_next];
            mp3s_carry mine = rc.out;
            if (!decode && sink_next > 0 && !carry_settles(sink_real, rc.guess, rc.carry_used, n_hide, mine)) { sink_on = false; break; }   // (it will be run again: its bytes change)
            const size_t off = decode ? (size_t)rc.first * 1152 * (size_t)nch * esz : (size_t)rc.out_off;
            const size_t n = decode ? (size_t)rc.count * 1152 * (size_t)nch * esz : (size_t)rc.out_len;
            if (off != c->sink_done) { sink_on = false; break; }
            // (a write that fails: the caller writes what is missing, and reports what fails there)
            if (pwrite_all(c->sink_fd, res->big[0].data() + (decode ? 64 : 0) + off, n, c->sink_base + off) != n) { sink_on = false; break; }
            c->sink_done = off + n;
            sink_real = mine;
        }
    }

    // issue frames [first, first + count) of the stream as a chunk on slot `slot`
    // A chunk is queued in two steps.  issue_a: its front end (file piece, parse, Huffman -- a latency chain of 0.1 ms whatever the
    // chunk's size).  issue_b: the results of the chunk in front, this chunk's encoder inputs (laid out here, 0.1 ms of host time
    // for 8 000 frames) and everything behind the front end.  step() runs issue_a(k + 1) BEFORE issue_b(k) (round 4): the next
    // chunk's front end is then on the device while this chunk's kernels still run -- queued behind issue_b(k) it started 0.1 ms
    // later, ended behind the chunk's rate loop, and the compute stream sat idle for 0.05 ms between two chunks.
    int issue_a(size_t k, const mp3s_carry *carry)
    {
        RunChunk &rc = chunks[k];
        rc.job.reset(new Job());
        Job &j = *rc.job;
        j.slot = (int)(k % (size_t)P->depth);
        j.ticket = (int64_t)k;
        // (the context's buffers the chunks take turns with -- Huffman outputs, PCM -- are asked for at the size of the call's largest
        // chunk: a chunk that asked for more than the one before it in the same set would have the buffer replaced while that
        // chunk's results still wait in it to be copied out, now that their copy is queued behind the next front end)
        j.grab_frames = (int)cap_frames;
        Slot &s = P->slots[(size_t)j.slot];
        if (!pipe_slot_ready(P, s)) return kRunFallback;
        Chunk &ck = j.ck;
        ck.decode = decode;
        chunk_window(ck, refs.data(), rc.first, rc.count, rc.last, mp3, len);
        ck.out_format = out_format; ck.rate = rate; ck.kbps = kbps; ck.nch = nch;
        ck.fix = rc.last && have_fix ? &fix : nullptr;
        ck.hide = bits.data(); ck.n_hide = (int)n_hide;
        j.clear_all = n_hide == 0;
        ck.has_carry = rc.first > 0;
        if (ck.has_carry) ck.carry_in = carry ? *carry : rc.guess;
        ck.tables = rc.first == 0 && n_hide ? tables.data() : nullptr;
        ck.n_tables = (int)std::min<long>(w.tables_frames, rc.count) * 4;
        ck.any_silent = w.any_silent ? 1 : 0;   // (of the frames walked so far: at worst the re-run launches are issued without need)
        if (decode) ck.dst = res->big[0].data() + 64 + (size_t)rc.first * 1152 * (size_t)nch * esz;
        if (!prepare_chunk(P, j, s, w.max_p23)) return kRunFallback;
        if (issue_front(P, j, s, 0, w.max_p23, true)) return kRunFallback;
        if (c->opt[MP3S_OPT_FAIL_CHUNK] == (int64_t)k + 1) {      // (test aid: a hard error with this chunk's front end and the chunks in front of it in flight)
            c->opt[MP3S_OPT_FAIL_CHUNK] = 0;
            return fail(MP3S_E_HIP, "chunk %zu: failure injected by MP3S_OPT_FAIL_CHUNK", k);
        }
        return MP3S_OK;
    }
    int issue_b(size_t k)
    {
        RunChunk &rc = chunks[k];
        Job &j = *rc.job;
        Slot &s = P->slots[(size_t)j.slot];
        const double t_i = trace_on() ? now_ms() : 0;
        // (the results of the chunk in front come down behind this chunk's inputs, not in front of them)
        if (k > 0 && chunks[k - 1].job && issue_down(P, *chunks[k - 1].job, P->slots[(size_t)chunks[k - 1].job->slot])) return kRunFallback;
        if (!prepare_chunk_encode(P, j, s)) { sync_all(P); return kRunFallback; }
        if (!decode) {
            rc.out_off = j.L.bytes_before;
            if ((size_t)rc.out_off + j.L.mp3_bytes > res_cap) { sync_all(P); return kRunFallback; }
            j.ck.dst = res->big[0].data() + rc.out_off;
        }
        const int e = issue_back(P, j, s, true, true);
        if (trace_on()) fprintf(stderr, "mp3s:   inputs + back of chunk %zu %.3f ms\n", k, now_ms() - t_i);
        return e ? kRunFallback : MP3S_OK;
    }
    int issue(size_t k, const mp3s_carry *carry) { const int r = issue_a(k, carry); return r ? r : issue_b(k); }

    // walk up to `want` frames behind those walked so far -> *got; the first chunk settles what the stream is and makes the result block,
    // the last one decodes the stream's last frame
    int walk_chunk(size_t k, long want, long *got_out)
    {
        long got = 0;
        const long room = (long)refs.size() - n_walked - 8;
        if (room <= 0) return fallback("more frames than the file's first frame size promised");
        want = std::min(want, room);
        uint8_t *tb = k == 0 && n_hide ? tables.data() : nullptr;
        while (got < want && !w.ended && !w.irregular) got += w.next(refs.data() + n_walked + got, want - got, tb ? tb + (size_t)got * 4 : nullptr, 0, 0);
        if (w.irregular || got <= 0) return fallback("the walk does not take this stream");
        if (k == 0) {
            nch = w.nch; rate = w.sampling_rate;
            if (nch < 1 || nch > 2) return fallback("channel count");
            if (!decode && reencode_params(w.sampling_rate, w.bit_rate, w.nch, got, 0, &kbps)) return fallback("not a stream the encoder takes");
            // the result block: the frames the file can hold at its first frame's size
            res_cap = run_result_bytes(decode, n_est, fs0, nch, esz);
            if (!res->big[0].reserve(res_cap)) return fallback("no memory for the result");
        } else if (w.nch != nch) return fallback("channel count changes");
        if (w.ended) {
            if (w.dup_last) return fallback("a repeated last frame");
            have_fix = fill_place_entry(fix, 0, [&](int16_t *is, mp3s_granule_si *si) { bool alone = false; return w.decode_last(is, si, &alone) == 0 && alone; });
        }
        *got_out = got;
        return MP3S_OK;
    }

    // chunk k: walk it, retire the chunk that had its slot, queue its front end and the back of the chunk in front (issue_a's comment)
    int step(size_t k, long want)
    {
        const double t_walk0 = trace_on() ? now_ms() : 0;
        long got = 0;
        if (const int r = walk_chunk(k, want, &got)) return r;
        const double t_walk1 = trace_on() ? now_ms() : 0;
        if (k >= (size_t)P->depth) {               // the slot's previous chunk first
            const int r = retire(k - (size_t)P->depth);
            if (r) return fallback("a chunk needs another path", r);
            sink_upto(k - (size_t)P->depth);
        }
        const double t_ret = trace_on() ? now_ms() : 0;
        chunks.emplace_back();
        RunChunk &rc = chunks.back();
        rc.first = n_walked; rc.count = got; rc.last = w.ended;
        rc.guess.cursor = MP3S_NO_CURSOR;          // "the message is hidden, nothing is inherited"
        n_walked += got;
        if (decode && 64 + (size_t)n_walked * 1152 * (size_t)nch * esz > res_cap) return fallback("more frames than the result block holds");
        int r = issue_a(k, nullptr);
        if (!r && k > 0) r = issue_b(k - 1);
        if (trace_on()) fprintf(stderr, "mp3s: run_file chunk %zu (%ld frames): walk %.3f ms, wait for the slot %.3f ms, prepare + issue %.3f ms\n", k, got, t_walk1 - t_walk0, t_ret - t_walk1, now_ms() - t_ret);
        return r ? fallback("a chunk does not fit the stages", r) : MP3S_OK;
    }

    // ---- settle the chunks in order: the carries
    int settle()
    {
        if (!decode && (w.sampling_rate != rate || w.bit_rate / 1000 != kbps)) return fallback("the last header names another rate");
        // (first everything that needs a chunk's device buffers -- its verdict, a resolve -- then the carries: a chunk that is run
        // again takes a slot, and with it the buffers of the chunk that had it last)
        for (size_t k = 0; k < chunks.size(); k++) {
            const int r = retire(k);
            if (r) return fallback("a chunk needs another path", r);
            sink_upto(k);
        }
        mp3s_carry real = {};
        for (size_t k = 0; k < chunks.size() && !decode; k++) {
            RunChunk &rc = chunks[k];
            if (k > 0 && !carry_settles(real, rc.guess, rc.carry_used, n_hide, rc.out)) {
                // the chunk looked at its carry and the guess was wrong: once more, on the real one (everything behind it has been issued
                // and stays as it is unless its own carry turns out wrong in turn)
                if (trace_on()) fprintf(stderr, "mp3s: run_file: chunk %zu depends on its carry: again\n", k);
                sync_all(P);
                c->run_stats.reruns++;
                rc.done = false;
                int r = issue(k, &real);
                if (!r) r = retire(k);
                if (r) return fallback("a chunk needs another path", r);
                sync_all(P);
            }
            real = rc.out;
            hide_offset = real.cursor;
        }
        return MP3S_OK;
    }

    // ---- the result
    void fill(RunResult *out)
    {
        std::memset(out, 0, sizeof *out);
        out->n_frames = n_walked; out->nch = nch; out->sampling_rate = w.sampling_rate; out->bit_rate = w.bit_rate;
        if (decode) {
            // stego bits: the serial pass over the table-index words of all chunks (their halo frames left out)
            uint8_t carry[4] = {0, 0, 0, 0};
            for (auto &rc : chunks) {
                const Job &j = *rc.job;
                stego_bits_from_tsel((const uint64_t *)j.res->big[1].data() + j.ck.halo, rc.count, nch, carry, res->bits);
            }
            out->pcm = res->big[0].data() + 64; out->n_rows = (int64_t)n_walked * 1152;
            out->bits = res->bits.data(); out->n_bits = res->bits.size();
        } else {
            const RunChunk &lc = chunks.back();
            out->mp3 = res->big[0].data(); out->mp3_len = (size_t)(lc.out_off + lc.out_len);
            out->kbps = kbps;
            out->hide_offset = hide_offset;
            out->too_long = hide_offset < n_hide - 1 ? 1 : 0;
        }
    }
};

int run_file_impl(mp3s_ctx *c, const uint8_t *mp3, size_t len, int mode, const uint8_t *utf8, size_t n_msg, int out_format, mp3s_buf **owner, RunResult *out, bool whole)
{
    c->sink_done = 0;                                                // (mp3s_*_fd: nothing of THIS attempt's result is in the file yet)
    if (!c->opt[MP3S_OPT_FILE_PIPELINE] || !c->opt[MP3S_OPT_DEVICE_PARSE]) return kRunFallback;
    const double t_call0 = trace_on() ? now_ms() : 0;
    FrameWalker w;
    // (errors and empty streams: the synchronous path words them)
    if (len < 8 || len > 0xffff0000ull || w.open(mp3, len) || w.ended || w.hd.version != 1 || w.hd.layer != 3 || w.frame_size <= 0) {
        c->run_stats.fallbacks++;
        return kRunFallback;
    }
    const long fs0 = w.frame_size;
    const long n_est = run_frames_estimate(len, (size_t)w.offset, fs0);
    std::vector<uint8_t> bits;
    if (mode == kRunHide) {
        message_frame(utf8, n_msg, bits);
        if (bits.size() > 0x3fffff00) { c->run_stats.fallbacks++; return kRunFallback; }
    }
    const RunPlan plan = run_plan(n_est, (int64_t)bits.size(), c->opt[MP3S_OPT_CHUNK_FRAMES], c->opt[MP3S_OPT_FIRST_CHUNK_FRAMES], whole);
    if (!plan.ok || ensure_own_pipe(c, plan.pipe_bytes(fs0), plan.pipe_frames())) { c->run_stats.fallbacks++; return kRunFallback; }
    mp3s_pipe *P = c->own_pipe;
    HIPCHK(hipSetDevice(c->device));
    StreamSwap swap(c, P->s_comp);
    // the file's bytes set off for the device now (the first chunk's first), the walk follows
    FileUpGuard up_guard{P};
    file_up_begin(P, mp3, len, (size_t)w.offset + (size_t)std::min<long>(plan.first_chunk, n_est) * (size_t)(fs0 + 1) + 2048, n_est);
    FileRun run(c, mp3, len, mode == kRunDecode, out_format, w, bits, fs0, n_est, plan, t_call0);
    // ---- walk and issue, chunk after chunk
    // (a helper thread that walks the chunks behind the first while this one queues was tried: it wakes up later than the walk takes --
    // 1.56 instead of 1.38 ms per 10 000-frame file)
    for (size_t k = 0; k == 0 || !w.ended; k++)
        if (const int r = run.step(k, k == 0 ? plan.first_chunk : plan.chunk)) return r;
    if (const int r = run.issue_b(run.chunks.size() - 1)) return run.fallback("a chunk does not fit the stages", r);
    if (trace_on()) fprintf(stderr, "mp3s: run_file: all chunks queued %.3f ms after the call's start\n", now_ms() - t_call0);
    if (const int r = run.settle()) return r;
    run.fill(out);
    pipe_release_slots(P, false);
    c->run_stats.files++; c->run_stats.chunks += (int64_t)run.chunks.size();
    *owner = run.res.release();
    if (trace_on()) fprintf(stderr, "mp3s: run_file: done %.3f ms after the call's start\n", now_ms() - t_call0);
    return MP3S_OK;
}

}  // namespace

int run_file(mp3s_ctx *c, const uint8_t *mp3, size_t len, int mode, const uint8_t *utf8, size_t n_msg, int out_format, mp3s_buf **owner, RunResult *out)
{
    int rc = run_file_impl(c, mp3, len, mode, utf8, n_msg, out_format, owner, out, false);
    // A granule of a mixed block (or one behind a short granule 0 with scfsi set) reads scalefactors written many frames earlier
    // (SURVEY D10); the Huffman kernel finds them by walking back through the stream's side records, which a chunk that
    // starts in the middle of the stream cannot.  Such a file goes through the same stages in ONE piece (the transforms still
    // in groups): 1.7 instead of 4.4 ms for 10 000 frames, which the synchronous path spends in the host parser.
    if (rc == kRunWhole) rc = run_file_impl(c, mp3, len, mode, utf8, n_msg, out_format, owner, out, true);
    return rc == kRunWhole ? kRunFallback : rc;
}

