// The part of a one-file call (run_file.cpp) that decides without a device: how many frames the file can hold, how large its result block and
// the pipe's slots are, how the stream is cut into chunks, and what the real carry across a chunk boundary means for a chunk that ran on a
// guessed one.  Arithmetic on integers and mp3s_carry only -- run_file.cpp holds the buffers, copies and launches -- so that a stand-alone
// program can run it (tests/test_run_plan.py).
#pragma once
#include "mp3s_internal.h"

constexpr int kRunWhole = 2;             // run_file_impl: the stream inherits scalefactors across frames -- once more, as one piece
constexpr long kWholeFrames = 4 * kDecodeChunk;   // ... if it is not longer than this (the slots are sized for the piece)

// ---- sizes: the frames a file of `len` bytes can hold behind `offset` at its first frame's size, and what is sized by them
inline long run_frames_estimate(size_t len, size_t offset, long fs0) { return (long)((len - offset) / (size_t)std::max<long>(fs0 - 1, 24)) + 8; }
// the result block: PCM behind a 64-byte head for a decode, frames at the first frame's size otherwise
inline size_t run_result_bytes(bool decode, long n_est, long fs0, int nch, size_t esz)
{
    return decode ? 64 + (size_t)(n_est + 64) * 1152 * (size_t)nch * esz : (size_t)(n_est + 64) * (size_t)(fs0 + 2);
}

// ---- the chunk plan.  Every chunk costs a dozen launches and their gaps, so few chunks; the first one small, so that
//      the device starts early; a message's reach inside the first chunk, where the cursor is decided (not guessed)
struct RunPlan {
    bool ok = false;                     // false: not for this path (the synchronous one plans over the whole file)
    long first_chunk = 0, chunk = 0;     // frames of the first chunk, of those behind it
    long cap_frames = 0;                 // what a slot of the pipe holds: the largest chunk with its lead and halo
    long reach_frames = 0;               // the frames a message of n_hide bits can reach
    // what ensure_own_pipe is asked for
    size_t pipe_bytes(long fs0) const { return (size_t)cap_frames * (size_t)(fs0 + 2) + 4096; }
    size_t pipe_frames() const { return (size_t)cap_frames; }
};

// opt_chunk / opt_first: MP3S_OPT_CHUNK_FRAMES / MP3S_OPT_FIRST_CHUNK_FRAMES (0: automatic); whole: the stream as one piece (kRunWhole)
inline RunPlan run_plan(long n_est, int64_t n_hide, int64_t opt_chunk, int64_t opt_first, bool whole)
{
    RunPlan p;
    p.reach_frames = n_hide ? (long)((n_hide * 5 / 14 + 32) / 4 * 9 / 8 + 64) : 0;
    const long kMaxChunk = kDecodeChunk - 2;
    p.chunk = (long)opt_chunk;
    if (p.chunk > 0) { p.chunk = std::min(p.chunk, kMaxChunk); p.first_chunk = p.chunk; }
    else if (n_est <= 3000) { p.chunk = p.first_chunk = std::min(kMaxChunk, n_est + 16); }                    // one chunk: nothing to overlap with
    else {
        // A short first chunk, so that the device starts early, then chunks as long as a transform group takes: every chunk
        // costs the host 0.15 ms of walking, laying out and queueing (two dozen runtime calls), which four chunks of a
        // 10 000-frame file do not win back (round 3, profiles/r03a_chunk_plans.json: 2 048 + the rest 1.41 ms, four chunks 1.49, one 1.57;
        // a 100 000-frame file: 8 192 + 16 000s 8.1 ms)
        p.first_chunk = std::min<long>(8192, std::max<long>(2048, n_est / 12));
        p.chunk = kMaxChunk;
    }
    if (opt_first > 0) p.first_chunk = (long)std::min<int64_t>(opt_first, kMaxChunk);
    p.first_chunk = std::min(kMaxChunk, std::max(p.first_chunk, p.reach_frames));
    if (whole) {
        if (n_est > kWholeFrames) return p;
        p.first_chunk = p.chunk = n_est + 64;          // one piece
    }
    p.cap_frames = std::max(p.chunk, p.first_chunk) + 2;
    // (a message that reaches further than a chunk: the synchronous path's plan over the whole file)
    p.ok = p.reach_frames <= kMaxChunk;
    return p;
}

// ---- the carry rule.  A chunk behind the first runs on a GUESSED carry ("the message is hidden, nothing is inherited") and reports
//      whether it looked at it.  (The same rule between ranks, stated in Python: mp3stego/sharded.py.)
// two carries a chunk cannot tell apart: equal chains, and cursors equal or both past the message
inline bool same_effect(const mp3s_carry &a, const mp3s_carry &b, int64_t n_hide)
{
    return std::memcmp(a.chain, b.chain, sizeof a.chain) == 0 && std::min<int64_t>(a.cursor, n_hide) == std::min<int64_t>(b.cursor, n_hide);
}

// `real` is the carry in front of a chunk that ran on `guess` and handed on `out`.  false: the chunk looked at its carry (or the message is
// still being hidden at this boundary) and the guess was wrong -- it runs again, on `real`; `out` is left as it is.  true: nothing in the
// chunk looked at the carry: every chain entry it hands on is its own; only the count of tables seen so far moves with the real cursor.
inline bool carry_settles(const mp3s_carry &real, const mp3s_carry &guess, bool carry_used, int64_t n_hide, mp3s_carry &out)
{
    const bool live = std::min<int64_t>(real.cursor, n_hide) < n_hide;     // the message is still being hidden at this boundary
    if (!same_effect(real, guess, n_hide) && (carry_used || live)) return false;
    out.cursor = real.cursor + (out.cursor - guess.cursor);
    return true;
}
