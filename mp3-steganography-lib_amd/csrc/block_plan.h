// How a stream is cut into blocks and how a batch is decoded in transform groups, without a device: a rank's share of the frames, the window
// of frames in front of a block, the walk over groups of kDecodeChunk frames, and the runs in which a group's PCM is copied out.  Arithmetic
// on frame indices only -- the callers (mp3s_reencode_block_indexed, mp3s_decode_block_indexed, chunk_window, prepare_block, decode_group,
// issue_back) hold the buffers, copies and launches -- so that a stand-alone program can run it (tests/test_block_plan.py).
#pragma once
#include "mp3s_internal.h"

// ---- a rank's share: contiguous blocks in rank order, sizes differing by at most one, the longer ones first.
//      (The same rule in Python: shard_frames of mp3stego/sharded.py.)
struct BlockShare { long first, count; };
inline BlockShare block_share(long total, long rank, long world)
{
    const long base = total / world, rem = total % world;
    return {rank * base + std::min(rank, rem), base + (rank < rem ? 1 : 0)};
}

// ---- the window of a block: frames [w0, w0 + n_win) of the stream go to the device for frames [first, first + count).  The first `halo`
//      only rebuild decoder state (IMDCT overlap, synthesis fifo: < 1 frame, Frame.py:151-153, 81-92), the next `lead` only encoder state
//      (filter bank + MDCT history: 1 056 samples, MP3_Encoder.py:356, 685, 747).
struct BlockWindow {
    int lead, halo;
    long w0, n_win;
    bool with_dup;                       // the frame the decoder repeats after a bad header (D12) belongs to the block; it is NOT one of n_win
};
// A stream of n_frames frames whose last one is repeated (dup_last).  An encode block counts PCM frames, of which the repeated one is the
// last (first + count <= n_frames + dup_last); a decode block (decode: no lead) counts the stream's own frames and ends where they end.
inline BlockWindow block_window(long first, long count, long n_frames, bool dup_last, bool decode)
{
    BlockWindow w;
    w.lead = !decode && first > 0 ? 1 : 0;
    w.halo = first - w.lead > 0 ? 1 : 0;
    w.w0 = first - w.lead - w.halo;
    w.n_win = std::min(first + count, n_frames) - w.w0;
    w.with_dup = dup_last && first + count >= n_frames + (decode ? 0 : 1);
    return w;
}

// ---- transform groups: frames [halo0, n) of a resident batch in groups of kDecodeChunk.  The first group brings the batch's own halo
//      (halo0 frames in front of it); a later one that starts inside a stream -- inside_stream(start) -- re-runs one frame of it for the
//      state.  fn(g) -> 0 or a code that ends the walk and is returned; no group runs when n <= halo0.
struct TransformGroup {
    long start;                          // the group's first own frame; its transforms begin at start - halo
    int halo, cnt;                       // cnt counts the halo
    bool last;
};
template <class Inside, class Fn>
inline int for_transform_groups(long n, int halo0, Inside inside_stream, Fn fn)
{
    for (long start = halo0; start < n; start += kDecodeChunk) {
        TransformGroup g;
        g.start = start;
        g.halo = start == halo0 ? halo0 : (inside_stream(start) ? 1 : 0);
        g.cnt = (int)std::min<long>(kDecodeChunk, n - start) + g.halo;
        g.last = start + kDecodeChunk >= n;
        if (const int rc = fn(g)) return rc;
    }
    return 0;
}

// ---- copy-out runs.  The streams of a batch lie end to end on the device; where they are copied to, one extra frame follows every
//      stream that repeats its last frame.  StreamSpan: a stream's first frame in the batch, its frames, whether it repeats the last.
struct StreamSpan { long first, n_frames; bool dup; };
// per stream its first frame on the destination side; *extra (when given): the frames the destination has more than the batch
inline std::vector<long> out_first_of(const std::vector<StreamSpan> &s, long *extra = nullptr)
{
    std::vector<long> out(s.size());
    long e = 0;
    for (size_t k = 0; k < s.size(); k++) { out[k] = s[k].first + e; e += s[k].dup ? 1 : 0; }
    if (extra) *extra = e;
    return out;
}
// Frames [start, end) of the batch in runs that are contiguous on both sides: a run ends with the last frame of a stream that repeats
// it, because the repeated frame is inserted behind it.  `count` frames from batch frame src_frame (of stream k) go to dst_frame.
struct CopyRun { size_t k; long src_frame, dst_frame, count; };
template <class Fn>
inline int for_copy_runs(const std::vector<StreamSpan> &s, const std::vector<long> &out_first, long start, long end, Fn fn)
{
    for (long a = start; a < end;) {
        const size_t k = (size_t)(std::upper_bound(s.begin(), s.end(), a, [](long f, const StreamSpan &x) { return f < x.first; }) - s.begin()) - 1;
        long b = end;
        for (size_t j = k; j < s.size() && s[j].first < end; j++)
            if (s[j].dup) { b = std::min(end, s[j].first + s[j].n_frames); break; }
        if (b <= a) b = std::min(end, a + 1);
        if (const int rc = fn(CopyRun{k, a, out_first[k] + (a - s[k].first), b - a})) return rc;
        a = b;
    }
    return 0;
}
