"""The device-free cut of a stream into blocks and of a batch into transform groups (csrc/block_plan.h) on the CPU: a stand-alone program reads
cases from a file and prints what the header returns; every rule is stated here a second time, as the callers had it before the header existed.
  block_share           against mp3stego.sharded.shard_frames and tests/shard.shard_frames (the same rule in Python)
  block_window          against mp3s_reencode_block_indexed, chunk_window and mp3s_decode_block_indexed as they computed lead, halo and window
  for_transform_groups  against the loops of decode_group and issue_back
  for_copy_runs         against the copy-out loop of decode_group, and against a frame-by-frame map
A case file is text: whitespace-separated integers, case after case, each beginning with its kind.  The copy-out cases name their windows
[start, end) themselves (a transform group's own frames are such a window), so they need no group of kDecodeChunk frames and stay small."""
import bisect
import itertools
import os
import re
import shutil
import subprocess

import pytest

from mp3stego import sharded
import shard
from test_run_plan import COMPILE_FLAGS, CSRC, ROCM_INCLUDE, run_program     # (one set of flags, one way to run a case program)

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "block_plan.h"

static FILE *g_in;
static long long next() { long long v; if (fscanf(g_in, "%lld", &v) != 1) { fprintf(stderr, "case file ends early\n"); exit(3); } return v; }

int main(int argc, char **argv)
{
    if (argc != 2 || !(g_in = fopen(argv[1], "r"))) return 2;
    long long kind;
    while (fscanf(g_in, "%lld", &kind) == 1) {
        if (kind == 0) {          // share: total rank world
            const long total = (long)next(), rank = (long)next(), world = (long)next();
            const BlockShare s = block_share(total, rank, world);
            printf("share %ld %ld\n", s.first, s.count);
        } else if (kind == 1) {   // window: first count n_frames dup_last decode
            const long first = (long)next(), count = (long)next(), n = (long)next();
            const bool dup = next() != 0, decode = next() != 0;
            const BlockWindow w = block_window(first, count, n, dup, decode);
            printf("window %d %d %ld %ld %d\n", w.lead, w.halo, w.w0, w.n_win, w.with_dup ? 1 : 0);
        } else if (kind == 2) {   // groups: n halo0 n_streams, the streams' first frames (ascending)
            const long n = (long)next();
            const int halo0 = (int)next();
            std::vector<long> first((size_t)next());
            for (long &f : first) f = (long)next();
            auto inside = [&](long f) { auto it = std::upper_bound(first.begin(), first.end(), f); return it != first.begin() && it[-1] < f; };
            printf("groups %d", kDecodeChunk);
            const int rc = for_transform_groups(n, halo0, inside, [&](const TransformGroup &g) { printf(" %ld %d %d %d", g.start, g.halo, g.cnt, g.last ? 1 : 0); return 0; });
            printf("\n");
            if (rc) return 4;
        } else if (kind == 3) {   // runs: start end n_streams, per stream its frames and whether it repeats the last
            const long start = (long)next(), end = (long)next();
            std::vector<StreamSpan> s((size_t)next());
            long at = 0;
            for (StreamSpan &x : s) { x.first = at; x.n_frames = (long)next(); x.dup = next() != 0; at += x.n_frames; }
            long extra = -1;
            const std::vector<long> out_first = out_first_of(s, &extra);
            printf("runs %ld", extra);
            for (long f : out_first) printf(" %ld", f);
            const int rc = for_copy_runs(s, out_first, start, end, [&](const CopyRun &r) { printf(" %zu %ld %ld %ld", r.k, r.src_frame, r.dst_frame, r.count); return 0; });
            printf("\n");
            if (rc) return 4;
        } else return 2;
    }
    return 0;
}
"""


def compile_program(directory, extra_flags=()):
    """-> path of the program, or None without a host compiler or the HIP headers"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None or not os.path.isdir(ROCM_INCLUDE):
        return None
    src, exe = os.path.join(directory, "block_plan_cases.cpp"), os.path.join(directory, "block_plan_cases")
    with open(src, "w") as f:
        f.write(PROGRAM)
    r = subprocess.run([cxx] + COMPILE_FLAGS + list(extra_flags) + ["-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("block_plan"))
    exe = compile_program(d)
    if exe is None:
        pytest.skip("no host compiler or no HIP headers")
    return lambda cases: run_program(exe, d, cases)


G = int(re.search(r"constexpr int kDecodeChunk = (\d+);", open(os.path.join(CSRC, "mp3s_internal.h")).read()).group(1))


# ------------------------------------------------------------------------------------------------ (a) a rank's share
def test_the_share_is_the_one_of_sharded_py(program):
    sizes = [(total, world) for total in range(41) for world in range(1, 10)]
    sizes += [(total, world) for total in (16383, 16384, 16385, 10 ** 6) for world in (1, 2, 7, 64)]
    cases = [(0, total, rank, world) for total, world in sizes for rank in range(world)]
    got = iter(program(cases))
    for total, world in sizes:
        shares = [tuple(next(got)) for _ in range(world)]
        for rank, (first, count) in enumerate(shares):
            assert (first, count) == tuple(sharded.shard_frames(total, rank, world)) == tuple(shard.shard_frames(total, rank, world)[:2]), (total, rank, world)
        # the shares partition [0, total) in rank order, sizes differing by at most one
        at = 0
        for first, count in shares:
            assert first == at and count >= 0
            at += count
        assert at == total
        assert max(c for _, c in shares) - min(c for _, c in shares) <= 1


# ------------------------------------------------------------------------------------------------ (b) the window in front of a block
def reencode_block_window(first, count, n, dup):
    """mp3s_reencode_block_indexed: blocks of PCM frames, of which the repeated frame is the last -> (lead, halo, w0, n_win, with_dup), rows_frames"""
    total = n + (1 if dup else 0)
    lead = 1 if first > 0 else 0
    halo = 1 if first - lead > 0 else 0
    w0, w1 = first - lead - halo, min(first + count, n)
    with_dup = 1 if first + count == total and dup else 0
    return (lead, halo, w0, w1 - w0, with_dup), (w1 - w0) + with_dup


def chunk_window(first, count, decode):
    """chunk_window of pipe_internal.h -> (lead, halo, w0, n_win)"""
    lead = 1 if not decode and first > 0 else 0
    halo = 1 if first - lead > 0 else 0
    return lead, halo, first - lead - halo, count + lead + halo


def decode_block_window(first, count, n, dup):
    """mp3s_decode_block_indexed asked for {first - halo, count + halo, keep_dup = true}; front_end cut that down to the stream
    -> (halo, the window's first frame, its frames, whether the repeated frame follows), and the window as asked for"""
    halo = 1 if first > 0 else 0
    asked = (first - halo, count + halo, 1)
    w_first = min(max(asked[0], 0), n)
    w_count = min(max(asked[1], 0), n - w_first)
    return (halo, w_first, w_count, 1 if w_first + w_count >= n and dup else 0), asked


def test_the_window_is_the_three_callers(program):
    cases, want = [], []
    for n in (1, 2, 3, 4, 7, 16382):
        for dup in (0, 1):
            for first in sorted({0, 1, 2, n - 1} & set(range(n))):
                # (an encode block may hold the repeated frame: count up to n + dup - first; the last block with it and without it)
                for count in sorted({1, 2, n - first, n + dup - first}):
                    if first + count <= n + dup:
                        w, rows = reencode_block_window(first, count, n, dup)
                        assert rows == w[3] + w[4] and w[2] + w[3] <= n
                        cases.append((1, first, count, n, dup, 0)); want.append(w)
                    d, asked = decode_block_window(first, count, n, dup)
                    cases.append((1, first, count, n, dup, 1)); want.append((0, d[0], d[1], d[2], d[3]))
                    # ... which does not know the stream: it asks as if the block ended one that repeats its last frame
                    cases.append((1, first, count, first + count, 1, 1)); want.append((0, d[0]) + asked)
                    if first + count <= n:
                        for decode in (0, 1):
                            cases.append((1, first, count, first + count, 0, decode)); want.append(chunk_window(first, count, decode) + (0,))
    got = program(cases)
    for c, g, w in zip(cases, got, want):
        assert tuple(g) == tuple(w), c
    assert any(w[4] for w in want) and any(not w[4] for w in want) and any(w[0] for w in want) and any(w[1] and not w[0] for w in want)


# ------------------------------------------------------------------------------------------------ (c) transform groups
def decode_group_groups(n, stream_first):
    """decode_group: `stream_first` = per frame the first frame of its stream (the decoder's frame headers) -> (start, halo, cnt) per group"""
    out = []
    for start in range(0, n, G):
        halo = 1 if (start and stream_first(start) < start) else 0
        out.append((start, halo, min(G, n - start) + halo))
    return out


def issue_back_groups(n, halo0, firsts):
    """issue_back: `firsts` = j.stream_first -> (start, halo, cnt, last) per group"""
    def inside_stream(f):
        k = bisect.bisect_right(firsts, f)
        return k > 0 and firsts[k - 1] < f
    out = []
    for start in range(halo0, n, G):
        halo = halo0 if start == halo0 else (1 if inside_stream(start) else 0)
        out.append((start, halo, min(G, n - start) + halo, 1 if start + G >= n else 0))
    return out


def test_the_groups_are_the_two_loops(program):
    cases, expect_halo = [], []
    for n, halo0 in itertools.product((0, 1, G - 1, G, G + 1, 2 * G, 2 * G + 1), (0, 1)):
        if n < halo0:
            continue
        bounds = list(range(halo0 + G, n, G))                 # where a group behind the first begins
        layouts = [((0,), {})]
        for b in bounds:                                      # a stream that starts on the boundary, one frame before it, one behind it
            layouts += [((0, b), {b: 0}), ((0, b - 1), {b: 1})] + ([((0, b + 1), {b: 1})] if b + 1 < n else [])
        layouts.append(((0,) + tuple(bounds), {b: 0 for b in bounds}))
        for firsts, halos in layouts:
            firsts = tuple(sorted(set(firsts)))
            cases.append((2, n, halo0, len(firsts)) + firsts)
            expect_halo.append(halos)
    got = program(cases)
    ran = {0: 0, 1: 0, 2: 0, 3: 0}
    for (_, n, halo0, _, *firsts), g, halos in zip(cases, got, expect_halo):
        assert g[0] == G
        groups = [tuple(g[i:i + 4]) for i in range(1, len(g), 4)]
        assert groups == issue_back_groups(n, halo0, firsts), (n, halo0, firsts)
        if halo0 == 0:
            assert [x[:3] for x in groups] == decode_group_groups(n, lambda f: firsts[bisect.bisect_right(firsts, f) - 1]), (n, firsts)
        # the groups' own frames tile [halo0, n); one group is the last, or none ran
        at = halo0
        for k, (start, halo, cnt, last) in enumerate(groups):
            assert start == at and cnt - halo >= 1 and start - halo >= 0 and cnt <= G + 1
            assert halo == (halo0 if k == 0 else halos.get(start, 1)), (n, halo0, firsts, start)
            at += cnt - halo
        assert at == max(n, halo0)
        assert [x[3] for x in groups] == [0] * (len(groups) - 1) + [1] * (1 if groups else 0)
        assert bool(groups) == (n > halo0)
        ran[len(groups)] += 1
    assert ran[0] and ran[1] and ran[2] and ran[3]


# ------------------------------------------------------------------------------------------------ (d) the copy-out runs
def decode_group_runs(first_of, n_frames, dup, start, end):
    """the copy-out loop of decode_group -> extra, out_first, [(k, src frame, dst frame, count)]"""
    out_first, extra = [], 0
    for k in range(len(first_of)):
        out_first.append(first_of[k] + extra)
        extra += 1 if dup[k] else 0
    runs, a = [], start
    while a < end:
        k = bisect.bisect_right(first_of, a) - 1
        b = end
        j = k
        while j < len(first_of) and first_of[j] < end:
            if dup[j]:
                b = min(end, first_of[j] + n_frames[j])
                break
            j += 1
        if b <= a:
            b = min(end, a + 1)
        runs.append((k, a, out_first[k] + (a - first_of[k]), b - a))
        a = b
    return extra, out_first, runs


def run_windows(first_of, n_frames, dup, every):
    total = first_of[-1] + n_frames[-1]
    if every:
        return [(s, e) for s in range(total) for e in range(s + 1, total + 1)]
    ends = [f + n for f, n, d in zip(first_of, n_frames, dup) if d] or [first_of[-1]]
    e0 = ends[0]
    pick = {(0, total), (min(1, total - 1), total), (0, e0), (max(e0 - 1, 0), min(e0 + 1, total)), (e0, total), (min(e0 + 1, total), total),
            (first_of[1], first_of[2] + 1), (first_of[1] + n_frames[1] - 1, first_of[3] + n_frames[3] - 1), (max(ends[-1] - 1, 0), total)}
    return sorted((s, e) for s, e in pick if 0 <= s < e <= total)


def test_the_runs_are_decode_groups_and_copy_every_frame_once(program):
    """streams of 1..5 frames, every pattern of repeated last frames: up to three streams with every window [start, end), four streams with
    windows that begin and end inside a stream, at a repeating stream's end and one frame behind it"""
    layouts = []
    for n_streams in (1, 2, 3, 4):
        for n_frames in itertools.product(range(1, 6), repeat=n_streams):
            first_of = [sum(n_frames[:k]) for k in range(n_streams)]
            for dup in itertools.product((0, 1), repeat=n_streams):
                for start, end in run_windows(first_of, n_frames, dup, n_streams < 4):
                    layouts.append((first_of, n_frames, dup, start, end))
    cases = [(3, start, end, len(n_frames)) + tuple(x for nd in zip(n_frames, dup) for x in nd) for _, n_frames, dup, start, end in layouts]
    got = program(cases)
    split = 0
    for (first_of, n_frames, dup, start, end), g in zip(layouts, got):
        ns = len(n_frames)
        extra, out_first = g[0], g[1:1 + ns]
        runs = [tuple(g[i:i + 4]) for i in range(1 + ns, len(g), 4)]
        assert (extra, out_first, runs) == decode_group_runs(first_of, n_frames, dup, start, end), (n_frames, dup, start, end)
        assert extra == sum(dup) and out_first == [first_of[k] + sum(dup[:k]) for k in range(ns)]
        # frame by frame: frame f of stream k lands at out_first[k] + f - first_of[k], every frame of [start, end) once, in order
        at = start
        for k, src, dst, count in runs:
            assert src == at and count >= 1 and k == bisect.bisect_right(first_of, src) - 1
            for f in range(src, src + count):
                kf = bisect.bisect_right(first_of, f) - 1
                assert dst + (f - src) == out_first[kf] + f - first_of[kf], (n_frames, dup, start, end, f)
            # no run reaches past the last frame of a stream that repeats it
            for j in range(ns):
                if dup[j]:
                    assert not (src < first_of[j] + n_frames[j] < src + count), (n_frames, dup, start, end)
            at += count
        assert at == end
        split += len(runs) > 1
    assert split > len(layouts) // 8


def test_the_rules_are_stated_once():
    """the callers ask block_plan.h: no share, lead / halo or group arithmetic is left in them"""
    src = {f: open(os.path.join(CSRC, f)).read() for f in ("mp3s_encode_pipeline.cpp", "mp3s_decode_pipeline.cpp", "pipe_jobs.cpp", "pipe_internal.h", "run_file.cpp")}
    for name, text in src.items():
        assert not re.search(r"\brem\b|% *(j\.)?world", text), name                       # the share
        assert not re.search(r"\b(lead|halo) *= *[^;]*first\w* *(-[^;]*)?> *0", text), name    # lead / halo from a first frame
        assert not re.search(r"start *\+= *kDecodeChunk|start \+ kDecodeChunk", text), name  # the walk over groups
    assert len(re.findall(r"block_share\(", src["mp3s_encode_pipeline.cpp"] + src["pipe_jobs.cpp"])) == 2
    assert len(re.findall(r"block_window\(", "".join(src.values()))) == 3
    assert len(re.findall(r"for_transform_groups\(", src["mp3s_decode_pipeline.cpp"] + src["pipe_jobs.cpp"])) == 2
    assert len(re.findall(r"for_copy_runs\(", src["mp3s_decode_pipeline.cpp"])) == 1
