"""The packer that lays out a pipe slot's packed inputs (csrc/pipe_pack.h) with the records it packs (SmallHead: csrc/mp3s_internal.h,
PlaceEntry: csrc/mp3s_device.h), on the CPU: a stand-alone program states the four layouts as the preparers of csrc/pipe_jobs.cpp do and
prints the offsets; they are compared with the arithmetic those preparers had before the packer existed -- their chains of up16, written out
here.  Same offsets = same upload sizes, byte for byte the same staged block."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mp3-steganography-lib_amd", "csrc")
ROCM_INCLUDE = "/opt/rocm/include"

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "mp3s_internal.h"
#include "pipe_pack.h"

// argv: layout o_in bound n_streams n_fix n_frames enc_bytes rec_bytes
int main(int argc, char **argv)
{
    if (argc != 9) return 2;
    const char kind = argv[1][0];
    const size_t o_in = strtoull(argv[2], nullptr, 0), bound = strtoull(argv[3], nullptr, 0);
    const int ns = atoi(argv[4]);
    const size_t n_fix = strtoull(argv[5], nullptr, 0), n = strtoull(argv[6], nullptr, 0), enc = strtoull(argv[7], nullptr, 0), rec = strtoull(argv[8], nullptr, 0);
    size_t o_small = 0, o_encblk = 0, o_fix = 0, o_refs = 0, o_streams = 0, front_end = 0;
    StagePacker pk;
    pk.begin(o_in, bound);
    if (kind == 'w') {          // walked list job: [small | encoder inputs | place entries | refs | streams]
        o_small = pk.add(small_bytes(ns));
        o_encblk = pk.add(0);
        pk.add(enc);
        o_fix = pk.add(n_fix * sizeof(PlaceEntry));
        o_refs = pk.add(n * sizeof(FrameRef));
        o_streams = pk.add((size_t)ns * sizeof(StreamRef));
    } else if (kind == 'c') {   // chunk: [small | place entry | refs | stream || encoder inputs]
        o_small = pk.add(small_bytes(1));
        o_fix = pk.add(n_fix * sizeof(PlaceEntry));
        o_refs = pk.add(n * sizeof(FrameRef));
        o_streams = pk.add(sizeof(StreamRef));
        o_encblk = front_end = pk.add(0);
        pk.add(enc);
    } else if (kind == 'e') {   // encode job: [small | encoder inputs | gather records]
        o_small = pk.add(small_bytes(ns));
        o_encblk = pk.add(0);
        pk.add(enc);
        o_refs = pk.add(rec);   // (printed in the refs column: where the records begin)
    } else if (kind == 's') {   // scanned job, the part the packer lays out: [dec headers, encoder inputs]
        pk.add(n * sizeof(mp3s_frame_hdr));
        o_encblk = pk.add(0);
        pk.add(enc);
    } else return 2;
    printf("%zu %zu %zu %zu %zu %zu %zu %d\n", o_small, o_encblk, o_fix, o_refs, o_streams, front_end, pk.end(), pk.ok ? 1 : 0);
    return 0;
}
"""


def up16(x):
    return (x + 15) & ~15


SMALL_HEAD, SEG_OUT, PLACE_ENTRY, FRAME_REF, STREAM_REF, FRAME_HDR = 32, 80, 4912, 16, 40, 8


def parent_walk(o_in, ns, n_fix, n, enc):
    """prepare_walk (hide job: one mp3s_chain_seg_out per stream)"""
    o_small = o_in
    o_encblk = o_small + up16(SMALL_HEAD + ns * SEG_OUT)
    o_fix = up16(o_encblk + enc)
    o_refs = up16(o_fix + n_fix * PLACE_ENTRY)
    o_streams = up16(o_refs + n * FRAME_REF)
    return [o_small, o_encblk, o_fix, o_refs, o_streams, 0, o_streams + ns * STREAM_REF]


def parent_chunk(o_in, n_fix, n, enc):
    """prepare_chunk, then prepare_chunk_encode"""
    o_small = o_in
    o_fix = o_small + up16(SMALL_HEAD + SEG_OUT)
    o_refs = up16(o_fix + n_fix * PLACE_ENTRY)
    o_streams = up16(o_refs + n * FRAME_REF)
    o_encblk = up16(o_streams + STREAM_REF)
    return [o_small, o_encblk, o_fix, o_refs, o_streams, o_encblk, o_encblk + enc]


def parent_encode(o_in, ns, enc, rec):
    """prepare_encode; WavBatch::place_records(base) begins the records at up16(base)"""
    o_small = o_in
    o_encblk = o_small + up16(SMALL_HEAD + ns * SEG_OUT)
    o_runs = up16(o_encblk + enc)
    return [o_small, o_encblk, 0, o_runs, 0, 0, o_runs + rec]


def parent_scan(o_in, n, enc):
    """prepare_fast: the encoder's inputs behind the decoder's frame headers"""
    o_enc = up16(n * FRAME_HDR)
    return [0, o_in + o_enc, 0, 0, 0, 0, o_in + o_enc + enc]


@pytest.fixture(scope="module")
def packer(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None or not os.path.isdir(ROCM_INCLUDE):
        pytest.skip("no host compiler or no HIP headers")
    d = tmp_path_factory.mktemp("packer")
    src = d / "packer.cpp"
    src.write_text(PROGRAM)
    exe = d / "packer"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", ROCM_INCLUDE, "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(kind, o_in, bound, ns=1, n_fix=0, n=1, enc=0, rec=0):
        out = subprocess.run([str(exe), kind] + [str(v) for v in (o_in, bound, ns, n_fix, n, enc, rec)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        v = [int(w) for w in out.stdout.split()]
        return v[:7], bool(v[7])
    return run


O_IN = 0x123450       # a slot's o_in is a multiple of 16
ENC = (16 * 37, 16 * 37 + 4)
FRAMES = (1, 7, 1000)


def test_the_four_layouts_have_the_parents_offsets(packer):
    far = 1 << 40
    for ns, n_fix, n, enc in itertools.product((1, 3), (0, 2), FRAMES, ENC):
        assert packer("w", O_IN, far, ns, n_fix, n, enc) == (parent_walk(O_IN, ns, n_fix, n, enc), True), (ns, n_fix, n, enc)
    for n_fix, n, enc in itertools.product((0, 1), FRAMES, ENC):
        assert packer("c", O_IN, far, 1, n_fix, n, enc) == (parent_chunk(O_IN, n_fix, n, enc), True), (n_fix, n, enc)
    for ns, enc in itertools.product((1, 3), ENC):
        # gather records: one WavRun of 16 bytes per file; import records: 32
        for rec in (ns * 16, ns * 32):
            assert packer("e", O_IN, far, ns, 0, 0, enc, rec) == (parent_encode(O_IN, ns, enc, rec), True), (ns, enc, rec)
    for n, enc in itertools.product(FRAMES, ENC):
        assert packer("s", O_IN, far, 1, 0, n, enc) == (parent_scan(O_IN, n, enc), True), (n, enc)


def test_a_part_one_byte_over_the_bound_fails(packer):
    for kind, args, end in (("w", (3, 2, 7, ENC[1]), parent_walk(O_IN, 3, 2, 7, ENC[1])[6]),
                            ("c", (1, 1, 7, ENC[1]), parent_chunk(O_IN, 1, 7, ENC[1])[6]),
                            ("e", (3, 0, 0, ENC[1], 48), parent_encode(O_IN, 3, ENC[1], 48)[6]),
                            ("s", (1, 0, 7, ENC[1]), parent_scan(O_IN, 7, ENC[1])[6])):
        assert packer(kind, O_IN, end, *args)[1] is True            # the last part ends at the bound
        assert packer(kind, O_IN, end - 1, *args)[1] is False       # ... one byte behind it
    # ... and a part in the middle: the refs of a walked job end one byte behind the bound, what follows would fit a larger one
    w = parent_walk(O_IN, 1, 0, 7, ENC[0])
    assert packer("w", O_IN, w[3] + 7 * FRAME_REF - 1, 1, 0, 7, ENC[0])[1] is False
