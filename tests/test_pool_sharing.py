"""The call families that share device buffers of one context's pool (PoolSlot, csrc/mp3s_internal.h), one after the other on ONE
Context and then again with larger files: encode_files, table_audits, pcm_distortions, pcm_alignments, capacities, reveal_messages,
hide_messages, decode_streams, a hide job and an encode job of a Pipe on that context, and the test aids capacity_dev, table_audit_dev
and pcm_diff_dev.  The first round has two files of 12 and 13 frames; the second three of 40 to 42, one of them mono, which is more
than the 25 % of head room a buffer is made with: every shared buffer is made anew between a writer and its next reader.

Every answer is compared exactly -- bytes, arrays and every field -- with the same call on a Context of its own, and with the oracle
(tests/oracle_lib.py), numpy on the oracle's decode or tests/table_audit_model.py where a committed helper computes it."""
import functools

import numpy as np
import pytest

import frame_synth as F
import table_audit_model as M
from synth_pcm import synth_pcm
from test_capacity import oracle_clear_capacity
from test_list_calls_foreign import oracle_decodes
from test_pcm_alignment import check_alignment, expect_alignment
from test_pcm_distortion import check_pair, expect_pairs
from test_table_audit import same as same_audit
from test_vbr_streams import expect_hide, oracle_i16

gpu = pytest.mark.gpu
RATE, KBPS = 44100, 128
ROUNDS = [dict(stereo=[12, 13], mono=None), dict(stereo=[40, 42], mono=41)]
MAX_LAG, SEARCH_ROWS = 64, 1152


@functools.lru_cache(maxsize=None)
def round_inputs(k):
    """the inputs of round k, made on the host: WAV files, the oracle's encodes of them (stereo MP3 files), a mono stream of
    tests/frame_synth.py, a message (or None) per file"""
    import oracle_lib
    from mp3stego import _lib
    r = ROUNDS[k]
    pcm = [synth_pcm(n, seed=7300 + 10 * k + i) for i, n in enumerate(r["stereo"])]
    wavs = [_lib.wav_header(len(p), 2, RATE) + p.tobytes() for p in pcm]
    stereo = [oracle_lib.encode(p, RATE, KBPS)["mp3"] for p in pcm]
    mono = [] if r["mono"] is None else [F.make_stream(7390 + k, r["mono"], mode=3)]
    messages = ["pool sharing, round %d" % k] + [None] * (len(stereo) - 1)
    return {"pcm": pcm, "wavs": wavs, "stereo": stereo, "mono": mono, "mp3s": stereo + mono, "messages": messages}


def same(a, b, where):
    """a == b through dicts, lists, arrays (type, shape and bytes), byte strings and the errors of single files"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), where
        for k in a:
            same(a[k], b[k], (where, k))
    elif isinstance(a, (list, tuple)):
        assert isinstance(b, (list, tuple)) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, (where, i))
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where
    elif isinstance(a, Exception):
        assert type(a) is type(b) and getattr(a, "code", None) == getattr(b, "code", None), (where, a, b)
    elif isinstance(a, (bytes, bytearray, memoryview)):
        assert bytes(a) == bytes(b), where
    elif isinstance(a, float):
        assert a == b or (a != a and b != b), (where, a, b)
    else:
        assert type(a) is type(b) and a == b, (where, a, b)


def alone(mlib, call):
    """call(c) on a Context of its own"""
    c = mlib.Context(0)
    try:
        return call(c)
    finally:
        c.close()


def pipe_jobs(mlib, c, x):
    """a hide job and an encode job in flight together on a pipe of c -> their results, with the bytes copied out of the pipe's blocks"""
    p = mlib.Pipe(c, depth=2, max_job_bytes=1 << 20, scan_threads=1, max_files=8)
    try:
        t_hide = p.submit(x["stereo"], x["messages"])
        t_enc = p.submit_encode(x["wavs"], KBPS, messages=x["messages"])
        assert t_hide is not None and t_enc is not None
        out = []
        for t in (t_hide, t_enc):
            got_t, files = p.collect()
            assert got_t == t
            out.append([f if isinstance(f, Exception) else {k: bytes(v) if k == "data" else v for k, v in f.items() if k != "bits"} for f in files])
        print("pipe:", p.stats())
        return out
    finally:
        p.close()


def dev_inputs(mlib, x, k):
    """what the three test aids are given: records of noise as in tests/test_capacity.py, the host parse of the round's files, two
    int16 buffers"""
    rng = np.random.default_rng(7400 + k)
    lengths = [len(p) // 1152 for p in x["pcm"]]
    n = sum(lengths)
    gr = np.frombuffer(rng.integers(-2 ** 31, 2 ** 31, size=n * 4 * 18, dtype=np.int64).astype("<i4").tobytes(), dtype=mlib.GR_OUT_DTYPE).copy()
    gr["n_tables"] = rng.integers(0, 4, size=n * 4)
    gr["flags"] = rng.integers(0, 2, size=n * 4)
    segs = np.zeros(len(lengths), dtype=mlib.CHAIN_SEG_DTYPE)
    segs["n_frames"], segs["first_frame"] = lengths, np.cumsum([0] + lengths[:-1])
    parsed, scanned = [mlib.parse_stream(f) for f in x["stereo"]], [mlib.scan_stream(f) for f in x["stereo"]]
    asegs = np.array(list(zip(np.cumsum([0] + lengths[:-1]), lengths)), dtype=mlib.TABLE_AUDIT_SEG_DTYPE)
    pcm = np.concatenate(x["pcm"] + [x["pcm"][0][::-1]])
    m = min(lengths)
    pairs = np.zeros(2, dtype=mlib.PCM_PAIR_DTYPE)
    pairs["a_first"], pairs["b_first"], pairs["n_frames"], pairs["out_first"] = [0, 0], [lengths[0], n], [m, lengths[0]], [0, m]
    return {"gr": gr, "segs": segs, "is": np.concatenate([p["is"] for p in parsed]), "side": np.concatenate([s["side"] for s in scanned]),
            "asegs": asegs, "pcm": pcm, "pairs": pairs}


def calls(mlib, x, k):
    """name -> call(c), in the order of the round"""
    a, b = x["stereo"] + x["mono"], x["stereo"][::-1] + x["mono"]    # the pair calls: each stereo file against the other, the mono stream against itself
    d = dev_inputs(mlib, x, k)
    return {
        "encode_files": lambda c: c.encode_files(x["wavs"], KBPS, messages=x["messages"]),
        "table_audits": lambda c: c.table_audits(x["mp3s"], profile=True),
        "pcm_distortions": lambda c: c.pcm_distortions(a, b, profile=True),
        "pcm_alignments": lambda c: c.pcm_alignments(a, b, max_lag=MAX_LAG, search_rows=SEARCH_ROWS, profile=True),
        "capacities": lambda c: c.capacities(x["mp3s"], None, profile=True),
        "reveal_messages": lambda c: c.reveal_messages(x["mp3s"]),
        "hide_messages": lambda c: c.hide_messages(x["mp3s"], x["messages"] + [None] * len(x["mono"])),
        "decode_streams": lambda c: c.decode_streams(x["mp3s"], per_file=True),
        "pipe": lambda c: pipe_jobs(mlib, c, x),
        "capacity_dev": lambda c: c.capacity_dev(d["gr"], d["segs"], profile=True),
        "table_audit_dev": lambda c: c.table_audit_dev(d["is"], d["side"], d["asegs"], 2),
        "pcm_diff_dev": lambda c: c.pcm_diff_dev(d["pcm"], d["pairs"], 2),
    }, a, b


def check_against_oracle(mlib, orc, x, a, b, got):
    """the answers of a round against what the committed helpers compute without a device"""
    dec = oracle_decodes(orc)
    o = {f: dec.known.setdefault(f, orc.decode(f)) for f in x["mp3s"]}
    assert all(v["rc"] == 0 for v in o.values())
    n_st = len(x["stereo"])
    for i, (r, pcm, msg) in enumerate(zip(got["encode_files"], x["pcm"], x["messages"])):
        e = orc.encode(pcm, RATE, KBPS, None if msg is None else np.array(mlib.message_frame(msg)))
        assert bytes(r["data"]) == e["mp3"] and (r["hide_offset"], r["too_long"]) == (e["hide_offset"], e["too_long"]), ("encode_files", i)
        assert msg is not None or bytes(r["data"]) == x["stereo"][i], ("encode_files", i)
    for i, (f, r) in enumerate(zip(x["mp3s"], got["table_audits"])):
        same_audit(r, M.audit_file(mlib, f), ("table_audits", i))
    want = expect_pairs(dec, a, b)
    for i, (r, w) in enumerate(zip(got["pcm_distortions"], want)):
        check_pair(("pcm_distortions", i), r, w)
    for i, r in enumerate(got["pcm_alignments"]):
        check_alignment(("pcm_alignments", i), r, expect_alignment(dec, a[i], b[i], MAX_LAG, SEARCH_ROWS))
    for i, (f, r) in enumerate(zip(x["mp3s"], got["capacities"])):
        if i >= n_st:
            assert isinstance(r, mlib.Mp3sError), ("capacities", i, r)
            continue
        w = oracle_clear_capacity(orc, mlib, o[f])
        assert (r["bits"], r["active_units"], r["n_frames"]) == (w["bits"], w["active_units"], o[f]["n_frames"]), ("capacities", i)
        assert np.array_equal(r["profile"], w["profile"]), ("capacities", i)
    for i, (f, r) in enumerate(zip(x["mp3s"], got["reveal_messages"])):
        assert np.array_equal(r["bits"], o[f]["bits"]) and r["data"] == mlib.message_reveal(o[f]["bits"]), ("reveal_messages", i)
        assert (r["n_frames"], r["channels"]) == (o[f]["n_frames"], o[f]["channels"]), ("reveal_messages", i)
    hidden = [expect_hide(orc, mlib, o[f], m) for f, m in zip(x["stereo"], x["messages"])]
    for name, res in (("hide_messages", got["hide_messages"]), ("pipe hide job", got["pipe"][0])):
        for i, (r, e) in enumerate(zip(res, hidden)):
            assert bytes(r["data"]) == e["mp3"], (name, i)
            assert x["messages"][i] is None or (r["hide_offset"], r["too_long"]) == (e["hide_offset"], e["too_long"]), (name, i)
    assert all(isinstance(r, mlib.Mp3sError) for r in got["hide_messages"][n_st:])
    for i, (f, r) in enumerate(zip(x["mp3s"], got["decode_streams"])):
        assert np.array_equal(r["pcm"], oracle_i16(o[f])) and (r["n_frames"], r["channels"]) == (o[f]["n_frames"], o[f]["channels"]), ("decode_streams", i)
    for i, (r, e) in enumerate(zip(got["pipe"][1], got["encode_files"])):        # (the encode job: what encode_files gave, which is the oracle's)
        same(r, {k: bytes(v) if k == "data" else v for k, v in e.items() if k != "bits"}, ("pipe encode job", i))


@gpu
def test_call_families_share_one_context(mlib, orc):
    shared = mlib.Context(0)
    try:
        for k in range(len(ROUNDS)):
            x = round_inputs(k)
            todo, a, b = calls(mlib, x, k)
            got = {name: call(shared) for name, call in todo.items()}
            for name, call in todo.items():
                same(got[name], alone(mlib, call), (k, name))
            check_against_oracle(mlib, orc, x, a, b, got)
    finally:
        shared.close()
