"""The decode transform at its parameter edges (tests/decode_edges.py): the quick path's table boundary, both ends of the gain tables,
every pair of per-channel cases, every block-type transition, a loud granule among quiet ones, a sweep of every line across the boundary.

CPU half: the oracle's stage chain equals the upstream reference's own functions on every frame of the case set
(tests/golden/g14_decode_edges.npz, made by tests/golden/gen_decode_edges_golden.py), and the cases reach what they are meant to reach.
GPU half: the device equals the fixture (float64) and the oracle chain (float32, int16 under every option that chooses other kernels)."""
import contextlib
import os

import numpy as np
import pytest

import decode_edges as E

OPTION_SETS = [dict(), dict(fused_decode=0), dict(fast_imdct=0)]
OPTION_IDS = ["defaults", "fused_decode=0", "fast_imdct=0"]


@pytest.fixture(scope="module")
def fix(golden_dir):
    g = np.load(os.path.join(golden_dir, "g14_decode_edges.npz"))
    names = [str(s) for s in g["case_names"]]
    start = np.concatenate([[0], np.cumsum(g["n_frames"])])
    return {"names": names, "in_digest": dict(zip(names, g["in_digest"].tolist())),
            "frame_digest": {n: g["frame_digest"][start[i]:start[i + 1]] for i, n in enumerate(names)},
            "first_frame": {n: g["first_frame_%d" % i] for i, n in enumerate(names)}}


@pytest.fixture(scope="module")
def refs(orc):
    """the oracle chain over every case, computed once and shared (read-only)"""
    out = {}
    for name, case in E.cases().items():
        out[name] = E.oracle_chain(orc, *case)
        out[name].setflags(write=False)
    return out


@contextlib.contextmanager
def options(ctx, **kw):
    old = {k: ctx.get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            ctx.set_option(k, v)


def first_difference(name, got, ref):
    """'' when the arrays hold the same bits, or where they first differ"""
    if got.shape != ref.shape:
        return "%s: shape %s against %s" % (name, got.shape, ref.shape)
    a, b = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    rows = np.nonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))[0]
    if not len(rows):
        return ""
    r = int(rows[0])
    return "%s: %d rows differ, the first in frame %d, granule %d, row %d: got %r, expected %r" % (
        name, len(rows), r // 1152, r % 1152 // 576, r % 576, a[r].tolist(), b[r].tolist())


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_builders_reproduce_the_fixture_inputs(fix):
    cases = E.cases()
    assert list(cases) == fix["names"]
    for name, case in cases.items():
        isv, si, hdr, nch = case
        assert np.abs(isv.astype(np.int32)).max() <= E.IS_MAX
        assert not si["scale_fac_l"][..., 21].any() and not si["scale_fac_s"][..., 12].any()
        assert E.input_digest(case) == fix["in_digest"][name], name
    print("frames:", {n: len(c[2]) for n, c in cases.items()}, "in all", sum(len(c[2]) for c in cases.values()))


def test_oracle_chain_equals_the_reference(fix, refs):
    for name in fix["names"]:
        pcm = refs[name]
        assert first_difference(name + " first frame", pcm[:1152], fix["first_frame"][name]) == ""
        d = E.frame_digests(pcm)
        assert len(d) == len(fix["frame_digest"][name])
        bad = np.nonzero(d != fix["frame_digest"][name])[0]
        assert not len(bad), (name, "frames", bad.tolist())


def test_gain_range_leaves_the_int16_comparison_something_to_say(refs):
    assert np.abs(refs["gain_range"] * 32767).max() < 2.0 ** 31
    assert np.abs(refs["loud_among_quiet"] * 32767).max() >= 2.0 ** 31        # (that one is meant to go beyond)


def test_table_boundary_has_a_pair_on_either_side():
    """each boundary of the quick path's test decides between two granules that are identical but for one line, at every position and rate"""
    for mode, nch in (("stereo", 2), ("ms", 2), ("mono", 1)):
        case = E.cases()["table_boundary/" + mode]
        isv, si, hdr, _ = case
        for lo, hi, quick_lo in ((511, 512, True), (-513, -512, False)):
            pairs = E.boundary_pairs(case, lo, hi)
            for (fa, ga), (fb, gb), ch, line in pairs:
                assert hdr["sr_idx"][fa] == hdr["sr_idx"][fb]
                assert E.quick(isv[fa, ga], si[fa, ga], nch) == quick_lo and E.quick(isv[fb, gb], si[fb, gb], nch) == (not quick_lo)
            want = {(0, 0), (0, 575)} | ({(1, 0), (1, 575), (1, 288)} if nch == 2 else set())
            assert {(ch, line) for _, _, ch, line in pairs} == want, (mode, lo, hi)
        # the boundary at the other sampling rates
        assert {int(hdr["sr_idx"][fa]) for (fa, _), _, _, _ in E.boundary_pairs(case, 511, 512)} == {0, 1, 2}
        # the neighbours that must not decide anything: -511 and 511 stay quick, 513 and -513 do not
        for v, q in ((-511, True), (513, False)):
            hits = [(f, g) for f in range(len(hdr)) for g in range(2) if (isv[f, g, :nch] == v).any()]
            assert hits and all(E.quick(isv[f, g], si[f, g], nch) == q for f, g in hits)


def test_gain_tables_are_reached_end_to_end():
    cases = E.cases()
    assert E.exp1_values(cases["gain_range"]) == set(range(-266, 46))
    _, si, _, _ = cases["gain_range"]
    long_gg = sorted(int(r["global_gain"]) for r in si.reshape(-1) if E.case_of(int(r["block_type"]), int(r["mixed_block_flag"])) == 0)
    assert long_gg == list(range(256))                                          # every global_gain once in a long granule
    short = [r for r in si.reshape(-1) if int(r["block_type"]) == 2]
    assert {(w, int(r["sub_block_gain"][w])) for r in short for w in range(3)} == {(w, s) for w in range(3) for s in range(8)}
    assert {(0, 7), (255, 0)} <= {(int(r["global_gain"]), int(s)) for r in short for s in r["sub_block_gain"]}
    # 2 * exp2 = scalefac_scale's 1 | 2 times (scalefactor <= 15 + preflag * pre_tab <= 3): 0..18 and the even values up to 36 exist
    assert E.k2_values(cases["exponent_top"]) == set(E.K2_REACHABLE) and max(E.K2_REACHABLE) == 36


def test_case_pairs_and_transitions_are_complete():
    cases = E.cases()
    for mode, ms in (("stereo", 0), ("ms", 1)):
        isv, si, hdr, _ = cases["case_pairs/" + mode]
        kinds = {((int(si["block_type"][f, g, 0]), int(si["mixed_block_flag"][f, g, 0])), (int(si["block_type"][f, g, 1]), int(si["mixed_block_flag"][f, g, 1])))
                 for f in range(len(hdr)) for g in range(2)}
        assert kinds == {(a, b) for a in E.KINDS for b in E.KINDS}
        assert (hdr["ms_stereo"] == ms).all()
        census = E.case_pair_census(cases["case_pairs/" + mode])
        for a in range(3):
            for b in range(3):
                assert all(census[(a, b, ms, sr, False)] + census[(a, b, ms, sr, True)] for sr in range(3)), (a, b)
                assert all(sum(census[(a, b, ms, sr, big)] for sr in range(3)) for big in (False, True)), (a, b)
    _, si, hdr, _ = cases["case_pairs/mono"]
    assert {(int(si["block_type"][f, g, 0]), int(si["mixed_block_flag"][f, g, 0])) for f in range(len(hdr)) for g in range(2)} == set(E.KINDS)
    for mode, nch in (("stereo", 2), ("ms", 2), ("mono", 1)):
        _, si, hdr, _ = cases["transitions/" + mode]
        assert len(set(hdr["stream_first"].tolist())) == 1
        for ch in range(nch):
            bt = si["block_type"][:, :, ch].reshape(-1).tolist()
            assert set(zip(bt, bt[1:])) == {(a, b) for a in range(4) for b in range(4)}, (mode, ch)


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_device_float64_equals_the_reference_digests(ctx, mlib, fix, refs):
    for name, (isv, si, hdr, nch) in E.cases().items():
        pcm = ctx.decode_transform(isv, si, hdr, nch, 0, mlib.MP3S_PCM_F64)
        if not np.array_equal(E.frame_digests(pcm), fix["frame_digest"][name]):
            raise AssertionError(first_difference(name, pcm, refs[name]) or name + ": equals the oracle chain, not the fixture")


@pytest.mark.gpu
def test_device_float32_equals_the_oracle_rounded_once(ctx, mlib, refs):
    assert ctx.get_option("float_fast") == 0
    for name, (isv, si, hdr, nch) in E.cases().items():
        pcm = ctx.decode_transform(isv, si, hdr, nch, 0, mlib.MP3S_PCM_F32)
        assert first_difference(name, pcm, refs[name].astype(np.float32)) == ""


@pytest.mark.gpu
@pytest.mark.parametrize("opts", OPTION_SETS, ids=OPTION_IDS)
def test_device_int16_equals_the_oracle(ctx, mlib, orc, refs, opts):
    with options(ctx, **opts):
        for name, (isv, si, hdr, nch) in E.cases().items():
            ctx.synth_mode(1.0)                                                 # (the proven bound, the default; reads and clears the count)
            pcm = ctx.decode_transform(isv, si, hdr, nch, 0, mlib.MP3S_PCM_I16)
            exact_samples = ctx.synth_mode(1.0)
            assert first_difference(name, pcm, orc.pcm_to_i16(refs[name])) == ""
            if name == "loud_among_quiet":
                print("exact_samples", opts, exact_samples)
                assert exact_samples > 0


@pytest.mark.gpu
def test_device_float_fast_within_the_contract(ctx, mlib, refs):
    worst = {}
    with options(ctx, float_fast=1):
        for name, (isv, si, hdr, nch) in E.cases().items():
            pcm = ctx.decode_transform(isv, si, hdr, nch, 0, mlib.MP3S_PCM_F32)
            ref = refs[name]
            worst[name] = float(np.abs(pcm.astype(np.float64) - ref).max() / max(1.0, np.abs(ref).max()))
    print("float_fast, largest difference over max(1, max|ref|):", worst)
    for name, w in worst.items():
        assert w <= 1e-5, (name, w)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["stereo", "ms", "mono"])
def test_device_streams_of_a_batch_decode_as_alone(ctx, mlib, orc, refs, mode):
    """case_pairs is three streams (one per sampling rate) in one batch: each of them alone gives the same rows"""
    name = "case_pairs/" + mode
    isv, si, hdr, nch = E.cases()[name]
    starts = sorted(set(hdr["stream_first"].tolist()))
    assert len(starts) == 3
    for fmt, ref in ((mlib.MP3S_PCM_F64, refs[name]), (mlib.MP3S_PCM_I16, orc.pcm_to_i16(refs[name]))):
        whole = ctx.decode_transform(isv, si, hdr, nch, 0, fmt)
        assert first_difference(name, whole, ref) == ""
        for a, b in zip(starts, starts[1:] + [len(hdr)]):
            h = hdr[a:b].copy()
            h["stream_first"] = 0
            alone = ctx.decode_transform(isv[a:b], si[a:b], h, nch, 0, fmt)
            assert first_difference("%s frames %d..%d alone" % (name, a, b), alone, whole[a * 1152:b * 1152]) == ""


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["stereo", "ms", "mono"])
def test_device_halo_behind_short_mixed_and_stop_frames(ctx, mlib, orc, refs, mode):
    """a chunk decoded with one frame of halo equals the same rows of the whole decode, where the halo frame ends in a block_type 2,
    a mixed and a stop (block_type 3) granule"""
    name = "transitions/" + mode
    isv, si, hdr, nch = E.cases()[name]
    last = si[:, 1, :nch]                                                       # the halo frame's second granule
    wanted = {"short": (last["block_type"] == 2).any(axis=1), "mixed": (last["mixed_block_flag"] != 0).any(axis=1),
              "stop": ((last["block_type"] == 3) & (last["mixed_block_flag"] == 0)).any(axis=1)}
    for fmt, ref in ((mlib.MP3S_PCM_F64, refs[name]), (mlib.MP3S_PCM_I16, orc.pcm_to_i16(refs[name]))):
        for what, mask in wanted.items():
            halo = [int(f) for f in np.nonzero(mask[:-1])[0]]
            assert halo, (mode, what)
            for f in (halo[0], halo[-1]):
                part = ctx.decode_transform(isv[f:], si[f:], hdr[f:], nch, 1, fmt)
                assert first_difference("%s behind %s frame %d" % (name, what, f), part, ref[(f + 1) * 1152:]) == ""


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [k for k, _, _ in E.SWEEP_KINDS])
@pytest.mark.parametrize("sr", [0, 1, 2])
def test_device_line_sweep_across_the_table_boundary(ctx, mlib, orc, sr, kind):
    """every line of ch 0 and, mirrored, of ch 1 alone in a granule, alternately just inside and just outside the small table: the line
    maps, the reorder and the edge subbands of the alias butterflies line by line, against the oracle"""
    isv, si, hdr, nch = E.line_sweep(sr, kind)
    ref = E.oracle_chain(orc, isv, si, hdr, nch)
    pcm = ctx.decode_transform(isv, si, hdr, nch, 0, mlib.MP3S_PCM_F64)
    assert first_difference("sweep %d %s f64" % (sr, kind), pcm, ref) == ""
    i16 = ctx.decode_transform(isv, si, hdr, nch, 0, mlib.MP3S_PCM_I16)
    assert first_difference("sweep %d %s i16" % (sr, kind), i16, orc.pcm_to_i16(ref)) == ""
