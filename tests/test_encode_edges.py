"""The encode transform (k_enc_analysis / k_enc_mdct / k_enc_fused, csrc/k_encode.hpp) where the reference's int32 arithmetic wraps and
where the kernels' tiles and workgroups end, against what the upstream reference ITSELF answered: tests/golden/g17_encode_edges.npz
(tests/golden/gen_encode_edges_golden.py) on the streams of tests/encode_edges.py.  Every comparison is equality of bits.

CPU: the exact model of tests/encode_edges.py equals the reference's __mdct_freq on every frame, so its flags may speak about the reference;
the conditions the fixture is for hold on the reference's records (a wrapped MDCT sum in every band and of both signs, butterfly results
beyond int32 without a wrapped sum, the largest subband sample, no line at -2^31); the oracle equals everything recorded, the refusal too.
GPU: every stream alone and in batches that reach every remainder and boundary the kernels distinguish, under both forms of the transform
and both matrixings, and the whole encoder downstream of the wrapped lines.

Census of the fixture (printed by test_conditions_hold_on_the_reference): 44 MDCT sums above 2^31 - 1 and 45 below -2^31 over the 29 streams,
in every band; 12 butterfly results beyond int32 in granules without a wrapped sum, at the band edges 1, 16 and 31; the reference refuses
one run, analysis_max at 32 kbit/s (IndexError in frame 0)."""
import contextlib
import hashlib
import os

import numpy as np
import pytest

import encode_edges as E

OPTIONS = [(fused, shared) for fused in (0, 1) for shared in (0, 1)]


@pytest.fixture(scope="module")
def g17(golden_dir):
    g = np.load(os.path.join(golden_dir, "g17_encode_edges.npz"))
    return {k: g[k] for k in g.files}


def run_of(g17, name, kbps):
    names = [str(n) for n in g17["names"]]
    return int(np.nonzero((g17["run_stream"] == names.index(name)) & (g17["run_kbps"] == kbps))[0][0])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest()


_REFERENCE = {}


def reference_mdct(g17, name):
    """the reference's __mdct_freq of a stream, int32 [frame][ch][gr][576]: the model's values, once every frame of them has the fixture's
    digest (in every run of the stream) and equals the frames the fixture holds whole"""
    if name not in _REFERENCE:
        names = [str(n) for n in g17["names"]]
        si = names.index(name)
        assert bytes(g17["pcm_sha256"][si]) == sha(E.streams()[name].pcm.astype("<i2")), "%s: the builder no longer makes the fixture's samples" % name
        v = E.stream_model(name)["value"]
        for r in np.nonzero(g17["run_stream"] == si)[0]:
            for f in range(E.FRAMES):
                assert bytes(g17["mdct_sha256"][r, f]) == sha(v[f].astype("<i4")), "%s frame %d: the model is not the reference" % (name, f)
        for (s, f), whole in zip(g17["mdct_full_at"], g17["mdct_full"]):
            if s == si:
                bad = np.argwhere(whole != v[f])
                assert not len(bad), "%s frame %d: model and reference differ first at channel %d granule %d line %d" % ((name, f) + tuple(bad[0]))
        _REFERENCE[name] = v
    return _REFERENCE[name]


def flags(name):
    m = E.stream_model(name)
    return m["sum_out"] | m["bfly_out"]


def wrapped_frame(name, f):
    return bool(flags(name)[f].any())


# ------------------------------------------------------------------------------------------------------------------------ CPU
def test_fixture_is_the_builders(g17):
    S = E.streams()
    assert [str(n) for n in g17["names"]] == list(S) and g17["rate"].tolist() == [s.rate for s in S.values()]
    assert [(str(g17["names"][s]), int(k)) for s, k in zip(g17["run_stream"], g17["run_kbps"])] == E.runs()
    assert len(S) == 29 and len(E.runs()) == 35
    assert sum(1 for n in S if n.startswith("tone/") and "@" not in n) == 16


def test_edge_streams_are_the_first_hits_of_the_grid():
    """the band-edge streams are what the search over the grid finds first, at all three edges (the grid's first point is a hit at each)"""
    assert len(E.edge_grid()) == len(E.EDGE_DELTAS) * len(E.EDGE_AMPS) * len(E.EDGE_PHASES)
    for b in E.EDGE_BANDS:
        assert E.edge_search(b) == E.EDGE_HITS[b], b


def test_model_equals_the_reference(g17):
    """the model's wrapped values are the reference's __mdct_freq: by digest on every frame of every run, line by line on the frames held
    whole -- which are exactly the frames the model flags"""
    names = [str(n) for n in g17["names"]]
    for name in names:
        reference_mdct(g17, name)
    flagged = [(si, f) for si, n in enumerate(names) for f in range(E.FRAMES) if wrapped_frame(n, f)]
    assert flagged == [tuple(x) for x in g17["mdct_full_at"].tolist()]


def test_conditions_hold_on_the_reference(g17):
    """what the fixture is for, on the reference's records (reference_mdct) with the model's flags"""
    names = [str(n) for n in g17["names"]]
    above = below = 0
    bands, lone, lone_edges, sb_max = set(), 0, set(), {}
    for name in names:
        v, m = reference_mdct(g17, name), E.stream_model(name)
        assert np.array_equal(v, E.wrap32(m["bfly"])) and not (v == E.I32_MIN).any(), name
        assert m["y_max"] <= E.I32_MAX and m["sb_max"] <= E.I32_MAX, name      # the analysis never wraps
        sb_max[name] = m["sb_max"]
        above, below = above + int((m["sum"] > E.I32_MAX).sum()), below + int((m["sum"] < E.I32_MIN).sum())
        bands |= set((np.nonzero(m["sum_out"])[3] // 18).tolist())
        # a wrapped sum shows in the record: where no butterfly follows, the line is the exact sum less a multiple of 2^32
        plain = m["sum_out"] & (np.arange(576) % 18 >= 8) & (np.arange(576) % 18 < 10)
        assert ((m["sum"][plain] - v[plain]) % (1 << 32) == 0).all() and (m["sum"][plain] != v[plain]).all(), name
        for f, ch, gr in np.ndindex(E.FRAMES, 2, 2):
            if m["bfly_out"][f, ch, gr].any() and not m["sum_out"][f, ch, gr].any():
                lines = np.nonzero(m["bfly_out"][f, ch, gr])[0]
                lone += len(lines)
                lone_edges |= {E.band_edge(l) for l in lines}
                assert (m["bfly"][f, ch, gr][lines] != v[f, ch, gr][lines]).all()
    print("wrapped MDCT sums: %d above, %d below; butterfly results beyond int32 in granules without a wrapped sum: %d at band edges %s" % (
        above, below, lone, sorted(lone_edges)))
    assert bands == set(range(32))
    assert above >= 8 and below >= 8
    assert 1 in lone_edges and len(lone_edges) >= 2
    # the census as the documents state it (the module's docstring, oracle/README.md, docs/LOG.md): the fixture pins the samples, so it cannot move
    assert (above, below, lone, sorted(lone_edges)) == (44, 45, 12, [1, 16, 31])
    assert max(sb_max, key=sb_max.get) == "analysis_max" and sb_max["analysis_max"] > 909_000_000
    for name in names:                                               # granule 0 of a stream overlaps with zeros: none of its sums wraps
        assert not E.stream_model(name)["sum_out"][0, :, 0].any(), name
    for name, rate in E.OTHER_RATES:                                   # the transform does not read the rate
        assert np.array_equal(reference_mdct(g17, "%s@%d" % (name, rate)), reference_mdct(g17, name))
    refused = [(str(names[g17["run_stream"][r]]), int(g17["run_kbps"][r]), str(g17["raises"][r]), int(g17["raises_at"][r]))
               for r in range(len(g17["raises"])) if str(g17["raises"][r])]
    print("the reference refuses:", refused)
    assert refused == [("analysis_max", E.KBPS_LOW, "IndexError", 0)]


def test_oracle_equals_the_reference(orc, g17):
    """orc.encode on every run: __mdct_freq of every frame, every GrInfo field, tables, scfsi, frame sizes, cursors, padding, ix, bytes;
    rc -3 in front of the frame in which the reference raises IndexError"""
    fields = [str(f) for f in g17["gi_fields"]]
    assert fields == orc.GI_FIELDS
    for r, (name, kbps) in enumerate(E.runs()):
        s = E.streams()[name]
        o = orc.encode(s.pcm, s.rate, kbps)
        if str(g17["raises"][r]):
            assert str(g17["raises"][r]) == "IndexError" and o["rc"] == -3 and o["n_frames"] == int(g17["raises_at"][r]), (name, kbps, o["rc"])
            continue
        assert o["rc"] == 0 and o["n_frames"] == E.FRAMES, (name, kbps)
        assert np.array_equal(o["mdct_freq"], reference_mdct(g17, name)), (name, kbps)
        for i, k in enumerate(fields):
            assert np.array_equal(o["frames"]["gi"][k], g17["gi"][r][..., i]), (name, kbps, k)
        assert np.array_equal(o["frames"]["gi"]["table_select"], g17["table_select"][r]), (name, kbps)
        for k in ("scfsi", "written", "hide_off", "padding"):
            assert np.array_equal(o["frames"][k], g17[k][r]), (name, kbps, k)
        assert sha(o["ix"].astype("<i2")) == bytes(g17["ix_sha256"][r]), (name, kbps)
        assert len(o["mp3"]) == int(g17["mp3_len"][r]) and hashlib.sha256(o["mp3"]).digest() == bytes(g17["mp3_sha256"][r]), (name, kbps)


def test_batches_reach_every_shape():
    """the census of the batch list, before anything is launched (the GPU tests depend on it through the fixture below)"""
    check_batches()


def check_batches():
    B = E.batches()
    S = E.streams()
    for name, b in B.items():
        assert all(s in S and 1 <= k <= E.FRAMES for s, k in b), name
    c = E.batch_census(B.values(), wrapped_frame)
    print("batch census:", c)
    assert c["max frames"] == 32
    assert c["n_gran % 13"] == set(range(13))
    assert c["n_frames % 4"] == set(range(4))
    assert c["Ts % 64"] == set(range(0, 64, 4))
    assert c["start offset"] == set(range(13))
    assert c["g0 parity"] == {0, 1}
    assert c["ends at workgroup end"] >= 1 and c["starts at workgroup start"] >= 1
    assert c["loud places"] >= 6
    # the granule behind a stream boundary that wraps on rows of its own stream only (frame 0 of a stream flags granule 1, whose lead-in is
    # granule 0) and the last frame of the stream in front wrapping as well: a leak in either direction would meet loud values
    both = sum(1 for b in B.values() for (s0, k0), (s1, _) in zip(b, b[1:]) if wrapped_frame(s0, k0 - 1) and wrapped_frame(s1, 0))
    assert both >= 6
    return B


# ------------------------------------------------------------------------------------------------------------------------ GPU
@contextlib.contextmanager
def options(ctx, fused, shared):
    old = ctx.get_option("fused_encode"), ctx.get_option("analysis_shared")
    ctx.set_option("fused_encode", fused)
    ctx.set_option("analysis_shared", shared)
    try:
        yield
    finally:
        ctx.set_option("fused_encode", old[0])
        ctx.set_option("analysis_shared", old[1])


def same_lines(got, want, flagged, owner, what):
    """device against reference [frame][ch][gr][576]; a failure names the first line that differs and whether the model flags it"""
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = np.argwhere(got != want)
    if len(bad):
        f, ch, gr, line = (int(x) for x in bad[0])
        raise AssertionError("%s: %d lines differ, first in frame %d (%s) granule %d channel %d line %d (band %d, k %d): device %d, reference %d; "
                             "the model %s" % (what, len(bad), f, owner(f), gr, ch, line, line // 18, line % 18, got[f, ch, gr, line], want[f, ch, gr, line],
                                               "flags the line (a value outside int32)" if flagged[f, ch, gr, line] else "does not flag the line"))


@pytest.fixture(scope="module")
def batch_list():
    return check_batches()


@pytest.mark.gpu
@pytest.mark.parametrize("fused,shared", OPTIONS)
def test_streams_alone_equal_the_reference(ctx, mlib, g17, fused, shared):
    """ctx.encode_transform on every stream alone, the stream's sampling rate in its headers"""
    with options(ctx, fused, shared):
        for name in E.streams():
            pcm, hdr = E.batch_inputs([(name, E.FRAMES)], mlib.FRAME_HDR_DTYPE)
            got = ctx.encode_transform(pcm, hdr)
            same_lines(got, reference_mdct(g17, name), flags(name), lambda f: "%s frame %d" % (name, f), "%s alone, fused %d shared %d" % (name, fused, shared))


@pytest.mark.gpu
@pytest.mark.parametrize("fused,shared", OPTIONS)
def test_batches_equal_the_reference(ctx, mlib, g17, batch_list, fused, shared):
    """the batches of encode_edges.batches(): every frame of every stream in them is the fixture's frame of that stream"""
    with options(ctx, fused, shared):
        for bname, b in batch_list.items():
            pcm, hdr = E.batch_inputs(b, mlib.FRAME_HDR_DTYPE)
            want = np.concatenate([reference_mdct(g17, s)[:k] for s, k in b])
            flagged = np.concatenate([flags(s)[:k] for s, k in b])
            frames = ["%s frame %d" % (s, f) for s, k in b for f in range(k)]
            got = ctx.encode_transform(pcm, hdr)
            same_lines(got, want, flagged, lambda f: frames[f], "batch %s, fused %d shared %d" % (bname, fused, shared))


@pytest.mark.gpu
@pytest.mark.parametrize("fused,shared", OPTIONS)
def test_encoder_downstream_equals_the_reference(ctx, mlib, g17, fused, shared):
    """ctx.encode_pcm on every run of the fixture: the bytes, every granule's fields, tables and addresses, scfsi and the cursor are the
    reference's; MP3S_E_STEP_RANGE where the reference raises IndexError"""
    from test_gpu_parity import _check_gr
    fields = ",".join(str(f) for f in g17["gi_fields"]).encode()
    with options(ctx, fused, shared):
        for r, (name, kbps) in enumerate(E.runs()):
            s = E.streams()[name]
            if str(g17["raises"][r]):
                with pytest.raises(mlib.Mp3sError) as e:
                    ctx.encode_pcm(s.pcm, s.rate, kbps)
                assert e.value.code == mlib.E_STEP_RANGE, (name, kbps, e.value.code)
                continue
            got = ctx.encode_pcm(s.pcm, s.rate, kbps)
            assert got["n_frames"] == E.FRAMES and not got["too_long"] and got["hide_offset"] == int(g17["hide_off"][r][-1]), (name, kbps)
            assert len(got["mp3"]) == int(g17["mp3_len"][r]) == int(g17["written"][r].sum()), (name, kbps)
            assert hashlib.sha256(got["mp3"]).digest() == bytes(g17["mp3_sha256"][r]), (name, kbps)
            _check_gr(got, {"gi_fields": fields, "gi": g17["gi"][r], "table_select": g17["table_select"][r], "scfsi": g17["scfsi"][r]})
