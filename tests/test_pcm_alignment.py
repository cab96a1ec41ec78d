"""A cover file against its stego file (include/mp3s.h section vi-d): the lag search and the comparison at a lag -- the three passes
alone (mp3s_pcm_align_dev), mp3s_pcm_alignment_files and the facade's stego_distortions.

The expected values run no code of the new calls: hand-made int16 arrays for the kernels, decode_streams of both lists for the files,
and a brute-force numpy loop over the lags in int64.  Every integer is compared exactly."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from test_pcm_distortion import check_pair, corpus, mono_streams, ratios, same_ratio  # noqa: F401  (corpus: the fixture)

gpu = pytest.mark.gpu
NO_DIFF = 0xFFFFFFFF
UNWRITTEN = 0xFFFFFFFFFFFFFFFF                                       # what pcm_align_dev's buffers hold where no pass wrote
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ no device
def test_alignment_symbols_and_layout(mlib):
    L = mlib.lib()
    for s in ("mp3s_pcm_align_dev", "mp3s_pcm_alignment_files"):
        assert hasattr(L, s) and s in mlib.SYMBOLS, s
    # the sizes the header states
    assert (C.sizeof(mlib.PcmRunPair), C.sizeof(mlib.PcmLag), C.sizeof(mlib.PcmAlignment)) == (24, 40, 144)
    assert (mlib.PCM_RUN_PAIR_DTYPE.itemsize, mlib.PCM_LAG_DTYPE.itemsize) == (24, 40)
    for st, dt in ((mlib.PcmRunPair, mlib.PCM_RUN_PAIR_DTYPE), (mlib.PcmLag, mlib.PCM_LAG_DTYPE)):
        assert [(n, getattr(st, n).offset, getattr(st, n).size) for n, _ in st._fields_] == [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names]
    assert [(n, getattr(mlib.PcmLag, n).offset) for n, _ in mlib.PcmLag._fields_] == [
        ("lag", 0), ("n_best", 4), ("err2_best", 8), ("err2_at_0", 16), ("search_first", 24), ("search_rows", 28), ("n_rows", 32), ("n_chunks", 36)]
    assert mlib.PCM_LAG_DTYPE.fields["lag"][0] == np.dtype("<i4")
    assert [(n, getattr(mlib.PcmAlignment, n).offset) for n, _ in mlib.PcmAlignment._fields_] == [("at_lag", 0), ("lag", 96), ("scores", 136)]
    assert mlib.PCM_MAX_LAG == 4608
    txt = open(os.path.join(ROOT, "include", "mp3s.h")).read()
    for decl in ("typedef struct { uint32_t a_first, a_rows, b_first, b_rows, out_first, reserved; } mp3s_pcm_run_pair;   /* 24 bytes",
                 "} mp3s_pcm_lag;                              /* 40 bytes */", "} mp3s_pcm_alignment;             /* 96 + 40 + 8 = 144 bytes */",
                 "#define MP3S_PCM_MAX_LAG 4608", "int32_t lag; uint32_t n_best;", "uint64_t err2_best, err2_at_0;", "uint32_t search_first, search_rows;",
                 "uint32_t n_rows, n_chunks;", "mp3s_pcm_distortion at_lag;", "mp3s_pcm_lag lag;", "const uint64_t *scores;"):
        assert decl in txt, decl
    assert txt.index("(vi-c) what hiding changed") < txt.index("(vi-d) a cover file against its stego file") < txt.index("(vii) asynchronous host-fed pipeline")


def test_alignment_argument_checks_need_no_device(mlib):
    L = mlib.lib()
    mem = C.create_string_buffer(4096)
    p = (C.addressof(mem) + 255) & ~255                              # stand-ins for the context and the arrays (never read)
    runs = np.zeros(2, dtype=mlib.PCM_RUN_PAIR_DTYPE)
    lags = np.zeros(2, dtype=np.int32)

    def dev(**kw):
        a = dict(ctx=p, pcm=p, nch=2, d_runs=p, h_runs=runs.ctypes.data, n=2, max_lag=100, search_rows=64, h_lags=None, scores=p, lags=p, frames=p, out=p)
        a.update(kw)
        return L.mp3s_pcm_align_dev(*a.values())
    assert L.mp3s_pcm_align_dev(None, None, 2, None, None, 1, 0, 1, None, None, None, None, None) == mlib.E_ARG
    for k in ("ctx", "pcm", "d_runs", "h_runs", "scores", "lags", "frames", "out"):   # every pointer in turn (scores: needed for a search)
        assert dev(**{k: None}) == mlib.E_ARG, k
    for n in (0, -3):
        assert dev(n=n) == mlib.E_ARG
    for nch in (0, 3, -1):
        assert dev(nch=nch) == mlib.E_ARG and b"nch" in L.mp3s_last_error()
    for m in (-1, 4609, 1 << 30):
        assert dev(max_lag=m) == mlib.E_ARG and b"max_lag" in L.mp3s_last_error(), m
    for s in (0, -1):
        assert dev(search_rows=s) == mlib.E_ARG and b"search_rows" in L.mp3s_last_error(), s
    for bad in (4609, -4609):
        lags[:] = (0, bad)
        assert dev(h_lags=lags.ctypes.data) == mlib.E_ARG and b"pair 1" in L.mp3s_last_error(), bad
        assert dev(h_lags=lags.ctypes.data, scores=None) == mlib.E_ARG
    assert dev(pcm=p + 8) == mlib.E_ARG and b"aligned" in L.mp3s_last_error()

    def files(**kw):
        a = dict(ctx=p, a=p, a_lens=p, b=p, b_lens=p, n=2, max_lag=100, search_rows=64, lags=None, profile=0, owner=C.cast(p, C.POINTER(C.c_void_p)), out=p, status=None)
        a.update(kw)
        return L.mp3s_pcm_alignment_files(*a.values())
    for k in ("ctx", "a", "a_lens", "b", "b_lens", "owner", "out"):
        assert files(**{k: None}) == mlib.E_ARG, k
    for n in (0, -1):
        assert files(n=n) == mlib.E_ARG
    for m in (-1, 4609):
        assert files(max_lag=m) == mlib.E_ARG and b"max_lag" in L.mp3s_last_error()
    assert files(search_rows=0) == mlib.E_ARG and b"search_rows" in L.mp3s_last_error()
    lags[:] = (-4609, 0)
    assert files(lags=lags.ctypes.data) == mlib.E_ARG and b"pair 0" in L.mp3s_last_error()


# ------------------------------------------------------------------------------------------------ numpy's side
def lag_search(a, b, max_lag, search_rows):
    """a, b: int16 [rows][nch] -> None for a pair that is not searched, else dict(scores, lag, n_best, err2_best, err2_at_0, search_first, search_rows)"""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    M = max_lag
    W = min(len(a), len(b)) - 2 * M
    if W < 1:
        return None
    S = min(W, search_rows)
    s0 = M + (W - S) // 2
    bw = b[s0:s0 + S]
    scores = np.zeros(2 * M + 1, dtype=np.int64)
    for L in range(-M, M + 1):
        d = a[s0 + L:s0 + L + S] - bw
        scores[L + M] = (d * d).sum()
    best = int(scores.min())
    lag = min((int(i) - M for i in np.nonzero(scores == best)[0]), key=lambda x: (abs(x), x < 0))   # smaller |L| first, then +k before -k
    return {"scores": scores, "lag": lag, "n_best": int((scores == best).sum()), "err2_best": best, "err2_at_0": int(scores[M]), "search_first": s0,
            "search_rows": S}


def compare_at(a, b, lag):
    """the chunk records (columns) and the pair record of a against b at `lag`, with n_rows and n_chunks"""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    nch = a.shape[1]
    i0, i1 = max(0, -lag), min(len(b), len(a) - lag)
    n_rows = max(0, i1 - i0)
    x, y = a[i0 + lag:i0 + lag + n_rows].reshape(-1), b[i0:i0 + n_rows].reshape(-1)
    d = x - y
    per = 1152 * nch
    cols = {f: [] for f in ("err2", "sig2", "max_abs", "n_diff", "first_diff")}
    for at in range(0, len(d), per):
        dd, xx = d[at:at + per], x[at:at + per]
        ne = np.nonzero(dd)[0]
        for f, v in (("err2", (dd * dd).sum()), ("sig2", (xx * xx).sum()), ("max_abs", np.abs(dd).max()), ("n_diff", len(ne)), ("first_diff", ne[0] if len(ne) else NO_DIFF)):
            cols[f].append(int(v))
    ne = np.nonzero(d)[0]
    pair = {"err2": int((d * d).sum()), "sig2": int((x * x).sum()), "max_abs": int(np.abs(d).max()) if len(d) else 0, "n_diff": len(ne),
            "first_diff": int(ne[0]) if len(ne) else -1}
    return {"chunks": {f: np.array(v, dtype=np.int64) for f, v in cols.items()}, "pair": pair, "n_rows": n_rows, "n_chunks": (n_rows + 1151) // 1152}


def place_runs(mlib, cases, rng, nch, whole=()):
    """one buffer, the runs of all pairs scrambled over it: the pairs `whole` (runs of whole frames) first, on frame boundaries; the others
    behind them, every run after a gap of 1 .. 3 rows.  All A runs in one shuffled order, then all B runs in another; the chunk records in
    a third.  -> (pcm [rows][nch], PCM_RUN_PAIR_DTYPE records)"""
    n = len(cases)
    runs = np.zeros(n, dtype=mlib.PCM_RUN_PAIR_DTYPE)
    rest = [int(k) for k in rng.permutation(n) if k not in whole]
    whole = list(whole)
    parts, at = [], 0
    for group, gap in ((whole, False), (rest, True)):
        for which, order in (("a", group), ("b", group[1:] + group[:1])):
            for k in order:
                run = cases[k][1 if which == "a" else 2]
                if gap:
                    g = int(rng.integers(1, 4))
                    parts.append(rng.integers(-32768, 32768, size=(g, nch)).astype(np.int16))
                    at += g
                runs[which + "_first"][k], runs[which + "_rows"][k] = at, len(run)
                parts.append(run)
                at += len(run)
    out_at = 0
    for k in rng.permutation(n):
        runs["out_first"][k] = out_at
        out_at += (min(len(cases[k][1]), len(cases[k][2])) + 1151) // 1152
    pcm = np.concatenate(parts)
    assert pcm.nbytes < 10_000_000 and at == len(pcm)
    some = np.minimum(runs["a_rows"], runs["b_rows"]) > 0
    assert (np.diff(runs["out_first"][some].astype(np.int64)) < 0).any(), "out_first is monotone"
    assert (runs["a_first"][some] + runs["a_rows"][some] != runs["b_first"][some]).all(), "A and B of a pair are adjacent"
    assert (runs["a_first"] % 2 == 1).any() and (runs["b_first"] % 2 == 1).any(), "no run starts at an odd row"
    return pcm, runs


def check_pair_at(name, k, runs, lag, a, b, frames, got):
    """the chunk records and the pair record of case k against numpy at `lag`"""
    w = compare_at(a, b, lag)
    first, n = int(runs["out_first"][k]), w["n_chunks"]
    for f in ("err2", "sig2", "max_abs", "n_diff", "first_diff"):
        assert np.array_equal(frames[f][first:first + n].astype(np.int64), w["chunks"][f]), (name, f)
        assert int(got[f][k]) == w["pair"][f], (name, f, int(got[f][k]), w["pair"][f])
    assert not frames["reserved"][first:first + n].any() and int(got["reserved"][k]) == 0, name
    bound = (min(len(a), len(b)) + 1151) // 1152
    assert (frames["err2"][first + n:first + bound] == UNWRITTEN).all(), (name, "a record past the overlap's chunks was written")
    return w


def noise(rng, rows, nch, amp=30000):
    return rng.integers(-amp, amp + 1, size=(rows, nch)).astype(np.int16)


def planted(rng, rows, nch, lag, max_lag):
    """B = noise, A = B delayed by `lag` rows (a[i + lag] = b[i]) + noise of +-1"""
    x = noise(rng, rows + 2 * max_lag, nch)
    b = x[max_lag:max_lag + rows]
    a = x[max_lag - lag:max_lag - lag + rows] + rng.integers(-1, 2, size=(rows, nch)).astype(np.int16)
    return a.astype(np.int16), b.copy()


# ------------------------------------------------------------------------------------------------ GPU, the kernels alone
MAX_LAG, SEARCH_ROWS = 1200, 2304


@gpu
@pytest.mark.parametrize("nch", [1, 2])
def test_lag_search_kernels_alone(ctx, mlib, nch):
    """one search call: planted lags (0, +-1, +3, -1057, +-max_lag), ties (constant runs, a period of 14), both extremes of d over the
    whole window, W = 1 and W = 0, unequal lengths, rows that are no multiple of 1152, exactly 1152 rows (too short: not searched),
    257 chunks, a pair of 0 rows"""
    rng = np.random.default_rng(500 + nch)
    M = MAX_LAG
    cases = []                                                       # (name, A, B)
    for lag in (0, 1, -1, 3, -1057, M, -M):
        cases.append((f"planted {lag}", *planted(rng, 5000, nch, lag, M)))
    const = np.full((3000, nch), 1234, np.int16)
    cases.append(("constant", const, const.copy()))
    wave = np.array([0, 900, -1700, 2500, 31000, -32768, 32767, 12, -13, 7000, -7001, 150, -2900, 444], np.int16)
    idx = np.arange(4000)
    cases.append(("period 14", np.repeat(wave[(idx + 7) % 14][:, None], nch, axis=1), np.repeat(wave[idx % 14][:, None], nch, axis=1)))
    lo, hi = np.full((2 * M + SEARCH_ROWS + 10, nch), -32768, np.int16), np.full((2 * M + SEARCH_ROWS + 10, nch), 32767, np.int16)
    cases.append(("lowest against highest", lo, hi))
    cases.append(("lowest against lowest", lo, lo.copy()))
    cases.append(("W = 1", noise(rng, 2 * M + 1, nch), noise(rng, 2 * M + 400, nch)))
    cases.append(("W = 0", noise(rng, 2 * M + 300, nch), noise(rng, 2 * M, nch)))
    cases.append(("unequal", *[x[:r] for x, r in zip(planted(rng, 5000, nch, -40, M), (5000, 4101))]))
    cases.append(("exactly 1152", noise(rng, 1152, nch), noise(rng, 1152, nch)))
    cases.append(("257 chunks", *planted(rng, 256 * 1152 + 1300, nch, 333, M)))
    cases.append(("no row", noise(rng, 0, nch), noise(rng, 0, nch)))
    pcm, runs = place_runs(mlib, cases, rng, nch)
    scores, lags, frames, got = ctx.pcm_align_dev(pcm, runs, nch, M, SEARCH_ROWS)
    assert scores.shape == (len(cases), 2 * M + 1) and len(lags) == len(got) == len(cases)
    by = {}
    for k, (name, a, b) in enumerate(cases):
        w = lag_search(a, b, M, SEARCH_ROWS)
        g = {f: int(lags[f][k]) for f in lags.dtype.names}
        print(nch, name, g, None if w is None else {f: v for f, v in w.items() if f != "scores"})
        if w is None:
            assert (g["lag"], g["n_best"], g["err2_best"], g["err2_at_0"], g["search_first"], g["search_rows"]) == (0, 0, 0, 0, 0, 0), name
            assert (scores[k] == UNWRITTEN).all(), name
            lag = 0
        else:
            assert np.array_equal(scores[k].astype(np.int64), w["scores"]), (name, np.nonzero(scores[k].astype(np.int64) != w["scores"])[0][:8])
            for f in ("lag", "n_best", "err2_best", "err2_at_0", "search_first", "search_rows"):
                assert g[f] == w[f], (name, f, g[f], w[f])
            lag = w["lag"]
        c = check_pair_at(name, k, runs, lag, a, b, frames, got)
        assert (g["n_rows"], g["n_chunks"]) == (c["n_rows"], c["n_chunks"]), name
        by[name] = (k, w, c)
    n_lags = 2 * M + 1
    for lag in (0, 1, -1, 3, -1057, M, -M):
        k, w, _ = by[f"planted {lag}"]
        assert (w["lag"], w["n_best"]) == (lag, 1) and int(lags["lag"][k]) == lag
    assert (by["constant"][1]["lag"], by["constant"][1]["n_best"], by["constant"][1]["err2_best"]) == (0, n_lags, 0)
    assert (by["period 14"][1]["lag"], by["period 14"][1]["n_best"]) == (7, sum(1 for L in range(-M, M + 1) if L % 14 == 7))
    k, w, _ = by["lowest against highest"]
    assert (scores[k] == np.uint64(SEARCH_ROWS * nch * 65535 ** 2)).all() and (w["lag"], w["n_best"]) == (0, n_lags)   # 2 * 65535^2 > 2^32 a row
    k, w, _ = by["lowest against lowest"]
    assert not scores[k].any() and (w["lag"], w["n_best"]) == (0, n_lags)
    assert (by["W = 1"][1]["search_rows"], by["W = 1"][1]["search_first"]) == (1, M) and by["W = 0"][1] is None and by["exactly 1152"][1] is None
    assert by["unequal"][1]["lag"] == -40 and by["257 chunks"][1]["lag"] == 333 and by["257 chunks"][2]["n_chunks"] == 257
    k, w, c = by["no row"]
    assert w is None and c["n_rows"] == 0 and [int(got[f][k]) for f in got.dtype.names] == [0, 0, 0, -1, 0, 0]


@gpu
@pytest.mark.parametrize("nch", [1, 2])
def test_given_lags_and_small_searches(ctx, mlib, nch):
    """given lags (0, +-5, an overlap of one row, an empty overlap, 257 chunks and one row more), lag 0 on runs of whole frames against
    pcm_diff_dev on the same buffer, and searches with max_lag 0 and 3 whose windows are cut out of longer pairs"""
    rng = np.random.default_rng(600 + nch)
    rows_a = 3000
    cases, given = [], []
    for name, frames_n in (("whole 3", 3), ("whole 257", 257), ("whole 1", 1)):
        cases.append((name, noise(rng, frames_n * 1152, nch, 32767), noise(rng, frames_n * 1152, nch, 32767)))
        given.append(0)
    whole = [0, 1, 2]
    same = noise(rng, 2 * 1152, nch)
    cases.append(("whole identical", same, same.copy()))
    given.append(0)
    whole.append(3)
    for lag in (0, 5, -5, rows_a - 1, rows_a, -4608, 4608):
        cases.append((f"given {lag}", noise(rng, rows_a, nch, 32767), noise(rng, 5000 if lag == -4608 else 3500, nch, 32767)))
        given.append(lag)
    cases.append(("one row past 256 chunks", noise(rng, 256 * 1152 + 8, nch), noise(rng, 256 * 1152 + 1, nch)))
    given.append(7)
    cases.append(("no row", noise(rng, 0, nch), noise(rng, 10, nch)))
    given.append(-2)
    pcm, runs = place_runs(mlib, cases, rng, nch, whole)
    scores, lags, frames, got = ctx.pcm_align_dev(pcm, runs, nch, 100, 64, lags=given)
    assert scores is None
    by = {}
    for k, (name, a, b) in enumerate(cases):
        g = {f: int(lags[f][k]) for f in lags.dtype.names}
        c = check_pair_at(name, k, runs, given[k], a, b, frames, got)
        print(nch, name, g, c["pair"])
        assert g == {"lag": given[k], "n_best": 0, "err2_best": 0, "err2_at_0": 0, "search_first": 0, "search_rows": 0, "n_rows": c["n_rows"],
                     "n_chunks": c["n_chunks"]}, name
        by[name] = (k, c)
    assert by[f"given {rows_a - 1}"][1]["n_rows"] == 1 and by[f"given {rows_a}"][1]["n_rows"] == 0
    k = by[f"given {rows_a}"][0]
    assert [int(got[f][k]) for f in got.dtype.names] == [0, 0, 0, -1, 0, 0]
    assert by["given -4608"][1]["n_rows"] == 5000 - 4608 and by["given 4608"][1]["n_rows"] == 0
    assert by["one row past 256 chunks"][1]["n_chunks"] == 257 and by["one row past 256 chunks"][1]["n_rows"] == 256 * 1152 + 1
    # lag 0 on runs of whole frames: what mp3s_pcm_diff_dev computes, on the same buffer
    assert (runs["a_first"][whole] % 1152 == 0).all() and (runs["b_first"][whole] % 1152 == 0).all()
    pairs = np.zeros(len(whole), dtype=mlib.PCM_PAIR_DTYPE)
    pairs["a_first"], pairs["b_first"] = runs["a_first"][whole] // 1152, runs["b_first"][whole] // 1152
    pairs["n_frames"], pairs["out_first"] = runs["a_rows"][whole] // 1152, runs["out_first"][whole]
    whole_rows = int(max((runs["a_first"][whole] + runs["a_rows"][whole]).max(), (runs["b_first"][whole] + runs["b_rows"][whole]).max()))
    frames0, got0 = ctx.pcm_diff_dev(pcm[:whole_rows].reshape(-1), pairs, nch)
    for j, k in enumerate(whole):
        first, n = int(runs["out_first"][k]), int(pairs["n_frames"][j])
        assert frames0[first:first + n].tobytes() == frames[first:first + n].tobytes(), cases[k][0]
        assert got0[j].tobytes() == got[k].tobytes(), cases[k][0]
    # searches with max_lag 0 (one score) and 3, a window of 64 rows out of the middle of the same pairs
    for M in (0, 3):
        scores, lags, frames, got = ctx.pcm_align_dev(pcm, runs, nch, M, 64)
        for k, (name, a, b) in enumerate(cases):
            w = lag_search(a, b, M, 64)
            if w is None:
                assert int(lags["n_best"][k]) == 0 and (scores[k] == UNWRITTEN).all(), (M, name)
                continue
            assert np.array_equal(scores[k].astype(np.int64), w["scores"]), (M, name)
            for f in ("lag", "n_best", "err2_best", "err2_at_0", "search_first", "search_rows"):
                assert int(lags[f][k]) == w[f], (M, name, f)
            assert w["search_rows"] == min(64, min(len(a), len(b)) - 2 * M) and w["search_first"] == M + (min(len(a), len(b)) - 2 * M - w["search_rows"]) // 2
            check_pair_at(name, k, runs, w["lag"], a, b, frames, got)


# ------------------------------------------------------------------------------------------------ GPU, files
FIXTURE_LAG = 1057                                                   # the re-encode's delay in rows, as the CPU oracle found it on tests/golden/test.mp3


def expect_alignment(ctx, a, b, max_lag, search_rows, lag=None):
    """the fields of pcm_alignments for file a against file b from decode_streams + numpy"""
    x, y = ctx.decode_streams([a, b], per_file=True)
    assert x["channels"] == y["channels"]
    x, y = dict(x, pcm=x["pcm"].reshape(len(x["pcm"]), -1)), dict(y, pcm=y["pcm"].reshape(len(y["pcm"]), -1))
    w = lag_search(x["pcm"], y["pcm"], max_lag, search_rows) if lag is None else None
    if w is None:
        w = {"scores": None, "lag": 0 if lag is None else lag, "n_best": 0, "err2_best": 0, "err2_at_0": 0, "search_first": 0, "search_rows": 0}
    c = compare_at(x["pcm"], y["pcm"], w["lag"])
    w.update(c["pair"], profile=c["chunks"], n_frames=c["n_chunks"], n_samples=c["n_rows"] * x["channels"], rows_a=len(x["pcm"]), rows_b=len(y["pcm"]),
             channels=x["channels"], sampling_rate=x["sampling_rate"])
    w["snr_db"], w["psnr_db"] = ratios(w["err2"], w["sig2"], w["n_samples"])
    return w


def check_alignment(i, r, w, profile=True):
    check_pair(i, r, w, profile)
    print(i, {k: r[k] for k in ("lag", "n_best", "err2_best", "err2_at_0", "search_first", "search_rows")})
    for f in ("lag", "n_best", "err2_best", "err2_at_0", "search_first", "search_rows"):
        assert int(r[f]) == int(w[f]), (i, f, r[f], w[f])
    if profile and w["scores"] is not None:
        assert r["scores"].dtype == np.uint64 and np.array_equal(r["scores"].astype(np.int64), w["scores"]), i
    else:
        assert r["scores"] is None, i


@pytest.fixture(scope="module")
def fixture_pair(ctx, golden_dir):
    cover = open(os.path.join(golden_dir, "test.mp3"), "rb").read()
    hidden = ctx.hide_messages([cover], ["a short message"])[0]
    assert not isinstance(hidden, Exception) and not hidden["too_long"]
    return bytes(hidden["data"]), cover


@gpu
def test_stego_against_cover_finds_the_delay(ctx, mlib, fixture_pair):
    stego, cover = fixture_pair
    w = expect_alignment(ctx, stego, cover, 2304, 4608)
    r = ctx.pcm_alignments([stego], [cover], profile=True)[0]
    check_alignment(0, r, w)
    assert len(r["scores"]) == 4609 and r["search_rows"] == 4608
    # the codec's delay, as numpy sees it and as the device sees it
    assert (w["lag"], w["n_best"]) == (FIXTURE_LAG, 1), (w["lag"], w["n_best"])
    assert (r["lag"], r["n_best"]) == (FIXTURE_LAG, 1)
    assert r["err2_best"] < r["err2_at_0"] and r["n_samples"] == 2 * (r["rows_a"] - FIXTURE_LAG) and r["n_frames"] == 36
    # the other way round the stego audio comes earlier
    back = ctx.pcm_alignments([cover], [stego], profile=True)[0]
    check_alignment(0, back, expect_alignment(ctx, cover, stego, 2304, 4608))
    assert (back["lag"], back["n_best"]) == (-FIXTURE_LAG, 1)
    # the found lag handed back: the same comparison, nothing searched; and without the profile nothing else changes
    again = ctx.pcm_alignments([stego, cover], [cover, stego], lags=[r["lag"], back["lag"]], profile=True)
    for i, (g, s) in enumerate(zip(again, (r, back))):
        check_alignment(i, g, expect_alignment(ctx, *((stego, cover) if i == 0 else (cover, stego)), 2304, 4608, lag=s["lag"]))
        for f in ("err2", "sig2", "n_samples", "n_diff", "first_diff", "rows_a", "rows_b", "max_abs", "channels", "sampling_rate", "n_frames", "snr_db", "psnr_db", "lag"):
            assert g[f] == s[f], (i, f)
        assert g["profile"].tobytes() == s["profile"].tobytes() and g["n_best"] == 0 and g["scores"] is None
    plain = ctx.pcm_alignments([stego], [cover])[0]
    check_alignment(0, plain, w, profile=False)


@gpu
def test_lag_zero_is_pcm_distortions(ctx, mlib, corpus):
    n = len(corpus["a"])
    out = ctx.pcm_alignments(corpus["a"], corpus["b"], lags=[0] * n, profile=True)
    base = ctx.pcm_distortions(corpus["a"], corpus["b"], profile=True)
    assert len(out) == n and all(w["rows_a"] == w["rows_b"] for w in corpus["want"])
    for i, (r, w, d) in enumerate(zip(out, corpus["want"], base)):
        check_pair(i, r, w)
        for f in ("err2", "sig2", "n_diff", "max_abs", "first_diff", "n_samples", "rows_a", "rows_b", "snr_db", "psnr_db"):
            assert r[f] == d[f], (i, f, r[f], d[f])
        assert r["profile"].tobytes() == d["profile"].tobytes(), i
        assert (r["lag"], r["n_best"], r["scores"]) == (0, 0, None)


@gpu
def test_every_failing_pair_gets_its_code_and_the_others_their_lag(ctx, mlib, corpus, fixture_pair):
    stego, cover = fixture_pair
    mono, _ = mono_streams()
    short = corpus["files"][5]                                       # 2 frames: 2304 rows, too few for max_lag 2304
    refs = mlib.walk_stream(stego)["refs"]
    cut = stego[:int(refs["file_off"][30])]                          # a truncated file: its first 30 frames
    garbage = b"\xff\xfb\x90"
    a = [stego, mono, mono, cut, None, short, garbage, cover]
    b = [cover, mono, cover, cover, cover, short, cover, stego]
    out = ctx.pcm_alignments(a, b, profile=True)
    for i in (0, 1, 3, 7):
        check_alignment(i, out[i], expect_alignment(ctx, a[i], b[i], 2304, 4608))
    assert out[0]["lag"] == FIXTURE_LAG and out[7]["lag"] == -FIXTURE_LAG and out[3]["lag"] == FIXTURE_LAG and out[3]["rows_a"] == 30 * 1152
    assert (out[1]["lag"], out[1]["err2"], out[1]["channels"], out[1]["err2_best"]) == (0, 0, 1, 0) and math.isinf(out[1]["snr_db"])
    dec = ctx.decode_streams([garbage], per_file=True)[0]
    assert [(type(out[i]), out[i].code) for i in (2, 4, 5, 6)] == [(mlib.Mp3sError, c) for c in (mlib.E_UNSUPPORTED, mlib.E_ARG, mlib.E_UNSUPPORTED, dec.code)]
    # given lags need no room to search: the short pair is compared
    given = ctx.pcm_alignments([short, stego], [short, cover], lags=[0, 5])
    assert given[0]["err2"] == 0 and given[0]["n_samples"] == 2 * 2304 and given[1]["lag"] == 5 and given[1]["n_samples"] == 2 * (36 * 1152 - 5)
    # status == NULL in the C call: the first failing pair fails the call with its code and its text, no owner
    L = mlib.lib()

    def raw(xa, xb, max_lag=2304):
        n, _ka, pa, la = mlib._file_list(xa)
        _, _kb, pb, lb = mlib._file_list(xb)
        res, owner = (mlib.PcmAlignment * n)(), C.c_void_p()
        rc = L.mp3s_pcm_alignment_files(ctx.handle, pa, la, pb, lb, n, max_lag, 4608, None, 0, C.byref(owner), res, None)
        assert not owner.value
        return rc, L.mp3s_last_error().decode()
    rc, why = raw([stego, short], [cover, short])
    assert rc == mlib.E_UNSUPPORTED and "pair 1" in why and "2304 rows" in why and "max_lag = 2304" in why, why
    rc, why = raw([stego, short], [cover, short], max_lag=1152)      # W = 0: one row short
    assert rc == mlib.E_UNSUPPORTED and "pair 1" in why and "max_lag = 1152" in why, why
    rc, why = raw([stego, mono], [cover, cover])
    assert rc == mlib.E_UNSUPPORTED and "pair 1" in why and "1 channel" in why and "2 channel" in why, why
    rc, why = raw([stego, garbage], [cover, cover])
    assert rc == dec.code and "pair 1" in why and "file a" in why, why


@gpu
def test_stego_distortions_is_the_two_step_way(ctx, mlib, golden_dir):
    from synth_pcm import synth_pcm
    files = [open(os.path.join(golden_dir, "test.mp3"), "rb").read()]
    files += [bytes(ctx.encode_pcm(synth_pcm(36, seed=3000 + i), 44100, 128, None)["mp3"]) for i in range(2)]
    msgs = ["fits", "a message that does not fit into thirty-six frames " * 200, None]
    hidden = ctx.hide_messages(files, msgs)
    assert [h["too_long"] for h in hidden] == [False, True, False]
    by_hand = ctx.pcm_alignments([h["data"] for h in hidden], files, profile=True)
    out = ctx.stego_distortions(files, msgs, profile=True)
    for i, (r, w, h) in enumerate(zip(out, by_hand, hidden)):
        assert set(r) == set(w) | {"too_long", "hide_offset"}
        assert (r["too_long"], r["hide_offset"]) == (h["too_long"], h["hide_offset"]), i
        for f in w:
            if f in ("profile", "scores"):
                assert r[f].tobytes() == w[f].tobytes(), (i, f)
            else:
                assert r[f] == w[f] or (math.isinf(r[f]) and math.isinf(w[f])), (i, f, r[f], w[f])
        check_alignment(i, r, expect_alignment(ctx, h["data"], files[i], 2304, 4608))
    print([(r["lag"], r["n_best"], round(r["snr_db"], 2)) for r in out])
    assert out[0]["lag"] == FIXTURE_LAG
    refused = ctx.stego_distortions([b"not an mp3 file at all" * 10], ["x"])[0]
    assert isinstance(refused, mlib.Mp3sError)
