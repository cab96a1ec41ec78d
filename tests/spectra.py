"""Spectra (MDCT lines, int32 [n][576]) that PCM through the encoder's filter bank does not produce: lone lines, empty regions below the last
big value, everything at the quantiser's first thresholds.  What the rate loop's shortcuts (csrc/k_rate.hpp rl_precheck, the bounds in rl_body)
are checked on, against the reference's loop body restated in oracle/ (MP3_Encoder.py:958-996, 1064-1095, 1170-1264)."""
import numpy as np

KINDS = ("lone_line", "hf_few", "hf_noise", "lf_gap", "dense", "ones", "twos_far_apart", "count1_only")


def sparse_spectra(seed, n, base=32768):
    """n spectra, kinds in rotation.  `base`: |xr| that quantises to 1 at the step the caller aims at (32768 = step -60, the binary search's
    first probe: tests/test_tables.py pins rl_t1[67]); amplitudes are drawn around small multiples of it so that a probe sees 0, 1, 2, 3 ..."""
    rng = np.random.default_rng(seed)
    xr = np.zeros((n, 576), dtype=np.int64)

    def amp(size, lo=0.3, hi=40.0):
        return (base * np.exp(rng.uniform(np.log(lo), np.log(hi), size))).astype(np.int64)

    def signs(size):
        return rng.integers(0, 2, size) * 2 - 1
    for i in range(n):
        k = KINDS[i % len(KINDS)]
        if k == "lone_line":                       # one line, mostly far up: big_values reaches it, every region below is empty
            p = int(rng.integers(0, 576)) if rng.random() < 0.3 else int(rng.integers(400, 576))
            xr[i, p] = amp(1, 1.0, 200.0)[0] * signs(1)[0]
        elif k == "hf_few":                        # a handful of lines above line 300
            m = int(rng.integers(1, 12))
            p = rng.choice(np.arange(300, 576), m, replace=False)
            xr[i, p] = amp(m, 0.8, 30.0) * signs(m)
        elif k == "hf_noise":                      # nothing below a cut, low-level noise above
            cut = int(rng.integers(100, 560))
            m = 576 - cut
            xr[i, cut:] = amp(m, 0.2, 6.0) * signs(m) * (rng.random(m) < rng.uniform(0.05, 1.0))
        elif k == "lf_gap":                        # a low band, a gap of zeros, a high band
            a, b = sorted(rng.integers(2, 570, 2))
            xr[i, :a] = amp(a, 0.3, 20.0) * signs(a)
            xr[i, b:] = amp(576 - b, 0.3, 8.0) * signs(576 - b)
        elif k == "dense":                         # every line, one level per spectrum
            lvl = np.exp(rng.uniform(np.log(0.5), np.log(3000.0)))
            xr[i] = (base * lvl * rng.random(576)).astype(np.int64) * signs(576)
        elif k == "ones":                          # everything quantises to 0 or 1 at the aimed step
            xr[i] = amp(576, 0.5, 1.9) * signs(576) * (rng.random(576) < rng.uniform(0.02, 1.0))
        elif k == "twos_far_apart":                # a few values >= 2 between long runs of zeros and ones
            xr[i] = amp(576, 0.5, 1.9) * signs(576) * (rng.random(576) < rng.uniform(0.0, 0.3))
            m = int(rng.integers(1, 5))
            p = rng.choice(576, m, replace=False)
            xr[i, p] = amp(m, 2.5, 12.0) * signs(m)
        else:                                      # count1_only: ones in the lowest lines only
            top = int(rng.integers(1, 200))
            xr[i, :top] = amp(top, 0.9, 1.9) * signs(top) * (rng.random(top) < 0.7)
    return np.clip(xr, -(2 ** 31 - 1), 2 ** 31 - 1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Families for the per-unit tests of the rate loop (tests/test_rate_units.py).  The quantiser (MP3_Encoder.py:373-415) takes
# ln = round(|xr| / (2 * base)) and gives int(ln ** 0.75 - 0.0946 + 0.5) below ln = 10000, int((|xr| / (2 * base)) ** 0.75) from there on,
# `base` being as above the |xr| that quantises to 1 at the aimed step (2 ** (30 + step / 4)).

# the boundaries of the table choice (MP3_Encoder.py:1170-1264): below 15 by x_len, 15 = the first escape, then 15 + linmax and one more for
# every linmax of books 16-23 and 24-31, and the two values around which quantize refuses (:392)
EDGE_VALUES = (1, 2, 3, 5, 7, 14, 15) + tuple(15 + m + d for m in (1, 3, 7, 15, 63, 255, 1023, 8191) for d in (0, 1)) + (8192, 8193)


def level_of(v):
    """|xr| / base in the middle of the quantiser's bucket for the value v >= 1"""
    if v == 8192:       # the last value quantize lets through: ln 165140.39 (8192 ** (4 / 3)) .. 165140.5 (rounds to 165140, the limit of :392)
        return 2.0 * 165140.45
    ln = (v + 0.0946) ** (4.0 / 3.0)
    if ln < 9000:
        ln = max(np.rint(ln), 1.0)
        assert int(ln ** 0.75 - 0.0946 + 0.5) == v, v
        return 2.0 * ln
    return 2.0 * (v + 0.5) ** (4.0 / 3.0)


def _finish(xr):
    return np.clip(np.rint(xr), -(2 ** 31 - 1), 2 ** 31 - 1).astype(np.int32)


def quiet(seed, n, base=32768):
    """n spectra whose lines all quantise to 0 or 1 at the aimed step, so that the final step or some probe of the search has big_values == 0
    and keeps the addresses it inherited (__subdivide, MP3_Encoder.py:1004-1006).  Density from a single line to all 576; every third spectrum
    has its ones only above line 400."""
    rng = np.random.default_rng(seed)
    xr = np.zeros((n, 576))
    for i in range(n):
        lo = 400 if i % 3 == 2 else 0
        m = 576 - lo
        k = (1, m)[i % 7 == 3] if i % 7 in (0, 3) else int(np.ceil(m * np.exp(rng.uniform(np.log(1.0 / m), 0.0))))
        p = lo + rng.choice(m, k, replace=False)
        xr[i, p] = base * rng.uniform(1.02, 2.9, k) * (rng.integers(0, 2, k) * 2 - 1)
    return _finish(xr)


def escape_edges(seed, n, base=32768):
    """n spectra of one to four lines whose largest value at the aimed step is EDGE_VALUES[i % len(EDGE_VALUES)], the other peaks anywhere
    below it, over low-level noise (values 0, 1 and a few 2 on a part of the lines).  A peak that does not fit into 31 bits is clipped."""
    rng = np.random.default_rng(seed)
    xr = np.zeros((n, 576))
    for i in range(n):
        v = EDGE_VALUES[i % len(EDGE_VALUES)]
        dens = rng.uniform(0.0, 0.25)
        noisy = rng.random(576) < dens
        xr[i, noisy] = base * rng.uniform(0.3, 3.4 if v > 1 else 2.9, int(noisy.sum()))
        m = int(rng.integers(1, 5))
        p = rng.choice(576, m, replace=False) if i % 2 else rng.choice(200, m, replace=False)
        vals = np.concatenate([[v], rng.integers(1, v + 1, m - 1)])
        xr[i, p] = [base * level_of(int(x)) for x in vals]
        xr[i] *= rng.integers(0, 2, 576) * 2 - 1
    return _finish(xr)


def ties(seed, n, base=32768):
    """n dense spectra of the values 0..3 at the aimed step, each with its own share of zeros (book 13 codes a pair of zeros in one bit, book
    15 in three) and its own mix of the rest, up to a line of its own: the bit sums of the two candidate books of a region (13 and 15 below
    15: MP3_Encoder.py:1190-1231 -- x_len 16 of book 13 ends the scan at once) come close to each other and meet exactly."""
    rng = np.random.default_rng(seed)
    lv = np.array([0.5] + [level_of(v) for v in (1, 2, 3)])
    xr = np.zeros((n, 576))
    for i in range(n):
        z = rng.uniform(0.35, 0.65)              # (where the two sums of a region are close: book 15 wins below, 13 above)
        w = np.concatenate([[z], (1.0 - z) * rng.dirichlet(np.ones(3))])
        top = int(rng.integers(8, 577))
        xr[i, :top] = base * lv[rng.choice(4, top, p=w)] * (rng.integers(0, 2, top) * 2 - 1)
    return _finish(xr)
