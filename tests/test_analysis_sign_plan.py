"""The plan by which k_enc_analysis computes a product once for filter coefficients that are equal up to SIGN (csrc/analysis_sign_plan.h,
written by tools/gen_analysis_sign_plan.py), checked on the CPU: the header is current, describes the reference's table, its zero argument
holds for the reference's window, and a numpy model of the kernel's fast path gives the direct sums bit for bit."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "mp3-steganography-lib_amd", "csrc", "analysis_sign_plan.h")


def read_plan():
    text = open(HEADER).read()
    text = text[text.index("#pragma once"):]

    def scalar(name):
        return int(re.search(name + r" = (0x[0-9a-f]+|-?\d+)", text).group(1), 0)

    def array(name):
        body = text.split(name + "[", 1)[1].split("= {", 1)[1].split("};", 1)[0]
        return [int(w, 0) for w in re.findall(r"0x[0-9a-f]+|-?\d+", body)]

    n = scalar("ANALYSIS_SIGN_PRODUCTS")
    return {"products": n, "stream": scalar("ANALYSIS_SIGN_STREAM"), "max_v2": scalar("ANALYSIS_SIGN_MAX_V2"),
            "zero_cols": scalar("ANALYSIS_SIGN_ZERO_COLS"), "first": array("ANALYSIS_SIGN_FIRST"),
            "neg": np.array(array("ANALYSIS_SIGN_NEG")).reshape(8, 4), "col": array("ANALYSIS_SIGN_COL")[:n],
            "set": array("ANALYSIS_SIGN_SET")[:n], "coef": array("ANALYSIS_SIGN_COEF")[:n]}


@pytest.fixture(scope="module")
def plan():
    return read_plan()


@pytest.fixture(scope="module")
def tables(golden_dir):
    g = np.load(os.path.join(golden_dir, "g1_tables.npz"))
    return g["enc_fl"].astype(np.int64).reshape(32, 64), g["enwindow"].astype(np.int64).reshape(512)


def v2(c):
    c = abs(int(c))
    return (c & -c).bit_length() - 1


def test_the_committed_header_is_current():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_analysis_sign_plan.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_plan_describes_the_reference_table(plan, tables):
    """re-derived from the golden enc_fl: every class is equal in absolute value with the stated signs, every coefficient that is not zero
    is fed exactly once, the count is the header's, no representative is INT_MIN, and a pass's products are ordered by their set"""
    fl, _ = tables
    assert plan["first"][0] == 0 and plan["first"][8] == plan["products"] == len(plan["col"])
    assert plan["stream"] % 32 == 0 and plan["products"] <= plan["stream"] < plan["products"] + 32
    fed = np.zeros((32, 64), dtype=int)
    neg = np.zeros((8, 4), dtype=int)
    zero_cols, vmax = 0, 0
    for p in range(8):
        o = [p, 15 - p, 16 + p, 31 - p]
        seen = []
        for n in range(plan["first"][p], plan["first"][p + 1]):
            k, s, c = plan["col"][n], plan["set"][n], plan["coef"][n]
            assert c != 0 and c != -2 ** 31 and s != 0
            feeds = [(j, (s >> (2 * j)) & 3) for j in range(4) if (s >> (2 * j)) & 3]
            assert all(f in (1, 3) for _, f in feeds) and feeds[0][1] == 1, (p, n)
            for j, f in feeds:
                assert fl[o[j]][k] == (c if f == 1 else -c), (p, n, j)
                fed[o[j]][k] += 1
                neg[p][j] += f == 3
            if s & 0xaa:
                zero_cols |= 1 << k
                vmax = max(vmax, v2(c))
            if not seen or seen[-1] != s:
                assert s not in seen, "a set's products stand together"
                seen.append(s)
    assert np.array_equal(fed, (fl != 0).astype(int))
    # grouping by absolute value from scratch gives the same number of products
    want = sum(len({abs(int(fl[i][k])) for i in (p, 15 - p, 16 + p, 31 - p)} - {0}) for p in range(8) for k in range(64))
    assert want == plan["products"] == 1030
    assert np.array_equal(neg, plan["neg"]) and zero_cols == plan["zero_cols"] and vmax == plan["max_v2"]


def test_a_window_sum_that_is_not_zero_never_gives_a_zero_low_word(plan, tables):
    """low32(y c) == 0 asks for y = 0 mod 2^(32 - v2(c)); |y| stays below that: eight terms of at most |enwindow| / 2 + 1 (|x << 16| <= 2^31)"""
    _, ew = tables
    ymax = max(sum(abs(int(ew[i + 64 * k])) / 2 + 1 for k in range(8)) for i in range(64))
    assert ymax < 2 ** (32 - plan["max_v2"])
    assert ymax < 2 ** 26          # (what the inputs of the model below are drawn from)


def direct(y, fl):
    """s[sb] = sum_k (y[k] * fl[sb][k]) >> 32 with int32 wrap-around; y: [n][64] -> [n][32]"""
    s = ((y[:, None, :] * fl[None, :, :]) >> 32).sum(axis=2)
    return ((s + 2 ** 31) % 2 ** 32 - 2 ** 31).astype(np.int64)


def shared(y, plan, per_product):
    """the kernel's fast path: one product per plan entry, singles into their output, shared ones into a partial sum folded where the set
    changes.  per_product: the exact correction -[low32(y c) != 0] with every negated use; otherwise the constant one the kernel applies."""
    out = np.zeros((y.shape[0], 32), dtype=np.int64)
    for p in range(8):
        o = [p, 15 - p, 16 + p, 31 - p]
        a = [np.full(y.shape[0], 0 if per_product else -int(plan["neg"][p][j]), dtype=np.int64) for j in range(4)]
        S, cur = None, None
        rng = range(plan["first"][p], plan["first"][p + 1])
        for n in rng:
            k, s, c = plan["col"][n], plan["set"][n], plan["coef"][n]
            prod = y[:, k] * c
            m = prod >> 32
            if s != cur:
                S, cur = np.zeros(y.shape[0], dtype=np.int64), s
            S = S + m
            if per_product:
                low = (prod & 0xffffffff) != 0
                for j in range(4):
                    if (s >> (2 * j)) & 3 == 3:
                        a[j] = a[j] - low
            if n + 1 == rng.stop or plan["set"][n + 1] != s:
                for j in range(4):
                    f = (s >> (2 * j)) & 3
                    if f == 1:
                        a[j] = a[j] + S
                    elif f == 3:
                        a[j] = a[j] - S
        for j in range(4):
            out[:, o[j]] = (a[j] + 2 ** 31) % 2 ** 32 - 2 ** 31
    return out


def test_model_of_the_fast_path_equals_the_direct_sums(plan, tables):
    fl, _ = tables
    rng = np.random.default_rng(3)
    y = rng.integers(-2 ** 26 + 1, 2 ** 26, size=(600, 64))
    y[y == 0] = 1
    edge = rng.choice(np.array([1, -1, 2 ** 26 - 1, -2 ** 26 + 1]), size=(600, 64))
    ones = rng.choice(np.array([1, -1]), size=(200, 64))
    for inp in (y, edge, ones):
        assert (inp != 0).all()
        want = direct(inp, fl)
        assert np.array_equal(shared(inp, plan, per_product=False), want)
        assert np.array_equal(shared(inp, plan, per_product=True), want)
    # zeros sprinkled in: the per-product correction is still exact, the constant one is not -- why a wave with a zero y takes the other way
    z = y.copy()
    z[rng.random(z.shape) < 0.1] = 0
    want = direct(z, fl)
    assert np.array_equal(shared(z, plan, per_product=True), want)
    assert not np.array_equal(shared(z, plan, per_product=False), want)
    # ... and only through columns that take part in a negated share
    z = y.copy()
    quiet = [k for k in range(64) if not (plan["zero_cols"] >> k) & 1]
    assert quiet
    z[:, quiet] = 0
    assert np.array_equal(shared(z, plan, per_product=False), direct(z, fl))
