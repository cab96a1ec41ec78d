"""The host's chain resolver (csrc/chain_resolve.h: ChainResolver, what enc_resolve of csrc/mp3s_encode_pipeline.cpp decides with) on the
CPU: a stand-alone program reads cases from a file, runs the resolver's methods and prints what they leave.
  walk()                              against chain_model.walk, the model the device's chain check is pinned to as well
  plan_variants() / choose_variants() against their statements in enc_resolve before the resolver existed, written out here
  stage_entries()                     against the [units | cursors | states] block, 24 bytes per entry
A case file is a flat array of little-endian int64 words; case after case, each beginning with its kind."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import chain_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mp3-steganography-lib_amd", "csrc")
ROCM_INCLUDE = "/opt/rocm/include"
COMPILE_FLAGS = ["-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", ROCM_INCLUDE]

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include "chain_resolve.h"

static char g_text[512];
int mp3s::fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_text, sizeof g_text, fmt, ap);
    va_end(ap);
    return code;
}

static std::vector<int64_t> g_words;
static size_t g_at = 0;
static int64_t next() { if (g_at >= g_words.size()) { fprintf(stderr, "case file ends early\n"); exit(3); } return g_words[g_at++]; }

template <class V> static void line(const char *name, const V &v)
{
    printf("%s", name);
    for (auto x : v) printf(" %lld", (long long)x);
    printf("\n");
}

// streams: n_frames first hide_base n_hide has_carry carry.cursor carry.chain[16]
static void read_segs(std::vector<EncSeg> &segs, std::vector<mp3s_carry> &carry)
{
    const size_t ns = (size_t)next();
    segs.assign(ns, EncSeg()); carry.assign(ns, mp3s_carry());
    for (size_t si = 0; si < ns; si++) {
        EncSeg &s = segs[si];
        s.n_frames = (int)next(); s.first = (int)next(); s.hide_base = (int)next(); s.n_hide = (int)next();
        const bool has = next() != 0;
        carry[si].cursor = next();
        for (int k = 0; k < 4; k++) for (int j = 0; j < 4; j++) carry[si].chain[k][j] = (int32_t)next();
        if (has) s.carry_in = &carry[si];
    }
}

// the resolver begun on a block that holds nothing but `units` assumed cursors, read from the file
static void begin(ChainResolver &R, const std::vector<EncSeg> &segs, int units)
{
    EncLayout L;
    L.units = units; L.o_cur = 16;
    std::vector<uint8_t> in(L.o_cur + (size_t)units * 4);
    int32_t *assumed = (int32_t *)(in.data() + L.o_cur);
    for (int u = 0; u < units; u++) assumed[u] = (int32_t)next();
    R.begin(L, segs, in.data());
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int64_t w;
    while (fread(&w, sizeof w, 1, f) == 1) g_words.push_back(w);
    fclose(f);
    ChainResolver R;   // one for all cases, as a context keeps one for all calls
    std::vector<EncSeg> segs;
    std::vector<mp3s_carry> carry;
    while (g_at < g_words.size()) {
        const int64_t kind = next();
        if (kind == 0) {          // walk: streams, units, assumed cursors, the state the units ran on, records (flags n_tables address[3] quantizer_step)
            read_segs(segs, carry);
            const int units = (int)next();
            begin(R, segs, units);
            for (int i = 0; i < units * 4; i++) R.state[(size_t)i] = (int32_t)next();
            std::vector<mp3s_gr_out> gr((size_t)units);
            for (auto &g : gr) {
                g = mp3s_gr_out();
                g.flags = (int32_t)next(); g.n_tables = (int32_t)next();
                for (int j = 0; j < 3; j++) g.address[j] = (int32_t)next();
                g.quantizer_step = (int32_t)next();
            }
            g_text[0] = 0;
            const int rc = R.walk(gr.data(), segs);
            printf("walk %d %d\ntext %s\n", rc, (int)MP3S_E_STEP_RANGE, g_text);
            line("list", R.list); line("want", R.want); line("state_want", R.state_want);
            std::vector<int64_t> rec, ends, pend;
            for (const auto &g : gr) for (int64_t x : {(int64_t)g.flags, (int64_t)g.n_tables, (int64_t)g.address[0], (int64_t)g.address[1], (int64_t)g.address[2], (int64_t)g.quantizer_step}) rec.push_back(x);
            for (size_t si = 0; si < segs.size(); si++) {
                const EncSeg &s = segs[si];
                ends.push_back(s.hide_offset); ends.push_back(s.carry_out.cursor); ends.push_back(s.carry_used ? 1 : 0);
                for (int k = 0; k < 4; k++) for (int j = 0; j < 4; j++) ends.push_back(s.carry_out.chain[k][j]);
                pend.push_back(R.pend[si].unit); pend.push_back(R.pend[si].cur);
            }
            line("records", rec); line("ends", ends); line("pend", pend);
        } else if (kind == 1) {   // variants: streams, units, entry cap, pend, state_want, the message array, launches x cap table counts
            read_segs(segs, carry);
            const int units = (int)next(), cap = (int)next();
            begin(R, segs, units);
            for (size_t si = 0; si < segs.size(); si++) { R.pend[si].unit = (int)next(); R.pend[si].cur = next(); }
            for (int i = 0; i < units * 4; i++) R.state_want[(size_t)i] = (int32_t)next();
            std::vector<uint8_t> hide((size_t)next());
            for (auto &b : hide) b = (uint8_t)next();
            const int launches = (int)next();
            std::vector<uint8_t> tables((size_t)launches * cap);
            for (auto &t : tables) t = (uint8_t)next();
            printf("variants\n");
            bool more = true;
            for (int l = 0; more; l++) {
                if (!R.plan_variants(segs, cap)) break;
                if (l >= launches || R.ent_unit.size() > (size_t)cap) return 4;
                line("ent_unit", R.ent_unit); line("ent_cursor", R.ent_cursor);
                more = R.choose_variants(segs, hide.data(), tables.data() + (size_t)l * cap);
                line("pairs", R.pairs); line("cursor", R.cursor); line("state", R.state);
                std::vector<int64_t> pend;
                for (const auto &p : R.pend) { pend.push_back(p.unit); pend.push_back(p.cur); }
                line("pend", pend);
                printf("more %d\n", more ? 1 : 0);
            }
            printf("end\n");
        } else if (kind == 2) {   // stage_entries: units, state_want, entries, their units, their cursors
            const int units = (int)next();
            R.state_want.resize((size_t)units * 4);
            for (auto &x : R.state_want) x = (int32_t)next();
            std::vector<int32_t> units_of((size_t)next()), cursor_of(units_of.size());
            for (auto &x : units_of) x = (int32_t)next();
            for (auto &x : cursor_of) x = (int32_t)next();
            R.stage_entries(units_of, cursor_of);
            printf("entries %zu\n", R.redo_in.size() * sizeof R.redo_in[0]);
            line("redo_in", R.redo_in);
        } else return 2;
    }
    return 0;
}
"""

RECORD = np.dtype([("flags", "<i4"), ("n_tables", "<i4"), ("address", "<i4", (3,)), ("quantizer_step", "<i4"), ("reserved0", "<i4")])
SEG = np.dtype([("first_frame", "<i4"), ("n_frames", "<i4"), ("hide_base", "<i4"), ("hide_begin", "<i4"), ("hide_end", "<i4"), ("chain_in", "<i4", (4, 4))])
PATTERN_BYTES = 32      # kPatternBytes: the messages begin behind the eight 3-bit patterns
E_STEP_RANGE = -6       # MP3S_E_STEP_RANGE


def compile_program(directory, extra_flags=()):
    """-> path of the program, or None without a host compiler or the HIP headers"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None or not os.path.isdir(ROCM_INCLUDE):
        return None
    src, exe = os.path.join(directory, "chain_resolve_cases.cpp"), os.path.join(directory, "chain_resolve_cases")
    with open(src, "w") as f:
        f.write(PROGRAM)
    r = subprocess.run([cxx] + COMPILE_FLAGS + list(extra_flags) + ["-o", exe, src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_program(exe, directory, words):
    """the program over the cases `words` -> its output split into cases: a list of {line name: [ints]} (launches of a variants case: a list of those)"""
    path = os.path.join(directory, "cases.bin")
    np.asarray(words, dtype="<i8").tofile(path)
    out = subprocess.run([exe, path], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    cases = []
    for ln in out.stdout.splitlines():
        name, _, rest = ln.partition(" ")
        if name in ("walk", "variants", "entries"):
            cases.append({"kind": name, "head": [int(x) for x in rest.split()], "launches": []})
        elif name == "text":
            cases[-1]["text"] = rest
        elif cases[-1]["kind"] == "variants":
            if name == "ent_unit":
                cases[-1]["launches"].append({})
            if name != "end":
                cases[-1]["launches"][-1][name] = [int(x) for x in rest.split()]
        else:
            cases[-1][name] = [int(x) for x in rest.split()]
    return cases


def seg_words(n_frames, n_hide, carries):
    """the streams of a batch as enc_layout lays them out -> (words, model segments)"""
    words, segs = [len(n_frames)], np.zeros(len(n_frames), dtype=SEG)
    first, base = 0, PATTERN_BYTES
    for si, (nf, nh, carry) in enumerate(zip(n_frames, n_hide, carries)):
        cursor, chain = carry if carry is not None else (0, np.zeros((4, 4), dtype=np.int64))
        words += [nf, first, base, nh, int(carry is not None), cursor] + [int(x) for x in np.asarray(chain).ravel()]
        begin = min(max(cursor, 0), cm.NO_CURSOR) if carry is not None else 0       # (cursor0 of csrc/mp3s_internal.h)
        segs[si] = (first, nf, base, base + begin, base + nh, np.asarray(chain) if carry is not None else 0)
        first, base = first + nf, base + nh
    return words, segs


# ------------------------------------------------------------------------------------------------ (a) the walk against the model
SHAPES = ((1,), (5,), (2, 1, 7))
MESSAGES = ("none", "ends inside", "too long", "two bits left")
SILENT = ("none", "start", "middle", "one chain")
ADDR_IN = ("none", "state is the chain", "state is not the chain")
CARRY = ("none", "inside", "negative cursor", "cursor past NO_CURSOR")
ASSUMED = ("true", "wrong behind the end", "no cursor")


def walk_case(rng, shape, message, silent, addr_in, carry, assumed, step_range_at=None):
    """-> (words of the case, what the model expects)"""
    units = 4 * sum(shape)
    rec = np.zeros(units, dtype=RECORD)
    rec["flags"] = cm.RF_ACTIVE
    rec["n_tables"] = rng.integers(0, 4, size=units)
    rec["address"] = rng.integers(0, 577, size=(units, 3))
    rec["quantizer_step"] = rng.integers(-100, 100, size=units)
    first = np.cumsum((0,) + shape)[:-1] * 4
    for u0, nf in zip(first, shape):
        n = nf * 4
        quiet = {"none": [], "start": range(min(3, n)), "middle": range(n // 2, min(n // 2 + 3, n)), "one chain": range(2, n, 4)}[silent]
        rec["flags"][[u0 + i for i in quiet]] = 0
    if addr_in != "none":
        rec["flags"][rng.random(units) < 0.4] |= cm.RF_USED_ADDR_IN
        rec["flags"][first] |= cm.RF_USED_ADDR_IN
    if step_range_at is not None:
        rec["flags"][step_range_at] |= cm.RF_STEP_RANGE
    taken = [int(rec["n_tables"][u0:u0 + nf * 4][(rec["flags"][u0:u0 + nf * 4] & cm.RF_ACTIVE) != 0].sum()) for u0, nf in zip(first, shape)]
    n_hide = [{"none": 0, "ends inside": max(t // 2, 1), "too long": t + 10, "two bits left": 2}[message] for t in taken]
    carries = []
    for nh in n_hide:
        chain = rng.integers(1, 577, size=(4, 4))
        at = {"inside": max(nh - 2, 1) if message == "two bits left" else min(3, nh), "negative cursor": -5, "cursor past NO_CURSOR": cm.NO_CURSOR + 7}.get(carry)
        carries.append(None if carry == "none" else (at, chain))
        if message == "two bits left" and carry == "inside":
            n_hide[len(carries) - 1] = nh = at + 2
    words, segs = seg_words(shape, n_hide, carries)
    rf = np.zeros(units // 4, dtype=[("stream", "<i4")])
    rf["stream"] = np.repeat(np.arange(len(shape)), shape)
    # what the chains really are does not depend on what the units were given: ask the model, then say what they were given
    true = cm.walk(rec, rf, segs, np.zeros(units, dtype=np.int64), state_in=np.zeros((units, 4), dtype=np.int32))
    true_cursor = np.concatenate([t["cursor"] for t in true])
    true_chain = np.concatenate([t["chain"] for t in true])
    end_of = np.repeat(segs["hide_end"].astype(np.int64), [4 * nf for nf in shape])
    cursors = {"true": np.minimum(true_cursor, cm.NO_CURSOR), "wrong behind the end": np.minimum(np.where(true_cursor < end_of, true_cursor, true_cursor + 5), cm.NO_CURSOR),
               "no cursor": np.full(units, cm.NO_CURSOR, dtype=np.int64)}[assumed]
    state = np.zeros((units, 4), dtype=np.int32)
    if addr_in != "none":
        state[:] = true_chain
    if addr_in == "state is not the chain":
        state[rng.random(units) < 0.5, rng.integers(0, 3)] += 1
    words += [units] +[int(x) for x in cursors] + [int(x) for x in state.ravel()]
    for r in rec:
        words += [int(r["flags"]), int(r["n_tables"])] + [int(x) for x in r["address"]] + [int(r["quantizer_step"])]
    model = cm.walk(rec, rf, segs, cursors, state_in=state)
    return [0] + words, (model, segs, cursors)


def check_walk(got, model, segs, cursors, case):
    assert got["head"][0] == 0, case
    assert got["list"] == [int(u) for m in model for u in m["faulted"]], case
    assert got["want"] == [min(int(c), cm.NO_CURSOR) for m in model for c in m["cursor"]], case
    assert got["state_want"] == [int(x) for m in model for x in m["chain"].ravel()], case
    want_rec = [[int(r["flags"]), int(r["n_tables"])] + [int(x) for x in r["address"]] + [int(r["quantizer_step"])] for m in model for r in m["records"]]
    assert got["records"] == [x for r in want_rec for x in r], case
    ends, pend = np.array(got["ends"]).reshape(len(model), 19), np.array(got["pend"]).reshape(len(model), 2)
    for si, m in enumerate(model):
        base, end = int(segs["hide_base"][si]), int(segs["hide_end"][si])
        assert ends[si, 0] == ends[si, 1] == m["end_cursor"] - base, (case, si)
        assert bool(ends[si, 2]) == m["carry_used"], (case, si)
        assert ends[si, 3:].tolist() == m["end_chain"].ravel().tolist(), (case, si)
        # the first faulted unit whose cursor was wrong, with the model's cursor there
        want_pend = (-1, 0)
        for u in m["faulted"]:
            used, c = int(cursors[u]), int(m["cursor"][u - m["first"]])
            if end > base and m["records"]["flags"][u - m["first"]] & cm.RF_ACTIVE and used != c and min(used, c) < end:
                want_pend = (int(u), c)
                break
        assert tuple(pend[si]) == want_pend, (case, si)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("chain_resolve"))
    exe = compile_program(d)
    if exe is None:
        pytest.skip("no host compiler or no HIP headers")
    return lambda words: run_program(exe, d, words)


def walk_cases():
    rng = np.random.default_rng(20)
    cases = []
    for combo in itertools.product(SHAPES, MESSAGES, SILENT, ADDR_IN, CARRY, ASSUMED):
        cases.append((combo,) + walk_case(rng, *combo))
    return cases


def test_walk_is_the_models_walk(program):
    cases = walk_cases()
    got = program([w for _, words, _ in cases for w in words])
    assert len(got) == len(cases)
    faulted = pended = 0
    for g, (combo, _, (model, segs, cursors)) in zip(got, cases):
        check_walk(g, model, segs, cursors, combo)
        faulted += bool(g["list"])
        pended += any(u >= 0 for u in g["pend"][::2])
    assert faulted > len(cases) // 4 and pended > len(cases) // 8      # (the cases do exercise the rules)


def test_walk_stops_at_a_step_out_of_range(program):
    rng = np.random.default_rng(21)
    words, (model, _, _) = walk_case(rng, (2, 1, 7), "ends inside", "middle", "state is the chain", "none", "true", step_range_at=9)
    got = program(words)[0]
    assert got["head"] == [E_STEP_RANGE, E_STEP_RANGE]
    assert got["text"] == "quantizer step left the table in unit 9"
    assert [m["step_range"] for m in model] == [False, True, False]


# ------------------------------------------------------------------------------------------------ (b) message variants
def parent_variants(segs, pend, cursor, state, state_want, hide_all, tables, cap):
    """The variant loop of enc_resolve as it stood before ChainResolver (plan: `spans.clear() ...` to `if (spans.empty()) break`, choice:
    `more = false` to `more |= pend[si].unit >= 0`), launch by launch; tables[l][e] = the table count the launch l reports for entry e.
    segs: (n_frames, first, hide_base, n_hide) per stream; pend: [unit, cur] per stream."""
    launches, more, l = [], True, 0
    while more:
        spans, ent_unit, ent_cursor, pairs = [], [], [], []
        for si, (n_frames, first, hide_base, n_hide) in enumerate(segs):
            if pend[si][0] < 0:
                continue
            end = hide_base + n_hide
            if pend[si][1] + 3 > end:
                pend[si][0] = -1
                continue
            room = (cap - len(ent_unit)) // 8
            count = min((first + n_frames) * 4 - pend[si][0], (end - pend[si][1]) * 5 // 14 + 32, room)
            if count <= 0:
                continue
            spans.append((si, pend[si][0], count, pend[si][1], len(ent_unit)))
            for v in range(8):
                for j in range(count):
                    ent_unit.append(pend[si][0] + j)
                    ent_cursor.append(4 * v)
        if not spans:
            break
        more = False
        for si, unit, count, cur, entry in spans:
            n_frames, first, hide_base, n_hide = segs[si]
            end = hide_base + n_hide
            j = 0
            while j < count and cur + 3 <= end:
                u = unit + j
                v = (hide_all[cur] & 1) * 4 + (hide_all[cur + 1] & 1) * 2 + (hide_all[cur + 2] & 1)
                e = entry + v * count + j
                cursor[u] = cur
                state[u * 4:u * 4 + 4] = state_want[u * 4:u * 4 + 4]
                pairs += [e, u]
                cur += tables[l][e]
                j += 1
            if j == count and cur < end and unit + count < (first + n_frames) * 4:
                pend[si] = [unit + count, cur]
                more = True
            else:
                pend[si][0] = -1
        more = more or any(p[0] >= 0 for p in pend)
        launches.append({"ent_unit": ent_unit, "ent_cursor": ent_cursor, "pairs": pairs, "cursor": list(cursor), "state": list(state),
                         "pend": [x for p in pend for x in p], "more": [int(more)]})
        l += 1
    return launches


VARIANT_CASES = {
    # name: (frames per stream, message bits per stream, pend (unit, bits of the message in front) per stream, entry cap, tables: None = random 0..3)
    "one stream whose span fits": ((5,), (20,), ((2, 0),), 8 * 64, None),
    "the second stream is cut by the room and comes round": ((5, 7), (90, 120), ((0, 0), (20, 4)), 8 * 24, None),
    "no room at all for the second stream in the first launch": ((5, 7), (90, 120), ((0, 0), (24, 0)), 8 * 20, None),
    "only the message's last unit is left: dropped before planning": ((3, 4), (40, 30), ((5, 38), (12, 1)), 8 * 64, None),
    "a span used up with message left (silence: no unit takes a table), then the stream's end": ((10,), (9,), ((0, 3),), 8 * 64, 0),
    "a span that reaches the stream's end with message left": ((2,), (400,), ((1, 7),), 8 * 64, None),
    "a stream that is not pending between two that are": ((2, 3, 2), (30, 30, 30), ((3, 2), (-1, 0), (21, 0)), 8 * 64, None),
}
MAX_LAUNCHES = 12


@pytest.mark.parametrize("name", list(VARIANT_CASES))
def test_variants_are_planned_and_chosen_as_before(program, name):
    shape, n_hide, pend_rel, cap, fixed = VARIANT_CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    units = 4 * sum(shape)
    words, segs = seg_words(shape, n_hide, [None] * len(shape))
    hide_all = rng.integers(0, 2, size=PATTERN_BYTES + sum(n_hide)).tolist()
    pend = [[u, int(segs["hide_base"][si]) + c if u >= 0 else 0] for si, (u, c) in enumerate(pend_rel)]
    assumed = rng.integers(0, 1000, size=units).tolist()
    state_want = rng.integers(0, 577, size=units * 4).tolist()
    tables = rng.integers(0, 4, size=(MAX_LAUNCHES, cap)) if fixed is None else np.full((MAX_LAUNCHES, cap), fixed)
    words = [1] + words + [units, cap] + assumed + [x for p in pend for x in p] + state_want + [len(hide_all)] + hide_all + [MAX_LAUNCHES] + [int(t) for t in tables.ravel()]
    got = program(words)[0]["launches"]
    want = parent_variants([(nf, int(s["first_frame"]), int(s["hide_base"]), nh) for nf, nh, s in zip(shape, n_hide, segs)], pend, list(assumed), [0] * (units * 4),
                           state_want, hide_all, tables.tolist(), cap)
    assert len(got) == len(want) and len(want) >= 1, (len(got), len(want))
    for l, (g, w) in enumerate(zip(got, want)):
        for key in ("ent_unit", "ent_cursor", "pairs", "cursor", "state", "pend", "more"):
            assert g[key] == w[key], (name, l, key)
    # the cases are what their names say
    if "comes round" in name or "no room" in name or "used up" in name:
        assert len(want) > 1 and want[0]["more"] == [1]
    if "no room" in name:
        assert set(want[0]["ent_unit"]) == set(range(20))
    if "dropped" in name:
        assert set(want[0]["ent_unit"]) == set(range(12, 28)) and len(want) == 1
    if "used up" in name:
        assert want[0]["pend"] == [34, PATTERN_BYTES + 3] and want[1]["more"] == [0]


# ------------------------------------------------------------------------------------------------ (c) the entries of a launch
@pytest.mark.parametrize("n_entries", [1, 5])
def test_entries_are_staged_as_units_cursors_states(program, n_entries):
    rng = np.random.default_rng(22 + n_entries)
    units = 12
    state_want = rng.integers(0, 577, size=(units, 4)).astype("<i4")
    units_of = rng.permutation(units)[:n_entries].astype("<i4")
    cursor_of = rng.integers(32, 5000, size=n_entries).astype("<i4")
    got = program([2, units] + state_want.ravel().tolist() + [n_entries] + units_of.tolist() + cursor_of.tolist())[0]
    block = np.concatenate([units_of, cursor_of, state_want[units_of].ravel()]).astype("<i4")
    assert got["head"] == [24 * n_entries] and block.nbytes == 24 * n_entries
    assert np.array_equal(np.array(got["redo_in"], dtype="<i4"), block)
