#!/usr/bin/env python3
"""Golden for the rate loop unit by unit: the upstream reference's own __iteration_loop (encoder/MP3_Encoder.py:760-815) run on units of
the case builders of tests/test_rate_units.py -- inherited address1/2/3 and quantizerStepSize, message cursors inside, at and behind the
message's end, budgets from 1 to 4095 bits, the boundaries of the table choice, the variant entries of the selection -- at 44.1, 48 and
32 kHz.  Runs the reference (build container only, refshim.py); the build (python __graft_entry__.py) must have been run, the case builders
need the host library and the oracle.

    python tests/golden/gen_rate_units_golden.py      ->  tests/golden/g12_rate_units.npz

How a unit reaches the reference: a live MP3Encoder on a one-frame WAV of the unit's sampling rate; its spectrum becomes mdct_freq of
(ch 0, gr 0), the other three units of the frame stay silent; __max_reservoir_bits is replaced on the instance by the unit's budget,
__resv_frame_end by nothing (it would add the frame's stuffing bits to part2_3_length of that very unit); address1/2/3, quantizerStepSize
and the message cursor are preset.  Nothing of the reference is copied: it is imported, and its methods are called by their mangled names.

Which units: of every case every fourth one, and the first 32 of every kind the case's builder counts (PER_KIND; every refused unit up to
64), found with the oracle -- the fixture holds their indices, tests/test_reference_rates.py counts the kinds again from the fixture's
own records.  Kinds that compare a unit with a run under other inputs (zero state, no message) bring that run along as the unit's twin.
The quantised lines are kept as max, sum and a 64-bit blake2b digest of |ix| as little-endian int16."""
import concurrent.futures
import copy
import hashlib
import importlib.util
import io
import multiprocessing
import os
import sys
import tempfile
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (HERE, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle_lib as orc  # noqa: E402
import spectra  # noqa: E402
import test_rate_units as RU  # noqa: E402

OUT = os.path.join(HERE, "g12_rate_units.npz")
GI_FIELDS = ["part2_3_length", "big_values", "count1", "global_gain", "scale_fac_compress", "region0_count", "region1_count", "preflag",
             "scale_fac_scale", "count1table_select", "part2_length", "address1", "address2", "address3", "quantizerStepSize"]
OWN, ZERO_STATE, NO_MESSAGE = 0, 1, 2       # a record's `twin`: the unit as the case has it / with zero state / without the message
STRIDE, PER_KIND, REFUSED = 4, 32, 64
SIZE_LIMIT = 663393                         # tests/golden/g6_synth128.npz, the largest fixture before this one
COMPARED = [b for _, b in RU.GI if b != "table_select"] + list(RU.ADDR)    # what same_result of tests/test_rate_units.py compares


def save_npz(path, arrays):
    """np.savez_compressed, but the members carry a fixed time stamp: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def load_project_lib():
    """the project's mp3stego/_lib.py under a name of its own: the reference's package is called mp3stego as well"""
    spec = importlib.util.spec_from_file_location("mp3s_project_lib", os.path.join(ROOT, "mp3-steganography-lib_amd", "mp3stego", "_lib.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.lib()
    return m


# ---------------------------------------------------------------------------------------------------------------- cases, shared with the tests
def cases(orc, mlib):
    """name -> Case of tests/test_rate_units.py, in the fixture's order"""
    out = {}
    for rate in RU.RATES:
        plain, hidden = RU.inherited_cases(orc, mlib, rate)
        first, second = RU.cursor_cases(orc, mlib, rate)
        for k, c in (("inherited_plain", plain), ("inherited_hidden", hidden), ("cursor_first", first), ("cursor_second", second),
                     ("budgets", RU.budget_case(orc, mlib, rate)), ("edges", RU.edge_case(orc, mlib, rate))):
            out["%d/%s" % (rate, k)] = c
    own, ent, _, eu, _ = RU.variant_case(orc, mlib)
    ent.units = eu                                                  # entry i is a run of unit eu[i] of `own`
    out["44100/variant_own"], out["44100/variant_entries"] = own, ent
    return out


def twin_inputs(c, kind):
    """the case with the inputs of a twin run (no oracle results)"""
    t = copy.copy(c)
    if kind == ZERO_STATE:
        t.state = None
    elif kind == NO_MESSAGE:
        t.hide, t.cursor = None, None
    t.want = t.ok = None
    return t


def oracle_run(orc, c):
    return orc.rate_units_from(c.rate, c.max_bits, c.xr, c.state, c.hide, c.cursor, c.hide_end)


def unit_inputs(c, u):
    """what the reference is given for unit u: (xr, state[4], message as a string of 0/1, cursor, budget).  The message ends at
    min(len(hide), hide_end); MP3S_NO_CURSOR is simply a cursor behind it."""
    state = np.zeros(4, dtype=np.int32) if c.state is None else np.asarray(c.state[u], dtype=np.int32)
    if c.hide is None:
        hide_str, cursor = "", 0
    else:
        end = max(min(len(c.hide), int(c.hide_end[u])), 0)
        assert np.asarray(c.hide[:end]).max(initial=0) <= 1
        hide_str, cursor = "".join(str(int(b)) for b in c.hide[:end]), 0 if c.cursor is None else int(c.cursor[u])
    return np.ascontiguousarray(c.xr[u], dtype=np.int32), state, hide_str, cursor, int(c.max_bits[u])


def digest64(b):
    return int.from_bytes(hashlib.blake2b(b, digest_size=8).digest(), "little")


def ix_digest(ix):
    """|ix| of one unit as little-endian int16"""
    return digest64(np.abs(np.asarray(ix)).astype("<i2").tobytes())


def input_digest(c, u):
    """the unit's inputs: a fixture made from other spectra, states or cursors than the builders give now is told apart"""
    xr, state, hide_str, cursor, max_bits = unit_inputs(c, u)
    return digest64(xr.astype("<i4").tobytes() + state.astype("<i4").tobytes() + np.array([cursor, max_bits, c.rate], dtype="<i8").tobytes() +
                    hide_str.encode())


# ---------------------------------------------------------------------------------------------------------------- kinds
def results_of_oracle(mlib, c, want):
    """the oracle's results of a case in the shape kinds() reads (every unit there)"""
    n = len(c.xr)
    gi = np.stack([want["gi"][k] for k in GI_FIELDS], axis=1).astype(np.int64)
    ts = want["gi"]["table_select"].astype(np.int64)
    ok = want["rc"] == 0
    sums = RU.region_sums(mlib.debug_tables(), want["ix"], want["gi"])
    small = ok & (want["ix"].max(1) < 15)
    return {"have": np.ones(n, dtype=bool), "ok": ok, "gi": gi, "ts": ts, "advance": want["advance"].astype(np.int64),
            "top": want["ix"].max(1).astype(np.int64), "ixd": np.array([ix_digest(r) for r in want["ix"]], dtype=np.uint64),
            "tie_regions": (small[:, None] & (ts == 15) & (sums[:, :, 0] == sums[:, :, 1])).sum(1)}


def same_result(a, b):
    """tests/test_rate_units.py same_result on two results of the shape above"""
    eq = (a["ixd"] == b["ixd"]) & (a["advance"] == b["advance"]) & (a["ok"] == b["ok"]) & (a["ts"] == b["ts"]).all(1)
    for f in COMPARED:
        k = GI_FIELDS.index(f)
        eq &= a["gi"][:, k] == b["gi"][:, k]
    return eq


def kinds(name, c, R, zero=None, nomsg=None, own=None):
    """kind -> bool [n]: the units of case `name` that are of that kind, by the conditions of the case's builder in tests/test_rate_units.py,
    from results R (zero / nomsg: of the twin runs, own: of 44100/variant_own for the entries' units); only units whose results are there"""
    what = name.split("/")[1]
    have, ok = R["have"], R["have"] & R["ok"]
    k = {"refused": have & ~R["ok"]}
    step, p23 = GI_FIELDS.index("quantizerStepSize"), GI_FIELDS.index("part2_3_length")
    if what.startswith("inherited"):
        act = (np.abs(c.xr).max(1) > 0) & ok & zero["have"] & zero["ok"]
        k["depends"] = act & ~same_result(R, zero)
        k["step_or_bits_change"] = k["depends"] & ((R["gi"][:, step] != zero["gi"][:, step]) | (R["gi"][:, p23] != zero["gi"][:, p23]))
    elif what.startswith("cursor"):
        adv, left = R["advance"], np.minimum(c.hide_end, len(c.hide)).astype(np.int64) - c.cursor
        took, by_end = ok & (adv > 0), c.hide_end < len(c.hide)
        k["two_left"], k["one_left"], k["none_left"] = took & ~by_end & (left == 2), took & ~by_end & (left == 1), took & ~by_end & (left <= 0)
        k["cut_by_hide_end"] = took & by_end & (left > 0) & (left < adv)
        k["swap_changes_a_table"] = ok & nomsg["have"] & nomsg["ok"] & (R["ts"] != nomsg["ts"]).any(1)
    elif what == "edges":
        edge, tie = np.char.startswith(c.labels, "escape_edges") & ok, np.char.startswith(c.labels, "ties") & ok
        for v in spectra.EDGE_VALUES:
            k["final_maximum_%d" % v] = edge & (R["top"] == v)
        for b in (3, 6, 8, 9, 11, 12, 13, 15):
            k["book_%d" % b] = tie & (R["ts"] == b).any(1)
        k["tie_13_15"] = ok & (R["tie_regions"] > 0)
    elif what == "variant_entries":
        eu = c.units
        k["tables_differ"] = ok & own["have"][eu] & own["ok"][eu] & (R["ts"] != own["ts"][eu]).any(1)
    return k


# which kinds bring which twin along / which the builders promise PER_KIND of (the rest is kept as met)
TWIN_OF = {"depends": ZERO_STATE, "step_or_bits_change": ZERO_STATE, "swap_changes_a_table": NO_MESSAGE}
PROMISED = {"inherited_plain": ("depends", "step_or_bits_change"), "inherited_hidden": ("depends", "step_or_bits_change"),
            "cursor_first": ("two_left", "one_left", "none_left", "swap_changes_a_table"),
            "cursor_second": ("cut_by_hide_end", "swap_changes_a_table"), "budgets": (), "edges": ("book_13", "book_15", "tie_13_15"),
            "variant_own": (), "variant_entries": ("tables_differ",)}


def choose(orc, mlib, all_cases):
    """-> list of (case name, unit, twin), sorted: every STRIDE-th unit of every case and the first PER_KIND of every kind"""
    picked = set()
    res = {name: results_of_oracle(mlib, c, c.want) for name, c in all_cases.items()}
    for name, c in all_cases.items():
        n = len(c.xr)
        u = np.arange(n)
        for v in u[(u + u // 4) % STRIDE == 0]:              # (not the same place in every frame)
            picked.add((name, int(v), OWN))
        what = name.split("/")[1]
        zero = nomsg = None
        if what.startswith("inherited"):
            t = twin_inputs(c, ZERO_STATE)
            zero = results_of_oracle(mlib, t, oracle_run(orc, t))
        if what.startswith("cursor"):
            t = twin_inputs(c, NO_MESSAGE)
            nomsg = results_of_oracle(mlib, t, oracle_run(orc, t))
        ks = kinds(name, c, res[name], zero, nomsg, res.get("44100/variant_own"))
        for kind, mask in ks.items():
            first = np.nonzero(mask)[0][:REFUSED if kind == "refused" else PER_KIND]
            if kind in PROMISED[what]:
                assert len(first) == PER_KIND, (name, kind, len(first))
            for v in first:
                picked.add((name, int(v), OWN))
                if kind in TWIN_OF:
                    picked.add((name, int(v), TWIN_OF[kind]))
                if kind == "tables_differ":
                    picked.add(("44100/variant_own", int(c.units[v]), OWN))
    order = list(all_cases)
    return sorted(picked, key=lambda r: (order.index(r[0]), r[1], r[2]))


# ---------------------------------------------------------------------------------------------------------------- the reference
class RefLoop:
    """one live reference encoder per sampling rate, driven a unit at a time"""

    def __init__(self, RE, RET, rate, workdir):
        self.RE, self.RET, self.budget = RE, RET, 0
        self.wav = os.path.join(workdir, "tiny_%d.wav" % rate)
        with open(self.wav, "wb") as f:
            f.write(orc.wav_bytes(np.zeros((1152, 2), dtype=np.int16), rate))
        self.fresh()

    def fresh(self):
        enc = self.RE.MP3Encoder(self.RE.WavReader(self.wav, 128))
        enc._MP3Encoder__max_reservoir_bits = lambda ch, gr: self.budget
        enc._MP3Encoder__resv_frame_end = lambda: None
        self.enc = enc

    def run(self, xr, state, hide_str, cursor, max_bits, want_sums):
        e = self.enc
        e._MP3Encoder__mdct_freq[:] = 0
        e._MP3Encoder__mdct_freq[0][0] = xr
        e._MP3Encoder__l3_enc[:] = 0
        tt = e._MP3Encoder__side_info.gr[0].ch[0].tt
        tt.address1, tt.address2, tt.address3, tt.quantizerStepSize = (int(v) for v in state)
        e._MP3Encoder__hide_str, e._MP3Encoder__hide_str_offset = hide_str, cursor
        self.budget = max_bits
        rec = {"error": "", "gi": np.zeros(len(GI_FIELDS), dtype=np.int32), "ts": np.zeros(3, dtype=np.int32), "advance": 0,
               "ix_max": 0, "ix_sum": 0, "ix_digest": 0, "sum13": np.full(3, -1, dtype=np.int32), "sum15": np.full(3, -1, dtype=np.int32)}
        try:
            e._MP3Encoder__iteration_loop()
        except Exception as ex:                                     # noqa: BLE001  (IndexError: the step left steptab)
            rec["error"] = type(ex).__name__
            self.fresh()
            return rec
        ix = np.asarray(e._MP3Encoder__l3_enc[0][0]).astype(np.int64)
        assert ix.min() >= 0 and ix.max() <= 8192
        rec["gi"][:] = [int(getattr(tt, k)) for k in GI_FIELDS]
        rec["ts"][:] = tt.table_select
        rec["advance"] = int(e._MP3Encoder__hide_str_offset) - cursor
        rec["ix_max"], rec["ix_sum"], rec["ix_digest"] = int(ix.max()), int(ix.sum()), ix_digest(ix)
        if want_sums and rec["ix_max"] < 15:
            # the two candidate books below 15 (:1227-1231), by the reference's own count_bit over the regions it chose
            bounds = [0, int(tt.address1), int(tt.address2), 2 * int(tt.big_values)]
            ixa = np.asarray(e._MP3Encoder__l3_enc[0][0])
            for r in range(3):
                for book, key in ((13, "sum13"), (15, "sum15")):
                    h = self.RET.huffman_table[book]
                    rec[key][r] = 0 if bounds[r + 1] <= bounds[r] else int(
                        self.RE.count_bit(ixa, bounds[r], bounds[r + 1], book, h.y_len, h.lin_bits, np.array(h.h_len)))
        return rec


_loops, _mods, _workdir = {}, None, None


def _init(workdir):
    """a worker: the reference is imported here, in a process that never loaded the project's library"""
    global _mods, _workdir
    from refshim import load_reference
    load_reference()
    from mp3stego.encoder import MP3_Encoder as RE
    from mp3stego.encoder import tables as RET
    _mods, _workdir = (RE, RET), workdir


def _work(chunk):
    rate, items = chunk
    if rate not in _loops:
        _loops[rate] = RefLoop(_mods[0], _mods[1], rate, _workdir)
    return [_loops[rate].run(*it) for it in items]


def main():
    t0 = time.time()
    orc.lib()
    mlib = load_project_lib()
    all_cases = cases(orc, mlib)
    names = list(all_cases)
    picked = choose(orc, mlib, all_cases)
    print("cases", len(names), "records", len(picked), "(twins %d)" % sum(1 for r in picked if r[2] != OWN), "chosen in %.1fs" % (time.time() - t0),
          flush=True)
    twins = {}
    work, in_digest = [], []
    for name, u, tw in picked:
        c = all_cases[name]
        if tw != OWN:
            c = twins.setdefault((name, tw), twin_inputs(c, tw))
        in_digest.append(input_digest(c, u))
        work.append((c.rate, unit_inputs(c, u) + (name.endswith("/edges"),)))
    t1 = time.time()
    with tempfile.TemporaryDirectory() as td:
        chunks, a = [], 0                                           # a chunk is of one sampling rate
        while a < len(work):
            b = a
            while b < len(work) and b - a < 40 and work[b][0] == work[a][0]:
                b += 1
            chunks.append((work[a][0], [w[1] for w in work[a:b]]))
            a = b
        jobs = max(1, min(int(os.environ.get("MP3S_GEN_JOBS", "8")), os.cpu_count() or 1))
        # fresh processes (spawn): a fork of this one would inherit the project's library and the threads of its runtime
        with concurrent.futures.ProcessPoolExecutor(jobs, multiprocessing.get_context("spawn"), _init, (td,)) as pool:
            recs = [r for part in pool.map(_work, chunks) for r in part]
    secs = time.time() - t1
    errors = sorted({r["error"] for r in recs})
    out = {"case_names": np.array(names), "gi_fields": np.array(GI_FIELDS), "error_names": np.array(errors),
           "case": np.array([names.index(r[0]) for r in picked], dtype=np.uint8), "unit": np.array([r[1] for r in picked], dtype=np.int32),
           "twin": np.array([r[2] for r in picked], dtype=np.uint8), "in_digest": np.array(in_digest, dtype=np.uint64),
           "error": np.array([errors.index(r["error"]) for r in recs], dtype=np.uint8),
           "gi": np.stack([r["gi"] for r in recs]), "table_select": np.stack([r["ts"] for r in recs]),
           "advance": np.array([r["advance"] for r in recs], dtype=np.int32), "ix_max": np.array([r["ix_max"] for r in recs], dtype=np.int32),
           "ix_sum": np.array([r["ix_sum"] for r in recs], dtype=np.int64), "ix_digest": np.array([r["ix_digest"] for r in recs], dtype=np.uint64),
           "sum13": np.stack([r["sum13"] for r in recs]), "sum15": np.stack([r["sum15"] for r in recs])}
    save_npz(OUT, out)
    size = os.path.getsize(OUT)
    assert size <= SIZE_LIMIT, size
    print("reference: %d units in %.0fs with %d processes (%.3fs a unit and process)" % (len(recs), secs, jobs, secs * jobs / len(recs)))
    for i, name in enumerate(names):
        m = out["case"] == i
        raised = m & (out["error"] != errors.index(""))
        print("%-28s pinned %4d  twins %3d  raised %3d %s" % (name, int((m & (out["twin"] == OWN)).sum()), int((m & (out["twin"] != OWN)).sum()),
                                                             int(raised.sum()), sorted({errors[e] for e in out["error"][raised]})))
    print("wrote", OUT, size, "bytes; all in %.0fs" % (time.time() - t0))


if __name__ == "__main__":
    main()
