"""The serial chains of the rate loop, restated on the host for the tests of the device's chain check and re-runs (csrc/k_chain.hpp,
k_rate_redo of csrc/k_rate.hpp).  Two things, kept apart:

  walk()          what the CHECK does with records somebody else computed: ChainResolver::walk of csrc/chain_resolve.h (the host's, compared
                  with this one in tests/test_chain_resolve.py), which k_chain_sum / k_chain_apply do as a scan.  It judges records, it
                  computes none.
  serial_truth()  what the records SHOULD be: the reference's order (ch outer, gr inner, frame by frame) with the oracle hook
                  oracle_lib.rate_units_from, one call per unit, the state of the unit's chain and the running cursor handed on.
  first_pass()    the same hook on what mp3s_rate_loop_dev is given without d_state_in: zero state, the caller's cursor guesses.

Units are u = frame * 4 + ch * 2 + gr; the chain of unit u is k = u & 3, the index of mp3s_chain_seg.chain_in."""
import numpy as np

RF_ACTIVE, RF_USED_ADDR_IN, RF_STEP_RANGE, RF_LOG_GUARD, RF_LISTED = 1, 2, 4, 8, 16     # MP3S_RF_* of include/mp3s.h
RF_ALL = RF_ACTIVE | RF_USED_ADDR_IN | RF_STEP_RANGE | RF_LOG_GUARD | RF_LISTED
NO_CURSOR = 0x3fffffff                                                                   # MP3S_NO_CURSOR


def pack3(a):
    """address1 | address2 << 10 | address3 << 20, as mp3s_gr_out.reserved0 keeps what a unit was given"""
    a = np.asarray(a)
    return a[..., 0] | (a[..., 1] << 10) | (a[..., 2] << 20)


def unpack3(w):
    w = np.asarray(w)
    return np.stack([w & 1023, (w >> 10) & 1023, (w >> 20) & 1023], axis=-1).astype(np.int32)


def stream_units(segs, s):
    f0, nf = int(segs["first_frame"][s]), int(segs["n_frames"][s])
    return f0 * 4, (f0 + nf) * 4


def walk(records, rf, segs, cursors, state_in=None):
    """The chain check on `records` (mp3s_gr_out [units]) that ran on `cursors` ([units] or None: nobody hides) and on the addresses
    `state_in` ([units][4]; None: what each record says it was given, reserved0 -- exactly as k_chain_apply reads them).
    -> one dict per stream:
         first, stop    its units are first .. stop - 1 of the batch
         faulted        the units (batch numbers) whose cursor or addresses were not the chain's, where that mattered
         cursor         int64 [n]: the cursor the walk finds in front of every unit
         chain          int32 [n][4]: address1..3 and quantizerStepSize it finds for every unit
         records        the stream's records, silent units given what they inherit
         step_range     some record has MP3S_RF_STEP_RANGE
         end_cursor, end_chain [4][4], carry_used   as mp3s_chain_seg_out"""
    assert len(rf) * 4 == len(records)
    out = []
    for s in range(len(segs)):
        u0, u1 = stream_units(segs, s)
        assert (rf["stream"][u0 // 4:u1 // 4] == s).all()
        rec = records[u0:u1].copy()
        flags, n_tables = rec["flags"].tolist(), rec["n_tables"].tolist()
        addr, step = rec["address"].tolist(), rec["quantizer_step"].tolist()
        given = (rec["reserved0"] if state_in is None else pack3(np.asarray(state_in)[u0:u1])).tolist()
        used_cur = None if cursors is None else np.asarray(cursors)[u0:u1].tolist()
        c, end = int(segs["hide_begin"][s]), int(segs["hide_end"][s])
        hiding = end > int(segs["hide_base"][s])
        assert not hiding or used_cur is not None
        chain = [list(map(int, row)) for row in segs["chain_in"][s]]
        own = [False] * 4
        carry_used = c < end
        faulted, cur_found, chain_found = [], np.zeros(u1 - u0, dtype=np.int64), np.zeros((u1 - u0, 4), dtype=np.int32)
        for i in range(u1 - u0):
            k = i & 3
            active, used_addr = bool(flags[i] & RF_ACTIVE), bool(flags[i] & RF_USED_ADDR_IN)
            if not own[k] and (not active or used_addr):
                carry_used = True
            redo = hiding and active and used_cur[i] != c and min(used_cur[i], c) < end
            if used_addr and given[i] != (chain[k][0] | (chain[k][1] << 10) | (chain[k][2] << 20)):
                redo = True
            if redo:
                faulted.append(u0 + i)
            cur_found[i] = c
            chain_found[i] = chain[k]
            if active:
                own[k] = True
                c += n_tables[i]
                chain[k] = addr[i] + [step[i]]
        silent = (rec["flags"] & RF_ACTIVE) == 0
        rec["address"][silent] = chain_found[silent, :3]
        rec["quantizer_step"][silent] = chain_found[silent, 3]
        out.append({"first": u0, "stop": u1, "faulted": np.array(faulted, dtype=np.int64), "cursor": cur_found, "chain": chain_found,
                    "records": rec, "step_range": bool((rec["flags"] & RF_STEP_RANGE).any()), "end_cursor": c,
                    "end_chain": np.array(chain, dtype=np.int32), "carry_used": bool(carry_used)})
    return out


def serial_truth(orc, rate, rf, xr, segs, hide):
    """The TRUE result of every unit: per stream from chain_in and hide_begin, units in batch order, each one call of the hook with the
    state of its chain and the running cursor (index into the batch's message array `hide`; None: nobody hides).
    -> {"gi": GRINFO_DTYPE [units], "ix": |ix| int32 [units][576], "rc", "advance", "en", "cursor": int64 [units] in front of each unit,
        "state": int32 [units][4] each unit was given, "end_cursor": [streams], "end_chain": int32 [streams][4][4]}"""
    units = len(xr)
    assert len(rf) * 4 == units
    t = {"gi": np.zeros(units, dtype=orc.GRINFO_DTYPE), "ix": np.zeros((units, 576), dtype=np.int32), "rc": np.zeros(units, dtype=np.int32),
         "advance": np.zeros(units, dtype=np.int32), "en": np.zeros((units, 22), dtype=np.int32), "cursor": np.zeros(units, dtype=np.int64),
         "state": np.zeros((units, 4), dtype=np.int32), "end_cursor": [], "end_chain": np.zeros((len(segs), 4, 4), dtype=np.int32)}
    for s in range(len(segs)):
        u0, u1 = stream_units(segs, s)
        chain = np.array(segs["chain_in"][s], dtype=np.int32)
        cursor = int(segs["hide_begin"][s])
        for u in range(u0, u1):
            k, f = u & 3, u >> 2
            r = orc.rate_units_from(rate, rf["max_bits"][f], xr[u], chain[k], hide, min(cursor, NO_CURSOR), rf["hide_end"][f])
            t["cursor"][u], t["state"][u] = cursor, chain[k]
            for key in ("gi", "ix", "rc", "advance", "en"):
                t[key][u] = r[key][0]
            gi = r["gi"][0]
            chain[k] = [gi["address1"], gi["address2"], gi["address3"], gi["quantizerStepSize"]]
            cursor += int(r["advance"][0])
        t["end_cursor"].append(cursor)
        t["end_chain"][s] = chain
    return t


def first_pass(orc, rate, rf, xr, hide=None, cursors=None):
    """what mp3s_rate_loop_dev computes without d_state_in: every unit on zero state and on the caller's cursor guess (None: nobody hides)"""
    frame = np.arange(len(xr)) // 4
    return orc.rate_units_from(rate, rf["max_bits"][frame], xr, None, hide, cursors, rf["hide_end"][frame])
