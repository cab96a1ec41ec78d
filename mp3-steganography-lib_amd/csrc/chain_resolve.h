// The host's resolution of the rate loop's serial chains (enc_resolve, mp3s_encode_pipeline.cpp), the part that decides: which units ran on
// wrong inputs, which message variants a launch holds and which of them are taken, what an exact re-run is given.  No HIP call and no
// context in here -- enc_resolve moves the bytes and launches -- so that a stand-alone program can run it (tests/test_chain_resolve.py,
// against tests/chain_model.py).  The chains are the hide cursor (MP3_Encoder.py:808-809) and the per-(gr,ch) inherited address1/2/3 +
// quantizerStepSize (E7).
#pragma once
#include "mp3s_internal.h"

struct ChainResolver {
    struct Pending { int unit; int64_t cur; };   // first unit of a stream that ran on a wrong cursor, the right cursor there
    struct Span { size_t seg; int unit, count; int64_t cur; size_t entry; };   // units [unit, unit + count) of stream seg in a variant launch, entries from `entry` on
    // cursor / state: what each unit's current result was computed with; want / state_want: what the walk says it should be
    std::vector<int32_t> cursor, state, want, state_want;
    std::vector<int32_t> list;      // walk(): the units whose assumed inputs were wrong
    std::vector<Pending> pend;      // ... and, per stream, where the cursor first went wrong
    // one variant launch: its spans, its (unit, pattern) entries, the (entry, unit) pairs chosen from it
    std::vector<Span> spans;
    std::vector<int32_t> ent_unit, ent_cursor, pairs;
    std::vector<int32_t> redo_in;   // stage_entries(): [units | cursors | states], 24 bytes per entry

    // `in` = the host copy of the batch's input block: every unit's result so far was computed with the cursor written there and zero state
    void begin(const EncLayout &L, const std::vector<EncSeg> &segs, const uint8_t *in)
    {
        const int32_t *assumed = enc_block(L, in).cursor;
        cursor.assign(assumed, assumed + L.units);
        state.assign((size_t)L.units * 4, 0);
        list.clear();
        pend.assign(segs.size(), Pending{0, 0});
        want.assign(L.units, 0); state_want.assign((size_t)L.units * 4, 0);
    }

    // Stream by stream through the records: lists the units whose assumed inputs were wrong and, per stream, where the cursor first went
    // wrong; silent units get what they inherit; every stream's end goes into its EncSeg.  MP3S_OK, or MP3S_E_STEP_RANGE from the unit
    // that says so (what lies behind it is left as it was).
    int walk(mp3s_gr_out *gr, std::vector<EncSeg> &segs)
    {
        list.clear();
        for (size_t si = 0; si < segs.size(); si++) {
            EncSeg &s = segs[si];
            pend[si] = {-1, 0};
            int64_t cur = s.hide_base + cursor0(s);
            const int64_t end = (int64_t)s.hide_base + s.n_hide;
            int32_t chain[4][4] = {};   // [(ch*2+gr)][a1,a2,a3,step]
            if (s.carry_in) std::memcpy(chain, s.carry_in->chain, sizeof chain);
            bool own[4] = {false, false, false, false};   // the block has set chain[k] itself
            s.carry_used = cur < end;                     // the message is still being hidden when the block starts
            for (int u = s.first * 4; u < (s.first + s.n_frames) * 4; u++) {
                const int k = u & 3;
                mp3s_gr_out &g = gr[u];
                bool redo = false;
                const bool active = g.flags & MP3S_RF_ACTIVE;
                if (!own[k] && (!active || (g.flags & MP3S_RF_USED_ADDR_IN))) s.carry_used = true;
                if (active) own[k] = true;
                if (s.n_hide > 0 && active) {
                    const int64_t used = cursor[u];
                    if (used != cur && std::min<int64_t>(used, cur) < end) {
                        redo = true;
                        if (pend[si].unit < 0) pend[si] = {u, cur};
                    }
                }
                if ((g.flags & MP3S_RF_USED_ADDR_IN) &&
                    (state[(size_t)u * 4] != chain[k][0] || state[(size_t)u * 4 + 1] != chain[k][1] ||
                     state[(size_t)u * 4 + 2] != chain[k][2]))
                    redo = true;
                if (redo) list.push_back(u);
                want[u] = (int32_t)std::min<int64_t>(cur, kNoCursor);
                for (int j = 0; j < 4; j++) state_want[(size_t)u * 4 + j] = chain[k][j];
                if (active) {
                    cur += g.n_tables;
                    chain[k][0] = g.address[0]; chain[k][1] = g.address[1]; chain[k][2] = g.address[2];
                    chain[k][3] = g.quantizer_step;
                } else {   // silent unit: everything is inherited (quantizerStepSize and addresses pass through)
                    g.address[0] = chain[k][0]; g.address[1] = chain[k][1]; g.address[2] = chain[k][2];
                    g.quantizer_step = chain[k][3];
                }
                if (g.flags & MP3S_RF_STEP_RANGE) return fail(MP3S_E_STEP_RANGE, "quantizer step left the table in unit %d", u);
            }
            s.hide_offset = cur - s.hide_base;
            s.carry_out.cursor = s.hide_offset;
            std::memcpy(s.carry_out.chain, chain, sizeof chain);
        }
        return (int)MP3S_OK;
    }

    // The next variant launch: per stream with a pending unit a span, per span eight entries (the 3-bit patterns, 4 bytes apart in front of
    // the messages) for each of its units, variant-major; at most entry_cap entries (kVariantEntries).  false: no stream has anything left.
    bool plan_variants(const std::vector<EncSeg> &segs, int entry_cap)
    {
        spans.clear(); ent_unit.clear(); ent_cursor.clear(); pairs.clear();
        for (size_t si = 0; si < segs.size(); si++) {
            if (pend[si].unit < 0) continue;
            const EncSeg &s = segs[si];
            const int64_t end = (int64_t)s.hide_base + s.n_hide;
            if (pend[si].cur + 3 > end) { pend[si].unit = -1; continue; }   // only the message's last unit is left
            // as many units as the rest of the message can reach at 2.8 tables per unit (measured on music: 2.96; a stream
            // that takes fewer -- silent units take none -- simply comes round again), as many as still fit into this launch
            const int room = (entry_cap - (int)ent_unit.size()) / 8;
            const int count = (int)std::min<int64_t>({(int64_t)(s.first + s.n_frames) * 4 - pend[si].unit, (end - pend[si].cur) * 5 / 14 + 32, (int64_t)room});
            if (count <= 0) continue;                                       // next launch
            spans.push_back({si, pend[si].unit, count, pend[si].cur, ent_unit.size()});
            for (int v = 0; v < 8; v++)
                for (int j = 0; j < count; j++) { ent_unit.push_back(pend[si].unit + j); ent_cursor.push_back(4 * v); }
        }
        return !spans.empty();
    }

    // The launch has run: tables_of[e] = the table count of entry e.  Along every span the entry whose pattern is the message's three bits
    // at the unit's cursor is taken (pairs: entry, unit) and the cursor moves on by its tables.  true: another launch is needed.
    bool choose_variants(const std::vector<EncSeg> &segs, const uint8_t *hide_all, const uint8_t *tables_of)
    {
        bool more = false;
        for (const Span &sp : spans) {
            const EncSeg &s = segs[sp.seg];
            const int64_t end = (int64_t)s.hide_base + s.n_hide;
            int64_t cur = sp.cur;
            int j = 0;
            for (; j < sp.count && cur + 3 <= end; j++) {     // all three bits the unit can ask for exist
                const int u = sp.unit + j;
                const int v = (hide_all[cur] & 1) * 4 + (hide_all[cur + 1] & 1) * 2 + (hide_all[cur + 2] & 1);
                const size_t e = sp.entry + (size_t)v * sp.count + j;
                cursor[u] = (int32_t)cur;
                for (int q = 0; q < 4; q++) state[(size_t)u * 4 + q] = state_want[(size_t)u * 4 + q];
                pairs.push_back((int32_t)e); pairs.push_back(u);
                cur += tables_of[e];                           // (the entry's GrInfo goes to the unit's place on the device)
            }
            // span used up with message left: the stream goes on in the next launch; otherwise the message's last unit
            // (fewer than three bits left) and whatever lies behind it are the exact re-run's
            if (j == sp.count && cur < end && sp.unit + sp.count < (s.first + s.n_frames) * 4) { pend[sp.seg] = {sp.unit + sp.count, cur}; more = true; }
            else pend[sp.seg].unit = -1;
        }
        for (size_t si = 0; si < segs.size(); si++) more |= pend[si].unit >= 0;
        return more;
    }

    // redo_in = the entries of one launch, (unit, cursor) from the caller and the inherited state the walk wants for the unit
    void stage_entries(const std::vector<int32_t> &units_of, const std::vector<int32_t> &cursor_of)
    {
        const size_t nl = units_of.size();
        redo_in.resize(nl * 6);
        for (size_t i = 0; i < nl; i++) {
            const int u = units_of[i];
            redo_in[i] = u;
            redo_in[nl + i] = cursor_of[i];
            for (int j = 0; j < 4; j++) redo_in[2 * nl + 4 * i + j] = state_want[(size_t)u * 4 + j];
        }
    }

    // exact re-runs have come down (tmp[i] = the record of units_of[i], run on cur_of[i] and the state the walk wanted)
    void accept_reruns(const std::vector<int32_t> &units_of, const std::vector<int32_t> &cur_of, const std::vector<mp3s_gr_out> &tmp, mp3s_gr_out *gr)
    {
        for (size_t i = 0; i < units_of.size(); i++) {
            const int u = units_of[i];
            gr[u] = tmp[i];
            cursor[u] = cur_of[i];
            for (int q = 0; q < 4; q++) state[(size_t)u * 4 + q] = state_want[(size_t)u * 4 + q];
        }
    }
};
