#!/usr/bin/env python3
"""Golden for the decode transform at its parameter edges: the upstream reference's own re_quantize, __ms_stereo, __reorder,
__alias_reduction, imdct, __frequency_inversion and synth_filter_bank (decoder/Frame.py:265-286), driven exactly as gen_golden.run_chain
drives them, over the cases of tests/decode_edges.py -- the quick path's table boundary, both ends of the gain tables, every pair of channel
kinds, every block-type transition, a loud granule among quiet ones.  Runs the reference (build container only, refshim.py).

    python tests/golden/gen_decode_edges_golden.py      ->  tests/golden/g14_decode_edges.npz

Per case the fixture holds a digest of the builder's inputs, per frame a 64-bit blake2b of the frame's float64 PCM bytes, and the full PCM
of the case's first frame.  Nothing of the reference is copied: it is imported, and its functions are called.  A stream of a case is one
reference Frame object (zero overlap and fifo, Frame.py:234-235); streams run in parallel processes."""
import concurrent.futures
import io
import multiprocessing
import os
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (HERE, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

import decode_edges as E  # noqa: E402

OUT = os.path.join(HERE, "g14_decode_edges.npz")
SIZE_LIMIT = 663393                         # tests/golden/g6_synth128.npz, the largest fixture


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


def header_bytes(sr_code, nch, ms):
    """the four header bytes of a 128 kbps MPEG-1 layer III frame: stereo, joint stereo with the MS bit, or mono"""
    mode, mode_ext = (3, 0) if nch == 1 else ((1, 2) if ms else (0, 0))
    return [0xFF, 0xFB, (9 << 4) | (sr_code << 2), (mode << 6) | (mode_ext << 4)]


_RF = None


def _init():
    """a worker: the reference is imported here"""
    global _RF
    from refshim import load_reference
    load_reference()
    from mp3stego.decoder import Frame as RF
    _RF = RF


def _run_stream(job):
    """one stream of a case through the reference -> float64 PCM [n * 1152][nch]"""
    name, a, b = job
    RF = _RF
    isv, si_in, hdr_in, nch = E.cases()[name]
    fr = RF.Frame()
    out = []
    for f in range(a, b):
        fr.init_header_params(header_bytes(int(hdr_in["sr_idx"][f]), nch, int(hdr_in["ms_stereo"][f])))
        hdr = fr._Frame__header
        assert hdr.channels == nch
        si = fr.side_info
        for gr in range(2):
            for ch in range(nch):
                r = si_in[f, gr, ch]
                si.block_type[gr][ch] = int(r["block_type"])
                si.window_switching[gr][ch] = int(r["block_type"]) != 0
                si.mixed_block_flag[gr][ch] = bool(r["mixed_block_flag"])
                si.global_gain[gr][ch] = int(r["global_gain"])
                si.scale_fac_scale[gr][ch] = int(r["scalefac_scale"])
                si.pre_flag[gr][ch] = int(r["preflag"])
                si.sub_block_gain[gr][ch][:] = r["sub_block_gain"]
                si.scale_fac_l[gr][ch][:] = r["scale_fac_l"]
                si.scale_fac_s[gr][ch][:] = r["scale_fac_s"]
        fr._Frame__samples[:] = isv[f].astype(np.float64)
        fr._Frame__pcm = np.zeros((1152, nch))
        for gr in range(2):
            for ch in range(nch):
                RF.re_quantize(gr, ch, si.scale_fac_scale, si.block_type, si.mixed_block_flag, hdr.band_width.short_win, si.global_gain,
                               si.scale_fac_s, hdr.band_index.long_win, si.scale_fac_l, si.pre_flag, fr._Frame__samples, si.sub_block_gain)
            if hdr.channel_mode == RF.ChannelMode.JointStereo and hdr.mode_extension[0]:
                assert hdr_in["ms_stereo"][f]
                fr._Frame__ms_stereo(gr)
            else:
                assert not hdr_in["ms_stereo"][f]
            for ch in range(nch):
                if si.block_type[gr][ch] == 2 or si.mixed_block_flag[gr][ch]:
                    fr._Frame__reorder(gr, ch)
                else:
                    fr._Frame__alias_reduction(gr, ch)
                RF.imdct(gr, ch, si.block_type, fr._Frame__samples, fr._Frame__sine_block, fr._Frame__prev_samples)
                fr._Frame__frequency_inversion(gr, ch)
                RF.synth_filter_bank(gr, ch, fr._Frame__samples, fr._Frame__fifo, fr._Frame__synth_filter_bank_block)
        fr._Frame__interleave()
        out.append(np.array(fr.pcm, dtype=np.float64))
    return np.concatenate(out, axis=0)


def main():
    t0 = time.time()
    all_cases = E.cases()
    jobs = []
    for name, (_, _, hdr, _) in all_cases.items():
        first = hdr["stream_first"].astype(np.int64)
        starts = sorted(set(first.tolist()))
        assert starts[0] == 0 and all(first[s] == s for s in starts) and (np.diff(first) >= 0).all()
        for a, b in zip(starts, starts[1:] + [len(hdr)]):
            jobs.append((name, a, b))
    procs = max(1, min(int(os.environ.get("MP3S_GEN_JOBS", "8")), os.cpu_count() or 1))
    with concurrent.futures.ProcessPoolExecutor(procs, multiprocessing.get_context("spawn"), _init) as pool:
        parts = list(pool.map(_run_stream, jobs))
    names = list(all_cases)
    out = {"case_names": np.array(names), "in_digest": np.array([E.input_digest(all_cases[n]) for n in names], dtype=np.uint64),
           "n_frames": np.array([len(all_cases[n][2]) for n in names], dtype=np.int32)}
    digests = []
    for i, name in enumerate(names):
        pcm = np.concatenate([p for j, p in zip(jobs, parts) if j[0] == name], axis=0)
        assert pcm.shape == (len(all_cases[name][2]) * 1152, all_cases[name][3]) and np.isfinite(pcm).all()
        if name == "gain_range":
            # the int16 comparison of this case is to say something: no sample beyond the int32 the conversion goes through
            assert np.abs(pcm * 32767).max() < 2.0 ** 31, np.abs(pcm * 32767).max()
        digests.append(E.frame_digests(pcm))
        out["first_frame_%d" % i] = pcm[:1152].copy()
        print("%-24s %3d frames  max|pcm| %.4g" % (name, len(pcm) // 1152, np.abs(pcm).max()))
    out["frame_digest"] = np.concatenate(digests)                   # in the cases' order; case i starts at sum(n_frames[:i])
    save_npz(OUT, out)
    size = os.path.getsize(OUT)
    assert size <= SIZE_LIMIT, size
    n = int(out["n_frames"].sum())
    print("wrote", OUT, size, "bytes: %d cases, %d frames in %.0fs with %d processes" % (len(names), n, time.time() - t0, procs))


if __name__ == "__main__":
    main()
