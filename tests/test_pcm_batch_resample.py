"""PCM batches at a sampling rate of the caller's choosing (include/mp3s.h section vi-f, the calls that take a rate): the ratio rules
(pcm_resample_plan), k_pcm_batch_resample alone, Context.decode_batch(samplerate=...), Context.encode_batch(resample=...) and both as
torch tensors.

Every comparison is exact: == on integers and byte strings, bit patterns for float32.  No expected value runs new code: the resampled
rows are tests/wav_resample_model.py on the library's tap table (pinned to the model by tests/test_wav_resample.py), the batch is
tests/pcm_batch_model.py of them, the streams are Context.decode_streams' int16 and the MP3 bytes are Context.encode_pcm's."""
import ctypes as C
import functools
import itertools
import os
from math import gcd

import numpy as np
import pytest

import pcm_batch_model as M
import wav_resample_model as R
import wav_import_files as W
from test_list_calls_foreign import OPTIONS
from test_pcm_batch import ESZ, FMT, TOO_LONG, Dev, decoded_streams, file_list, random_pcm, same_bits
from test_vbr_streams import options

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MP3_RATES = (32000, 44100, 48000)
OUT_RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 96000)
E_TEXT = "Unsupported sampling frequency."


def model_plan(in_rate, out_rate):
    """the header's ratio rule in Python integers -> dict(L, M, taps, half), or None where it refuses (the table's own bound aside)"""
    g = gcd(in_rate, out_rate)
    L, M = out_rate // g, in_rate // g
    H = 16 if L >= M else -(-16 * M // L)
    return None if L > 1280 or 2 * H > 256 else dict(L=L, M=M, taps=2 * H, half=H)


@functools.lru_cache(maxsize=None)
def lib_taps(L, M):
    from mp3stego import _lib
    return _lib.wav_resample_taps(L, M).astype(np.int64)


def resampled(x, L, M):
    """int16 rows [n][nch] at L / M by the model's output rule on the library's table; 1 / 1 is the rows themselves"""
    x = np.asarray(x, dtype=np.int16)
    if L == M == 1:
        return x
    n_out, _ = R.counts(len(x), L, M)
    if n_out == 0:
        return np.zeros((0,) + x.shape[1:], dtype=np.int16)
    return R.resample(x, L, M, lib_taps(L, M))


# ------------------------------------------------------------------------------------------------ without a device
def test_symbols_and_records(mlib):
    L = mlib.lib()
    for s in ("mp3s_pcm_resample_plan", "mp3s_pcm_batch_resample_dev", "mp3s_pcm_batch_decode_files_at", "mp3s_pcm_batch_encode_at"):
        assert hasattr(L, s) and s in mlib.SYMBOLS, s
    want = {mlib.PcmResampleRatio: (16, None, dict(L=0, M=4, taps=8, half=12)),
            mlib.PcmResampleItem: (40, mlib.PCM_RESAMPLE_ITEM_DTYPE, dict(src_row=0, n_rows=8, first_row=16, slot=24, L=28, M=32, reserved=36)),
            mlib.PcmBatchInfoAt: (64, mlib.PCM_BATCH_INFO_AT_DTYPE, dict(n_frames=0, nch=4, sampling_rate=8, bit_rate=12, n_rows=16, first_row=24, valid_rows=32,
                                                                         in_rows=40, out_rate=48, L=52, M=56, reserved=60))}
    for rec, (size, dtype, offsets) in want.items():
        assert C.sizeof(rec) == size and [f for f, _ in rec._fields_] == list(offsets), rec
        for f, off in offsets.items():
            assert getattr(rec, f).offset == off, (rec, f)
        if dtype is not None:
            assert dtype.itemsize == size and list(dtype.names) == list(offsets) and all(dtype.fields[f][1] == off for f, off in offsets.items()), rec
    assert mlib.Context.OPTIONS["wav_resample"] == 21 and len(mlib.Context.KERNELS) == 9           # no new option, no new profile entry


def test_the_declarations_lie_inside_section_vi_f():
    txt = open(os.path.join(ROOT, "include", "mp3s.h")).read()
    body = txt[txt.index("(vi-f) PCM batches in the caller's device memory"):txt.index("(vii) asynchronous host-fed pipeline")]
    for s in ("int mp3s_pcm_resample_plan(", "int mp3s_pcm_batch_resample_dev(", "int mp3s_pcm_batch_decode_files_at(", "int mp3s_pcm_batch_encode_at(",
              "} mp3s_pcm_resample_ratio;", "} mp3s_pcm_resample_item;", "} mp3s_pcm_batch_info_at;"):
        assert body.count(s) == 1 and txt.count(s) == 1, s
    assert "(vi-g)" not in txt
    assert "resampled per channel FIRST and mixed afterwards" in body


def test_the_plan_is_the_models_arithmetic(mlib):
    pairs = [(i, o) for i in MP3_RATES for o in OUT_RATES]
    assert len([p for p in pairs if p[0] != p[1]]) == 27
    longest = 0
    for i, o in pairs:
        want = model_plan(i, o)
        assert want is not None and mlib.pcm_resample_plan(i, o) == want, (i, o)
        longest = max(longest, want["taps"])
        if i != o:                                                       # ... and the table's own bound holds for either half of every phase
            c = lib_taps(want["L"], want["M"])
            cut = 2 * (want["half"] // 2)
            assert c.shape == (want["L"], want["taps"]) and np.abs(c[:, :cut]).sum(axis=1).max() <= 65535 and np.abs(c[:, cut:]).sum(axis=1).max() <= 65535
    assert longest == 192
    assert mlib.pcm_resample_plan(44100, 16000) == dict(L=160, M=441, taps=90, half=45)
    assert mlib.pcm_resample_plan(48000, 8000) == dict(L=1, M=6, taps=192, half=96)
    assert mlib.pcm_resample_plan(48000, 48000)["L"] == mlib.pcm_resample_plan(48000, 48000)["M"] == 1
    for i, o in ((44100, 44101), (48000, 5000)):                         # L > 1280; T = 308
        assert model_plan(i, o) is None
        with pytest.raises(mlib.Mp3sError) as e:
            mlib.pcm_resample_plan(i, o)
        assert e.value.code == mlib.E_UNSUPPORTED, (i, o)
    g = gcd(48000, 5000)
    assert 2 * -(-16 * (48000 // g) // (5000 // g)) == 308
    r = mlib.PcmResampleRatio()
    for i, o in ((0, 16000), (-1, 16000), (44100, 0), (44100, -8000)):
        assert mlib.lib().mp3s_pcm_resample_plan(i, o, C.byref(r)) == mlib.E_ARG, (i, o)
    assert mlib.lib().mp3s_pcm_resample_plan(44100, 16000, None) == mlib.E_ARG


def test_the_plan_agrees_with_the_wav_resampler(mlib):
    """wherever both are defined the decode side's plan and the WAV path's give the same L, M, T"""
    x = np.zeros((4, 2), dtype=np.int16)
    n = 0
    for rate in (8000, 11025, 12000, 16000, 22050, 24000, 37800, 88200, 96000, 384000, 32000, 44100, 48000):
        for mode in (1, 32000, 44100, 48000):
            want = R.plan(rate, mode)
            try:
                got = mlib.wav_resample_info(W.wav_file(x, W.S16, rate=rate), 128, mode)
            except mlib.Mp3sError:
                assert want is None, (rate, mode)
                continue
            p = mlib.pcm_resample_plan(rate, got["out_rate"])
            assert (p["L"], p["M"], p["taps"], p["half"]) == (got["L"], got["M"], got["taps"], got["half"]) == (want["L"], want["M"], want["taps"], want["half"])
            n += 1
    assert n >= 40


def test_argument_checks_need_no_device(mlib):
    """the checks that answer before the context is looked at: stand-ins for the context and the arrays (never read)"""
    L = mlib.lib()
    mem = C.create_string_buffer(4096)
    p = (C.addressof(mem) + 255) & ~255
    pp = C.cast(p, C.POINTER(C.c_void_p))
    item = np.zeros(1, dtype=mlib.PCM_RESAMPLE_ITEM_DTYPE)
    item["L"], item["M"] = 160, 441
    one = (C.c_int64 * 1)(1)

    def resample_dev(**kw):
        a = dict(c=p, pcm=p, nch=2, h_items=item.ctypes.data, n=1, ch=2, fmt=0, T=8, out=p)
        a.update(kw)
        return L.mp3s_pcm_batch_resample_dev(*a.values())

    def decode_at(**kw):
        a = dict(c=p, mp3s=p, lens=p, n=1, rate=16000, first=None, T=8, ch=2, fmt=1, out=p, out_bytes=1 << 20, info=p, status=None)
        a.update(kw)
        return L.mp3s_pcm_batch_decode_files_at(*a.values())

    def encode_at(**kw):
        a = dict(c=p, d_in=p, n=1, ch=2, fmt=0, T=8, n_rows=one, rate=16000, mode=1, kbps=128, hide=None, n_hide=None, owner=pp, out=p, status=None)
        a.update(kw)
        return L.mp3s_pcm_batch_encode_at(*a.values())

    E = mlib.E_ARG
    for f, ptrs, chan in ((resample_dev, ("c", "pcm", "h_items", "out"), ("nch", "ch")), (decode_at, ("c", "mp3s", "lens", "info"), ("ch",)),
                          (encode_at, ("c", "d_in", "n_rows", "owner", "out"), ("ch",))):
        for k in ptrs:                                               # null pointers in turn
            assert f(**{k: None}) == E, (f.__name__, k)
        for k in chan:                                               # channel counts outside {1, 2}
            for v in (0, 3, -1):
                assert f(**{k: v}) == E, (f.__name__, k, v)
        for v in (2, -1, 7):                                         # an unknown format
            assert f(fmt=v) == E, (f.__name__, v)
        for v in (0, -5):
            assert f(T=v) == E, (f.__name__, "T", v)
            assert f(n=v) == E, (f.__name__, "n", v)
    # alignment to an element / a row, an item the kernel may not follow
    assert resample_dev(out=p + 1) == E and resample_dev(fmt=1, out=p + 2) == E and resample_dev(pcm=p + 2) == E and resample_dev(nch=1, pcm=p + 1) == E
    for field in ("src_row", "n_rows", "first_row", "slot"):
        bad = item.copy()
        bad[field] = -1
        assert resample_dev(h_items=bad.ctypes.data) == E, field
    for field in ("src_row", "n_rows", "first_row"):
        bad = item.copy()
        bad[field] = (1 << 40) + 1
        assert resample_dev(h_items=bad.ctypes.data) == E, field
    for lm, want in (((0, 1), E), ((1, -1), E), ((2, 2), mlib.E_UNSUPPORTED), ((320, 882), mlib.E_UNSUPPORTED),      # not in lowest terms
                     ((44101, 44100), mlib.E_UNSUPPORTED), ((5, 48), mlib.E_UNSUPPORTED)):                             # L > 1280; T = 308
        bad = item.copy()
        bad["L"], bad["M"] = lm
        assert resample_dev(h_items=bad.ctypes.data) == want, lm
    for v in (0, -16000):
        assert decode_at(rate=v) == E and b"out_rate" in L.mp3s_last_error()
        assert encode_at(rate=v) == E
    assert decode_at(out_bytes=2 * 8 * 4 - 1) == E and decode_at(first=(C.c_int64 * 1)(-1)) == E
    for v in (0, 2, -1, 16000, 22050):
        assert encode_at(mode=v) == E and b"mode" in L.mp3s_last_error(), v
    assert encode_at(hide=pp, n_hide=None) == E
    for rate in (44101, 400000):                                     # no target: L > 1280; T > 256
        assert R.plan(rate, 1) is None
        assert encode_at(rate=rate) == mlib.E_EXIT and L.mp3s_last_error() == E_TEXT.encode()
    assert encode_at(rate=16000, kbps=0) == mlib.E_UNSUPPORTED and encode_at(rate=16000, kbps=100) == mlib.E_UNSUPPORTED


# the model's own numbers, re-measured on the CPU when this was written (LSB of int16)
SINE_1K_DEVIATION = 4.0                                               # 1 kHz, amplitude 16 384, 44 100 -> 16 000 Hz: distance from the ideal sine
STOPBAND_PEAK = {(44100, 16000): (3, 3), (48000, 16000): (1, 1), (48000, 8000): (1, 4), (44100, 22050): (2, 1), (32000, 16000): (2, 1)}   # tones at 0.6, 0.75 of the output rate


def tone(rate, f, n, amp=16384):
    return np.rint(amp * np.sin(2 * np.pi * f * np.arange(n) / rate)).astype(np.int64)


def test_model_facts_for_down_ratios():
    """quality is a property of the model (the device equals it bit for bit): DC gain 1, a pass-band tone stays, stop-band tones go"""
    for L, M in ((160, 441), (1, 6), (1, 3), (147, 160)):
        c, _, _ = R.model_taps(L, M)
        edge = c.shape[1] * max(1, -(-L // M))
        for v in (32767, -32768, 12345):
            y = R.resample(np.full(3000, v, dtype=np.int16), L, M, c)
            assert len(y) > 2 * edge + 10 and (y[edge:len(y) - edge] == v).all(), (L, M, v)
    p = model_plan(44100, 16000)
    c, _, _ = R.model_taps(p["L"], p["M"])
    y = R.resample(tone(44100, 1000.0, 44100 // 4), p["L"], p["M"], c).astype(np.float64)
    edge = p["taps"]
    d = float(np.abs(y - 16384 * np.sin(2 * np.pi * 1000.0 * np.arange(len(y)) / 16000))[edge:len(y) - edge].max())
    assert abs(d - SINE_1K_DEVIATION) <= 0.01 and d <= 4.0, d
    for (i, o), recorded in STOPBAND_PEAK.items():
        p = model_plan(i, o)
        c, _, _ = R.model_taps(p["L"], p["M"])
        got = []
        for fr in (0.6, 0.75):
            y = R.resample(tone(i, fr * o, i // 4), p["L"], p["M"], c)
            got.append(int(np.abs(y[p["taps"]:len(y) - p["taps"]]).max()))
        assert tuple(got) == recorded and max(got) <= 4, (i, o, got)


def test_kernel_listing():
    """the compiler's listing of k_pcm_batch_resample: all 8 instantiations, no scratch, no spill; k_wav_resample and the committed
    resource table are as they were"""
    import json
    from test_build_resources import TABLE, resource_table, resource_usage
    usage = resource_usage()
    hits = sorted(k for k in usage if k.startswith("void mp3s::k_pcm_batch_resample<"))
    assert hits == sorted(f"void mp3s::k_pcm_batch_resample<{n}, {c}, {f}>" for n in (1, 2) for c in (1, 2) for f in ("false", "true")), hits
    for k in hits:
        u = usage[k]
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (k, u)
        assert u["VGPRs"] <= 64 and u["Occupancy [waves/SIMD]"] >= 4, (k, u)           # four workgroups of four waves a CU: LDS, not registers, sets the limit
    w = [k for k in usage if k.startswith("mp3s::k_wav_resample")]
    assert len(w) == 1 and usage[w[0]]["ScratchSize [bytes/lane]"] == 0 and usage[w[0]]["VGPRs Spill"] == 0 and usage[w[0]]["VGPRs"] <= 64
    if os.path.exists(TABLE):
        assert json.load(open(TABLE)) == resource_table(usage)


def test_tensors_refuse_the_new_arguments_before_anything_is_touched():
    torch = pytest.importorskip("torch")
    from mp3stego import tensors

    class NoContext:
        device = 0

        def __getattr__(self, name):
            raise AssertionError(f"the context was asked for {name}")

    t = torch.zeros((2, 2, 64), dtype=torch.int16)
    for bad in (0, -16000, 16000.0, "16000", True):
        with pytest.raises(ValueError, match="samplerate"):
            tensors.decode([b"", b""], samplerate=bad, ctx=NoContext())
        with pytest.raises(ValueError, match="samplerate"):
            tensors.encode(t, [64, 64], bad, resample=1, ctx=NoContext())
    for bad in (2, -1, 16000, 22050, True, "1"):
        with pytest.raises(ValueError, match="resample"):
            tensors.encode(t, [64, 64], 16000, resample=bad, ctx=NoContext())
    with pytest.raises(ValueError, match="is on cpu"):                 # the old refusals come behind the new ones
        tensors.decode([b"", b""], samplerate=16000, out=torch.zeros((2, 2, 64), dtype=torch.float32), ctx=NoContext())
    with pytest.raises(ValueError, match="is on cpu"):
        tensors.encode(t, [64, 64], 16000, resample=1, ctx=NoContext())


# ------------------------------------------------------------------------------------------------ k_pcm_batch_resample alone
RATIOS = ((1, 1), (2, 1), (1, 2), (160, 441), (147, 160), (1, 6), (441, 320))     # 160 / 441, 441 / 320: taps from global memory; 1 / 6: the longest filter
TILE = 1024                                                           # output elements of a plane a workgroup owns
T_VALUES = (1, 3, 8, 1151, 1153, 2 * TILE + 70)


def kernel_items(mlib, rng, nch):
    """per ratio one stream per input length, scattered over one buffer with garbage between them; an item per (stream, first_row);
    slots not monotone, two of them nobody's -> (items, pcm, resampled stream per item, n_slots)"""
    streams = []                                                      # (L, M, n_in)
    for L, M in RATIOS:
        two_tiles = -(-(2 * TILE + 60) * M // L)                      # an output of a little over two tiles: it crosses two tile boundaries
        streams += [(L, M, n) for n in (0, 1, 5, 1152, 1153, two_tiles)]
    order = rng.permutation(len(streams))
    at, src = {}, 37
    for k in order:
        at[k] = src
        src += streams[k][2] + int(rng.integers(3, 40))               # (odd and even starts: a mono stream begins in either half of a dword)
    pcm = rng.integers(-32768, 32768, size=(src + 64, nch), dtype=np.int64).astype(np.int16)
    outs = {}
    for k, (L, M, n) in enumerate(streams):
        pcm[at[k]:at[k] + n] = random_pcm(rng, n, nch)
        outs[k] = resampled(pcm[at[k]:at[k] + n], L, M)
        assert len(outs[k]) == -(-n * L // M)
    combos = [(k, f) for k in range(len(streams)) for f in sorted({0, 1, 3, max(len(outs[k]) - 1, 0), len(outs[k]), len(outs[k]) + 5})]
    slots = rng.permutation(len(combos) + 2)[:len(combos)]
    items = np.zeros(len(combos), dtype=mlib.PCM_RESAMPLE_ITEM_DTYPE)
    for i, ((k, f), b) in enumerate(zip(combos, slots)):
        items[i] = (at[k], streams[k][2], f, b, streams[k][0], streams[k][1], 0)
    return items, pcm, [outs[k] for k, _ in combos], len(combos) + 2


@gpu
@pytest.mark.parametrize("nch,channels,fmt", list(itertools.product((1, 2), (1, 2), FMT)))
def test_resample_kernel(ctx, mlib, nch, channels, fmt):
    rng = np.random.default_rng(5000 + 100 * nch + 10 * channels + FMT.index(fmt))
    items, pcm, streams, n_slots = kernel_items(mlib, rng, nch)
    assert len({(int(i["L"]), int(i["M"])) for i in items}) == len(RATIOS) and (np.diff(items["slot"]) < 0).any()
    free = sorted(set(range(n_slots)) - set(items["slot"].tolist()))
    assert len(free) == 2
    with Dev(ctx) as dev:
        d_pcm = dev.put(pcm)
        for T in T_VALUES:
            want, valid = M.batch(streams, items["first_row"].tolist(), T, channels, fmt, n_slots, items["slot"].tolist())
            d_out, read = dev.padded(want.nbytes, lead=ESZ[fmt])     # one element into the allocation: no plane starts on 16 bytes by design
            ctx.pcm_batch_resample_dev(d_pcm, nch, items, channels, fmt, T, d_out)   # ONE launch for all ratios
            got = read().view(M.DTYPES[fmt]).reshape(want.shape)     # (read() proves that nothing around the batch was written)
            assert (got[free].view(np.uint8) == 0x55).all(), "a slot of no item was written"
            got[free] = 0
            bits = np.uint16 if fmt == "i16" else np.uint32
            assert same_bits(got, want), (T, [(items[np.flatnonzero(items["slot"] == b)[0]].tolist(), c, t) for b, c, t in np.argwhere(got.view(bits) != want.view(bits))[:5]])
            for it, v in zip(items, valid):                          # the padding inside: zero
                assert not got[it["slot"], :, v:].any()


@gpu
def test_the_clamp_and_the_two_part_sums(ctx, mlib):
    """the worst input there is: full scale with the sign of every tap of a phase, left with it and right against it.  The row's sum
    is beyond +-2^31 for 2 / 1 (what ONE int32 accumulator would wrap), far outside int16 for 1 / 6; the clamp gives [32767, -32768],
    and their downmix is -1 as int16 and -1 / 65536 as float32"""
    cases = []
    for (L, Mr), want_overflow in (((2, 1), True), ((1, 6), False)):
        taps = lib_taps(L, Mr)
        H = taps.shape[1] // 2
        p_bad = int(np.abs(taps).sum(axis=1).argmax())
        assert (p_bad == 1 and np.abs(taps[p_bad]).sum() > 65535) if want_overflow else (L == 1 and np.abs(taps[0]).sum() > 32768)
        x = np.zeros((6000, 2), dtype=np.int16)
        x[:, 0] = np.where(np.arange(6000) % 64 < 32, 30000, -30000)
        x[:, 1] = -x[:, 0]
        rows = []
        for i0 in (1200, 3000):                                       # output row n with floor(n M / L) = i0 and phase p_bad: taps on x[i0 - H + 1 .. i0 + H]
            sign = np.where(taps[p_bad] >= 0, 32767, -32768)
            x[i0 - H + 1:i0 + H + 1, 0], x[i0 - H + 1:i0 + H + 1, 1] = sign, -1 - sign
            n = (i0 * L + p_bad) // Mr
            assert n * Mr // L == i0 and n * Mr % L == p_bad
            assert (abs(int((taps[p_bad] * x[i0 - H + 1:i0 + H + 1, 0].astype(np.int64)).sum())) > 1 << 31) == want_overflow
            rows.append(n)
        y = resampled(x, L, Mr)
        for n in rows:
            assert y[n].tolist() == [32767, -32768], (L, Mr, n)
        cases.append((L, Mr, x, y, rows))
    pcm = np.concatenate([c[2] for c in cases])
    items = np.zeros(2, dtype=mlib.PCM_RESAMPLE_ITEM_DTYPE)
    items[0] = (0, 6000, 0, 1, 2, 1, 0)
    items[1] = (6000, 6000, 0, 0, 1, 6, 0)
    T = 12000
    with Dev(ctx) as dev:
        d_pcm = dev.put(pcm)
        for channels, fmt in itertools.product((2, 1), FMT):
            want, _ = M.batch([c[3] for c in cases], [0, 0], T, channels, fmt, 2, [1, 0])
            d_out, read = dev.padded(want.nbytes)
            ctx.pcm_batch_resample_dev(d_pcm, 2, items, channels, fmt, T, d_out)
            got = read().view(M.DTYPES[fmt]).reshape(want.shape)
            assert same_bits(got, want), (channels, fmt)
            for slot, (L, Mr, x, y, rows) in zip((1, 0), cases):
                for n in rows:
                    v = got[slot, :, n].tolist()
                    if channels == 2:
                        assert v == ([32767, -32768] if fmt == "i16" else [32767 / 32768, -1.0])
                    else:
                        assert v == ([-1] if fmt == "i16" else [-1 / 65536])


# ------------------------------------------------------------------------------------------------ files in
def expected_at(mlib, ref, rate):
    """per file of the list: (the stream resampled to `rate`, its plan), None for a file that fails in front of the resampler, or the
    string "refused" for one whose rate the plan refuses"""
    out = []
    for r in ref:
        if isinstance(r, Exception):
            out.append(None)
            continue
        p = model_plan(r["sampling_rate"], rate)
        out.append("refused" if p is None else (resampled(r["pcm"], p["L"], p["M"]), p))
    return out


def check_decode_at(ctx, mlib, files, ref, rate, T, first_rows, channels, fmt, dev):
    names = list(files)
    exp = expected_at(mlib, ref, rate)
    nbytes = len(names) * channels * T * ESZ[fmt]
    d_out, read = dev.padded(nbytes)
    infos = ctx.decode_batch([files[n] for n in names], d_out, nbytes, T, first_rows, channels, fmt, per_file=True, samplerate=rate)
    want, valid = M.batch([e[0] if isinstance(e, tuple) else None for e in exp], first_rows, T, channels, fmt)
    got = read()
    assert got.tobytes() == want.tobytes(), (rate, T, [n for k, n in enumerate(names) if got.reshape(len(names), -1)[k].tobytes() != want[k].tobytes()])
    for n, i, r, e, first, v in zip(names, infos, ref, exp, first_rows, valid):
        if e is None:
            assert isinstance(i, mlib.Mp3sError) and i.code == r.code, n             # the codes of decode_streams
        elif e == "refused":
            assert isinstance(i, mlib.Mp3sError) and i.code == mlib.E_UNSUPPORTED, n
        else:
            assert i == {"n_frames": r["n_frames"], "channels": r["channels"], "sampling_rate": r["sampling_rate"], "bit_rate": r["bit_rate"],
                         "n_rows": len(e[0]), "first_row": first, "valid_rows": v, "in_rows": len(r["pcm"]), "out_rate": rate, "L": e[1]["L"], "M": e[1]["M"]}, n
    return exp


@gpu
@pytest.mark.parametrize("channels,fmt", list(itertools.product((1, 2), FMT)))
def test_decode_batch_at_a_rate(ctx, mlib, orc, channels, fmt):
    files = file_list(mlib)
    names = list(files)
    ref = decoded_streams(ctx, mlib, orc, files)
    with Dev(ctx) as dev:
        for rate in (16000, 44100):
            exp = expected_at(mlib, ref, rate)
            ratios = {(e[1]["L"], e[1]["M"]) for e in exp if isinstance(e, tuple)}
            assert ratios == ({(160, 441), (1, 3), (1, 2)} if rate == 16000 else {(1, 1), (147, 160), (441, 320)})
            rows = [len(e[0]) for e in exp if isinstance(e, tuple)]
            sized = ctx.batch_rows([files[n] for n in names], per_file=True, samplerate=rate)
            for s, e, r in zip(sized, exp, ref):
                if isinstance(e, tuple):
                    assert (s["n_rows"], s["valid_rows"], s["in_rows"], s["out_rate"], s["L"], s["M"]) == (len(e[0]), 0, len(r["pcm"]), rate, e[1]["L"], e[1]["M"])
                else:
                    assert isinstance(s, mlib.Mp3sError) and s.code == r.code
            first_rows = [0, 1, 1153, 0, 7, rows[5], min(rows) + 5, 3]   # 0, odd, a stream's whole length, behind the end
            assert first_rows[5] == len(exp[5][0])
            check_decode_at(ctx, mlib, files, ref, rate, min(rows) - 101, first_rows, channels, fmt, dev)
            check_decode_at(ctx, mlib, files, ref, rate, max(rows), [0] * len(names), channels, fmt, dev)


@gpu
def test_decode_batch_without_a_rate_is_the_call_as_it_was(ctx, mlib, orc):
    files = file_list(mlib)
    names = list(files)
    ref = decoded_streams(ctx, mlib, orc, files)
    first_rows, T = [0, 1, 1153, 0, 7, 23040, 0, 3], 4000
    want, valid = M.batch([None if isinstance(r, Exception) else r["pcm"] for r in ref], first_rows, T, 2, "f32")
    with Dev(ctx) as dev:
        nbytes = want.nbytes
        outs = []
        for kw in ({}, dict(samplerate=None)):
            d_out, read = dev.padded(nbytes)
            infos = ctx.decode_batch([files[n] for n in names], d_out, nbytes, T, first_rows, 2, "f32", per_file=True, **kw)
            outs.append((read().tobytes(), [i if isinstance(i, dict) else i.code for i in infos]))
        assert outs[0] == outs[1] and outs[0][0] == want.tobytes()
        for i, r, first, v in zip(outs[1][1], ref, first_rows, valid):
            if not isinstance(r, Exception):
                assert i == {"n_frames": r["n_frames"], "channels": r["channels"], "sampling_rate": r["sampling_rate"], "bit_rate": r["bit_rate"],
                             "n_rows": len(r["pcm"]), "first_row": first, "valid_rows": v}
        assert [s if isinstance(s, dict) else s.code for s in ctx.batch_rows([files[n] for n in names], per_file=True)] == \
            [s if isinstance(s, dict) else s.code for s in ctx.batch_rows([files[n] for n in names], per_file=True, samplerate=None)]


@gpu
def test_a_refused_rate_fails_its_file_alone(ctx, mlib, orc):
    files = file_list(mlib)
    names = list(files)
    ref = decoded_streams(ctx, mlib, orc, files)
    rates = {r["sampling_rate"] for r in ref if not isinstance(r, Exception)}
    assert rates == {32000, 44100, 48000}
    # 44 101: every file is refused (L > 1280).  5 000: the 48 kHz file (T = 308) -- and the 44.1 kHz files, whose T is 284 -- are
    # refused, the 32 kHz file is not.  5 880: the 48 kHz file alone (T = 262).  Which, is the model's arithmetic, not the library's
    assert [model_plan(r, 44101) for r in sorted(rates)] == [None] * 3
    assert [model_plan(r, 5000) is None for r in sorted(rates)] == [False, True, True]
    assert [model_plan(r, 5880) is None for r in sorted(rates)] == [False, False, True]
    with Dev(ctx) as dev:
        for rate in (44101, 5000, 5880):
            exp = check_decode_at(ctx, mlib, files, ref, rate, 700, [0, 1, 3, 0, 7, 0, 0, 3], 2, "i16", dev)
            assert "refused" in exp
        nbytes = 2 * 2 * 64 * 4
        d_out, read = dev.padded(nbytes)
        with pytest.raises(mlib.Mp3sError) as e:                     # without per_file the refused file fails the call
            ctx.decode_batch([files["32k"], files["48k"]], d_out, nbytes, 64, samplerate=5000)
        assert e.value.code == mlib.E_UNSUPPORTED
        with pytest.raises(mlib.Mp3sError) as e:                     # too small: nothing is touched
            ctx.decode_batch([files["32k"], files["48k"]], d_out, nbytes - 1, 64, samplerate=16000, per_file=True)
        assert e.value.code == mlib.E_ARG and (read() == 0x55).all()


@gpu
@pytest.mark.parametrize("opts", OPTIONS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_decode_batch_at_a_rate_under_options(ctx, mlib, orc, opts):
    files = file_list(mlib)
    ref = decoded_streams(ctx, mlib, orc, files)
    with Dev(ctx) as dev, options(ctx, **opts):
        check_decode_at(ctx, mlib, files, ref, 16000, 11000, [0, 1, 1153, 0, 7, 8000, 0, 3], 2, "f32", dev)


# ------------------------------------------------------------------------------------------------ batch in
E_ROWS = (1, 1151, 1153, 2305)
E_T = 2400


def encode_tensor(channels, fmt):
    from synth_pcm import synth_pcm
    pcm = synth_pcm(3, seed=91)                                      # int16 [3456][2]
    x = np.zeros((len(E_ROWS) + 1, channels, E_T), dtype=np.int16)
    for b in range(x.shape[0]):
        x[b] = np.roll(pcm, 173 * b, axis=0)[:E_T].T[:channels]
    if fmt == "i16":
        return x
    f = x.astype(np.float32) / np.float32(32768) + np.float32(0.25 / 32768)
    f[:, :, 5::97] = np.float32(1.5)                                 # clamped
    f[:, :, 9::101] = np.rint(f[:, :, 9::101] * 32768) / 32768 + np.float32(0.5 / 32768)   # ties
    f[:, :, E_T - 20:] = np.nan
    return f


@gpu
@pytest.mark.parametrize("channels,fmt", list(itertools.product((1, 2), FMT)))
@pytest.mark.parametrize("in_rate,mode,target", [(22050, 1, 44100), (16000, 1, 32000), (8000, 1, 32000), (44100, 48000, 48000)])
def test_encode_batch_at_a_rate_is_encode_pcm_of_the_model_frames(ctx, mlib, channels, fmt, in_rate, mode, target):
    x = encode_tensor(channels, fmt)
    lengths = list(E_ROWS) + [E_T + 1]                               # the last item: n_rows outside [1, T]
    p = R.plan(in_rate, mode)
    assert p["out_rate"] == target
    hidden = (channels + FMT.index(fmt)) % 2 == 0                    # with and without a hidden message
    messages = ["a", TOO_LONG, None, "in the fourth", "never looked at"] if hidden else None
    bits = [None if not hidden or m is None else np.array(mlib.message_frame(m), dtype=np.uint8) for m in (messages or [None] * 5)]
    with Dev(ctx) as dev:
        d_in = dev.put(x)
        got = ctx.encode_batch(d_in, len(lengths), channels, fmt, E_T, lengths, in_rate, 128, messages=messages, per_file=True, resample=mode)
        assert isinstance(got[4], mlib.Mp3sError) and got[4].code == mlib.E_ARG     # ... and it fails alone
        with pytest.raises(mlib.Mp3sError) as e:
            ctx.encode_batch(d_in, len(lengths), channels, fmt, E_T, lengths, in_rate, 128, messages=messages, resample=mode)
        assert e.value.code == mlib.E_ARG
    for k, n in enumerate(E_ROWS):
        rows = R.resample(M.frames(x[k], n)[:n], p["L"], p["M"], lib_taps(p["L"], p["M"]))
        want = ctx.encode_pcm(R.frames_of(rows), target, 128, bits[k])
        g = got[k]
        assert bytes(g["data"]) == want["mp3"], k
        assert (g["hide_offset"], g["too_long"], g["n_frames"], g["kbps"], g["sampling_rate"], g["channels"]) == \
            (want["hide_offset"], want["too_long"], (-(-n * p["L"] // p["M"]) + 1151) // 1152, 128, target, 2), k
    if hidden:
        assert got[1]["too_long"]


@gpu
def test_encode_batch_at_a_supported_rate_and_at_refused_ones(ctx, mlib):
    x = encode_tensor(2, "i16")
    lengths = list(E_ROWS)
    messages = ["a", None, "b", None]
    with Dev(ctx) as dev:
        d_in = dev.put(x)
        today = ctx.encode_batch(d_in, 4, 2, "i16", E_T, lengths, 44100, 128, messages=messages)
        auto = ctx.encode_batch(d_in, 4, 2, "i16", E_T, lengths, 44100, 128, messages=messages, resample=1)
        forced = ctx.encode_batch(d_in, 4, 2, "i16", E_T, lengths, 44100, 128, messages=messages, resample=44100)
        for a, b, c in zip(today, auto, forced):
            assert bytes(a["data"]) == bytes(b["data"]) == bytes(c["data"])
            assert all(a[k] == b[k] == c[k] for k in ("kbps", "sampling_rate", "channels", "n_frames", "too_long", "hide_offset"))
        # 7 350 Hz is a sixth of 44 100: the auto rule takes it there (L = 6).  No target exists where L > 1280 or T > 256
        p = R.plan(7350, 1)
        assert (p["out_rate"], p["L"], p["M"]) == (44100, 6, 1)
        got = ctx.encode_batch(d_in, 1, 2, "i16", E_T, [700], 7350, 128, resample=1)[0]
        want = ctx.encode_pcm(R.frames_of(R.resample(M.frames(x[0], 700)[:700], 6, 1, lib_taps(6, 1))), 44100, 128, None)
        assert bytes(got["data"]) == want["mp3"] and got["sampling_rate"] == 44100
        for rate in (44101, 400000):
            assert R.plan(rate, 1) is None
            with pytest.raises(mlib.Mp3sError) as e:
                ctx.encode_batch(d_in, 4, 2, "i16", E_T, lengths, rate, 128, resample=1, per_file=True)
            assert (e.value.code, e.value.text) == (mlib.E_EXIT, E_TEXT)
        with pytest.raises(mlib.Mp3sError) as e:                     # the bitrate is checked against the target
            ctx.encode_batch(d_in, 4, 2, "i16", E_T, lengths, 16000, 100, resample=1)
        assert e.value.code == mlib.E_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ torch
@gpu
def test_tensors_at_a_rate(ctx, mlib, orc):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no torch.cuda")
    from mp3stego import tensors
    files = file_list(mlib)
    names = [n for n in files if n not in ("refused", "none")]
    mp3s = [files[n] for n in names]
    batch, lengths, infos = tensors.decode(mp3s, samplerate=16000, channels=1, ctx=ctx)
    rows = [i["n_rows"] for i in infos]
    assert tuple(batch.shape) == (len(mp3s), 1, max(rows)) and batch.dtype == torch.float32 and lengths.tolist() == rows
    with Dev(ctx) as dev:
        nbytes = batch.numel() * 4
        d_out, read = dev.padded(nbytes)
        again = ctx.decode_batch(mp3s, d_out, nbytes, max(rows), None, 1, "f32", samplerate=16000)
        assert again == infos and read().tobytes() == batch.cpu().numpy().tobytes()
    got = tensors.encode(batch, lengths, 16000, bitrate=128, resample=1, ctx=ctx)
    back = ctx.decode_streams([bytes(g["data"]) for g in got], mlib.MP3S_PCM_I16)
    for g, b, n in zip(got, back, rows):
        assert g["sampling_rate"] == b["sampling_rate"] == 32000 and b["n_frames"] == g["n_frames"] == -(-(2 * n) // 1152), n
