"""PCM batches in the caller's device memory (include/mp3s.h section vi-f): k_pcm_batch and k_pcm_unbatch alone, a list of MP3 files
into a planar batch (Context.decode_batch), a batch into MP3 files (Context.encode_batch), and both as torch tensors
(mp3stego/tensors.py).

Every comparison is exact: == on integers, bit patterns for float32.  No expected value runs new code: tests/pcm_batch_model.py
(numpy, from the header's rules), Context.decode_streams and Context.encode_pcm (calls from before this section, pinned to the oracle
by the rest of the suite) and, for two streams, the oracle's own int16 (tests/oracle_lib.py)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import pcm_batch_model as M
from synth_pcm import synth_pcm
from test_list_calls_foreign import OPTIONS, stream_bytes
from test_vbr_streams import options, oracle_i16

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT = ("i16", "f32")
ESZ = {"i16": 2, "f32": 4}
PAD = 320                                                            # bytes kept around a result, prefilled with 0x55


# ------------------------------------------------------------------------------------------------ without a device
def test_symbols_and_records(mlib):
    L = mlib.lib()
    for s in ("mp3s_pcm_batch_dev", "mp3s_pcm_unbatch_dev", "mp3s_pcm_batch_decode_files", "mp3s_pcm_batch_encode"):
        assert hasattr(L, s) and s in mlib.SYMBOLS, s
    want = {mlib.PcmBatchItem: (32, mlib.PCM_BATCH_ITEM_DTYPE, dict(src_row=0, n_rows=8, first_row=16, slot=24, reserved=28)),
            mlib.PcmUnbatchItem: (24, mlib.PCM_UNBATCH_ITEM_DTYPE, dict(dst_frame=0, n_rows=8, slot=16, reserved=20)),
            mlib.PcmBatchInfo: (40, mlib.PCM_BATCH_INFO_DTYPE, dict(n_frames=0, nch=4, sampling_rate=8, bit_rate=12, n_rows=16, first_row=24, valid_rows=32))}
    for rec, (size, dtype, offsets) in want.items():
        assert C.sizeof(rec) == size == dtype.itemsize, rec
        assert [f for f, _ in rec._fields_] == list(offsets) == list(dtype.names)
        for f, off in offsets.items():
            assert getattr(rec, f).offset == off == dtype.fields[f][1], (rec, f)
    assert (mlib.BATCH_I16, mlib.BATCH_F32) == (0, 1)


def test_header_section_order():
    txt = open(os.path.join(ROOT, "include", "mp3s.h")).read()
    sections = re.findall(r"^/\* -{10,} \(([a-z-]+)\)", txt, flags=re.M)
    assert "vi-f" in sections and sections[sections.index("vi-f") - 1] == "vi-e" and sections[sections.index("vi-f") + 1] == "vii"
    body = txt[txt.index("(vi-f) PCM batches in the caller's device memory"):txt.index("(vii) asynchronous host-fed pipeline")]
    assert "replaces: none -- the reference writes a WAV file (decoder/decoder.py) and reads one (encoder/WAV_Reader.py)" in body
    for s in ("mp3s_pcm_batch_dev(", "mp3s_pcm_unbatch_dev(", "mp3s_pcm_batch_decode_files(", "mp3s_pcm_batch_encode(", "#define MP3S_BATCH_I16 0", "#define MP3S_BATCH_F32 1"):
        assert s in body, s


def test_argument_checks_need_no_device(mlib):
    """the checks that answer before the context is looked at: stand-ins for the context and the arrays (never read)"""
    L = mlib.lib()
    mem = C.create_string_buffer(4096)
    p = (C.addressof(mem) + 255) & ~255
    pp = C.cast(p, C.POINTER(C.c_void_p))
    item = np.zeros(1, dtype=mlib.PCM_BATCH_ITEM_DTYPE)
    uitem = np.zeros(1, dtype=mlib.PCM_UNBATCH_ITEM_DTYPE)
    uitem["n_rows"] = 1
    one = (C.c_int64 * 1)(1)

    def batch_dev(**kw):
        a = dict(c=p, pcm=p, nch=2, d_items=p, h_items=item.ctypes.data, n=1, ch=2, fmt=0, T=8, out=p)
        a.update(kw)
        return L.mp3s_pcm_batch_dev(*a.values())

    def unbatch_dev(**kw):
        a = dict(c=p, d_in=p, ch=2, fmt=0, T=8, d_items=p, h_items=uitem.ctypes.data, n=1, pcm=p)
        a.update(kw)
        return L.mp3s_pcm_unbatch_dev(*a.values())

    def decode_files(**kw):
        a = dict(c=p, mp3s=p, lens=p, n=1, first=None, T=8, ch=2, fmt=1, out=p, out_bytes=1 << 20, info=p, status=None)
        a.update(kw)
        return L.mp3s_pcm_batch_decode_files(*a.values())

    def encode(**kw):
        a = dict(c=p, d_in=p, n=1, ch=2, fmt=0, T=8, n_rows=one, rate=44100, kbps=128, hide=None, n_hide=None, owner=pp, out=p, status=None)
        a.update(kw)
        return L.mp3s_pcm_batch_encode(*a.values())

    E = mlib.E_ARG
    for f, ptrs, chan in ((batch_dev, ("c", "pcm", "d_items", "h_items", "out"), ("nch", "ch")), (unbatch_dev, ("c", "d_in", "d_items", "h_items", "pcm"), ("ch",)),
                          (decode_files, ("c", "mp3s", "lens", "info"), ("ch",)), (encode, ("c", "d_in", "n_rows", "owner", "out"), ("ch",))):
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
    assert batch_dev(nch=3) == E and b"nch" in L.mp3s_last_error()
    # alignment to an element / a row, an item the kernel may not follow, the encoder's frames on 16 bytes
    assert batch_dev(out=p + 1) == E and batch_dev(fmt=1, out=p + 2) == E and batch_dev(pcm=p + 2) == E and batch_dev(nch=1, pcm=p + 1) == E
    for field in ("src_row", "n_rows", "first_row", "slot"):
        bad = item.copy()
        bad[field] = -1
        assert batch_dev(h_items=bad.ctypes.data) == E, field
    assert unbatch_dev(pcm=p + 8) == E and unbatch_dev(d_in=p + 1) == E and unbatch_dev(fmt=1, d_in=p + 2) == E
    for field, v in (("dst_frame", -1), ("n_rows", 0), ("n_rows", 9), ("slot", -1)):
        bad = uitem.copy()
        bad[field] = v
        assert unbatch_dev(h_items=bad.ctypes.data) == E, (field, v)
    assert decode_files(out_bytes=2 * 8 * 4 - 1) == E                # out_bytes < n_files * C * T * element size
    assert decode_files(first=(C.c_int64 * 1)(-1)) == E
    assert encode(hide=pp, n_hide=None) == E


def test_model_on_the_edge_values():
    for (l, r), want_i16, want_f32 in M.DOWNMIX_EDGES:
        x = np.array([[l, r]], dtype=np.int16)
        assert M.plane_rows(x, 1, "i16").tolist() == [[want_i16]] and M.plane_rows(x, 1, "i16").dtype == np.int16
        f = M.plane_rows(x, 1, "f32")
        assert f.dtype == np.float32 and f[0, 0] == np.float32(want_f32) and float(f[0, 0]) == want_f32   # exact in float32
        assert M.plane_rows(x, 2, "i16").tolist() == [[l], [r]]
        assert M.plane_rows(x, 2, "f32").tolist() == [[l / 32768], [r / 32768]]
        assert M.plane_rows(x[:, :1], 2, "i16").tolist() == [[l], [l]]
    assert M.plane_rows(np.array([[-1, 0]], dtype=np.int16), 1, "f32")[0, 0] != M.plane_rows(np.array([[-1, 0]], dtype=np.int16), 1, "i16")[0, 0] / np.float32(32768)
    for k in (2, 3, 100, 101, -2, -3, -101, 32766):                  # (k + 0.5) / 32768: to the even neighbour
        assert M.float_to_i16(np.float32((k + 0.5) / 32768)) == (k if k % 2 == 0 else k + 1), k
    for x, want in M.FLOAT_EDGES:
        assert M.float_to_i16(np.float32(x)) == want, x
    out, valid = M.batch([np.arange(10, dtype=np.int16).reshape(5, 2), None], [3, 0], 4, 2, "i16")
    assert valid == [2, 0] and out.tolist() == [[[6, 8, 0, 0], [7, 9, 0, 0]], [[0] * 4] * 2]
    fr = M.frames(np.array([[0.5, np.nan, -2.0, 9.0]], dtype=np.float32), 3)
    assert fr.shape == (1152, 2) and fr[:4].tolist() == [[16384, 16384], [0, 0], [-32768, -32768], [0, 0]] and not fr[4:].any()


def test_tensors_refuse_before_anything_is_touched():
    """the three refusals of mp3stego.tensors, in both directions: they answer before the library is called (a stand-in for the context)"""
    torch = pytest.importorskip("torch")
    from mp3stego import tensors

    class NoContext:
        device = 0

        def __getattr__(self, name):
            raise AssertionError(f"the context was asked for {name}")

    for t, why in ((torch.zeros((2, 2, 64), dtype=torch.float64), "dtype"), (torch.zeros((2, 2, 64), dtype=torch.float32), "is on cpu"),
                   (torch.zeros((2, 2, 128), dtype=torch.int16)[:, :, ::2], "not contiguous")):
        with pytest.raises(ValueError, match=why):
            tensors.decode([b"", b""], out=t, ctx=NoContext())
        with pytest.raises(ValueError, match=why):
            tensors.encode(t, [64, 64], 44100, ctx=NoContext())


# ------------------------------------------------------------------------------------------------ device helpers
class Dev:
    """device allocations of a test, freed when it ends"""

    def __init__(self, ctx):
        self.ctx, self.held = ctx, []

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.ctx.sync()
        for p in self.held:
            self.ctx.free(p)

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        self.held.append(self.ctx.to_device(arr if arr.nbytes else np.zeros(16, dtype=np.uint8)))
        return self.held[-1].value

    def padded(self, nbytes, lead=0):
        """nbytes of result room, PAD + lead bytes of 0x55 in front and PAD behind -> (address of the room, read())"""
        total = PAD + lead + nbytes + PAD
        base = self.put(np.full(total, 0x55, dtype=np.uint8))

        def read():
            raw = self.ctx.download(base, np.uint8, (total,))
            assert (raw[:PAD + lead] == 0x55).all() and (raw[PAD + lead + nbytes:] == 0x55).all(), "bytes around the result were written"
            return raw[PAD + lead:PAD + lead + nbytes]
        return base + PAD + lead, read


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def random_pcm(rng, rows, nch):
    x = rng.integers(-32768, 32768, size=(rows, nch), dtype=np.int64).astype(np.int16)
    if rows >= 4:
        x[1], x[rows - 2] = -32768, 32767                            # both extremes in both channels
        x[2, 0], x[2, -1] = 32767, -32768
    elif rows:
        x[0] = -32768
    return x


# ------------------------------------------------------------------------------------------------ k_pcm_batch alone
N_ROWS = (0, 1, 5, 1152, 1153, 2311)
T_VALUES = (1, 3, 8, 1151, 1153)


def batch_items(mlib, rng):
    """one stream per n_rows, scrambled in one buffer on frame boundaries; an item per (stream, first_row); slots not monotone"""
    order = rng.permutation(len(N_ROWS))
    at, src = {}, 3 * 1152                                           # (rows in front of the first stream: never read)
    for k in order:
        at[N_ROWS[k]] = src
        src += (N_ROWS[k] + 1151) // 1152 * 1152 + 1152
    combos = [(n, f) for n in N_ROWS for f in sorted({0, 1, 3, max(n - 1, 0), n, n + 5})]
    slots = rng.permutation(len(combos) + 2)[:len(combos)]           # (two slots belong to no item: they stay as they were)
    items = np.zeros(len(combos), dtype=mlib.PCM_BATCH_ITEM_DTYPE)
    for i, ((n, f), b) in enumerate(zip(combos, slots)):
        items[i] = (at[n], n, f, b, 0)
    return items, at, src, len(combos) + 2


@gpu
@pytest.mark.parametrize("nch,channels,fmt", list(itertools.product((1, 2), (1, 2), FMT)))
def test_pcm_batch_kernel(ctx, mlib, nch, channels, fmt):
    rng = np.random.default_rng(1000 + 100 * nch + 10 * channels + FMT.index(fmt))
    items, at, total, n_slots = batch_items(mlib, rng)
    pcm = rng.integers(-32768, 32768, size=(total, nch), dtype=np.int64).astype(np.int16)   # garbage between the streams
    for n, src in at.items():
        pcm[src:src + n] = random_pcm(rng, n, nch)
    streams = [pcm[it["src_row"]:it["src_row"] + it["n_rows"]] for it in items]
    with Dev(ctx) as dev:
        d_pcm, d_items = dev.put(pcm), dev.put(items)
        for T in T_VALUES:
            want, valid = M.batch(streams, items["first_row"].tolist(), T, channels, fmt, n_slots, items["slot"].tolist())
            assert valid == [int(min(max(n - f, 0), T)) for n, f in zip(items["n_rows"], items["first_row"])]
            d_out, read = dev.padded(want.nbytes, lead=ESZ[fmt])     # one element into the allocation: no plane starts on 16 bytes by design
            ctx.pcm_batch_dev(d_pcm, nch, d_items, items, channels, fmt, T, d_out)
            got = read().view(M.DTYPES[fmt]).reshape(want.shape)
            free = sorted(set(range(n_slots)) - set(items["slot"].tolist()))
            assert (got[free].view(np.uint8) == 0x55).all(), "a slot of no item was written"
            got[free] = 0
            assert same_bits(got, want), (T, np.argwhere(got.view(np.uint16 if fmt == "i16" else np.uint32) != want.view(np.uint16 if fmt == "i16" else np.uint32))[:5])
            for it, v in zip(items, valid):                          # the padding inside: zero
                assert not got[it["slot"], :, v:].any()


# ------------------------------------------------------------------------------------------------ k_pcm_unbatch alone
U_ROWS = (1, 1151, 1152, 1153, 2305)
U_T = 2400


def unbatch_tensor(rng, channels, fmt):
    if fmt == "i16":
        x = rng.integers(-32768, 32768, size=(len(U_ROWS) + 1, channels, U_T), dtype=np.int64).astype(np.int16)
        x[:, :, 0] = -32768
        return x
    x = (rng.random((len(U_ROWS) + 1, channels, U_T)) * 2.4 - 1.2).astype(np.float32)
    x[:, :, ::7] = np.rint(x[:, :, ::7] * 32768) / 32768 + np.float32(0.5 / 32768)    # ties
    special = np.array([e[0] for e in M.FLOAT_EDGES], dtype=np.float32)
    x[:, :, :1] = special[0]
    for b in range(x.shape[0]):
        n = min(len(special), (U_ROWS + (U_T,))[b])
        x[b, :, :n] = special[:n]
        x[b, -1, :n] = special[:n][::-1]
    x[:, :, U_T - 40:] = np.nan                                      # garbage behind every n_rows
    return x


@gpu
@pytest.mark.parametrize("channels,fmt", list(itertools.product((1, 2), FMT)))
def test_pcm_unbatch_kernel(ctx, mlib, channels, fmt):
    rng = np.random.default_rng(2000 + 10 * channels + FMT.index(fmt))
    x = unbatch_tensor(rng, channels, fmt)
    slots = [4, 0, 3, 1, 5]                                          # (slot 2 belongs to no item)
    frames_of = [(n + 1151) // 1152 for n in U_ROWS]
    order, dst, at = rng.permutation(len(U_ROWS)), 2, {}             # sentinel frames in front, between and behind
    for k in order:
        at[k] = dst
        dst += frames_of[k] + (1 if k % 2 else 0)
    n_frames = dst + 2
    items = np.zeros(len(U_ROWS), dtype=mlib.PCM_UNBATCH_ITEM_DTYPE)
    for k, n in enumerate(U_ROWS):
        items[k] = (at[k], n, slots[k], 0)
    want = np.full((n_frames, 1152, 2), 0x5555, dtype=np.int16)
    for k, n in enumerate(U_ROWS):
        want[at[k]:at[k] + frames_of[k]] = M.frames(x[slots[k]], n).reshape(frames_of[k], 1152, 2)
    with Dev(ctx) as dev:
        d_items = dev.put(items)
        for lead in (0, ESZ[fmt]):                                   # the tensor on a 16-byte boundary, and one element off it
            d_in = dev.put(np.concatenate([np.zeros(lead, dtype=np.uint8), x.view(np.uint8).reshape(-1)])) + lead
            d_pcm, read = dev.padded(want.nbytes)
            assert d_pcm % 16 == 0
            ctx.pcm_unbatch_dev(d_in, channels, fmt, U_T, d_items, items, d_pcm)
            got = read().view(np.int16).reshape(want.shape)
            assert same_bits(got, want), (lead, np.argwhere(got != want)[:5])


# ------------------------------------------------------------------------------------------------ files in
def file_list(mlib):
    """name -> bytes; which one repeats its last frame is asked of the host scan, not assumed"""
    files = {"cbr": stream_bytes("cbr"), "mono": stream_bytes("a_44_mono"), "48k": stream_bytes("a_48_stereo"), "32k": stream_bytes("a_32_stereo"),
             "inherit_0": stream_bytes("inherit_0"), "cut": stream_bytes("own_cbr") + b"\x00" * 700, "refused": stream_bytes("f_to_mono_late"),
             "none": None}
    w = {n: mlib.parse_stream(f) for n, f in files.items() if f is not None and n != "refused"}
    assert [n for n in w if w[n]["dup_last_frame"]] == ["cut"]
    assert w["mono"]["channels"] == 1 and w["48k"]["sampling_rate"] == 48000 and w["32k"]["sampling_rate"] == 32000
    assert not mlib.scan_stream(files["inherit_0"])["gpu_ok"]
    return files


_decoded = {}


def decoded_streams(ctx, mlib, orc, files):
    """Context.decode_streams per file (int16), once; for two of the streams the oracle's own int16 stands in its place"""
    if not _decoded:
        names = list(files)
        out = ctx.decode_streams([files[n] for n in names if files[n] is not None], mlib.MP3S_PCM_I16, per_file=True)
        out = [r if isinstance(r, Exception) else dict(r, pcm=np.array(r["pcm"])) for r in out]   # (copies: the cache outlives the call's owner)
        out.insert(names.index("none"), mlib.Mp3sError(mlib.E_ARG, "null"))
        for n in ("cbr", "cut"):
            o = orc.decode(files[n])
            assert o["rc"] == 0 and np.array_equal(oracle_i16(o), out[names.index(n)]["pcm"])
            out[names.index(n)] = dict(out[names.index(n)], pcm=oracle_i16(o))
        assert len(out[names.index("cut")]["pcm"]) == 1152 * (out[names.index("cut")]["n_frames"] + 1)
        _decoded["out"] = out
    return _decoded["out"]


def check_decode_batch(ctx, mlib, files, ref, T, first_rows, channels, fmt, dev):
    names = list(files)
    nbytes = len(names) * channels * T * ESZ[fmt]
    d_out, read = dev.padded(nbytes)
    infos = ctx.decode_batch([files[n] for n in names], d_out, nbytes, T, first_rows, channels, fmt, per_file=True)
    streams = [None if isinstance(r, Exception) else r["pcm"] for r in ref]
    want, valid = M.batch(streams, first_rows, T, channels, fmt)
    got = read()
    assert got.tobytes() == want.tobytes(), [n for k, n in enumerate(names) if got.reshape(len(names), -1)[k].tobytes() != want[k].tobytes()]
    for n, i, r, first, v in zip(names, infos, ref, first_rows, valid):
        if isinstance(r, Exception):
            assert isinstance(i, mlib.Mp3sError) and i.code == r.code, n     # the codes of decode_streams
            continue
        assert i == {"n_frames": r["n_frames"], "channels": r["channels"], "sampling_rate": r["sampling_rate"], "bit_rate": r["bit_rate"],
                     "n_rows": len(r["pcm"]), "first_row": first, "valid_rows": v}, n
    return got


@gpu
@pytest.mark.parametrize("channels,fmt", list(itertools.product((1, 2), FMT)))
def test_decode_batch_of_a_mixed_list(ctx, mlib, orc, channels, fmt):
    files = file_list(mlib)
    names = list(files)
    ref = decoded_streams(ctx, mlib, orc, files)
    assert isinstance(ref[names.index("refused")], mlib.Mp3sError) and ref[names.index("refused")].code == mlib.E_UNSUPPORTED
    sized = ctx.batch_rows([files[n] for n in names], per_file=True)
    rows = [len(r["pcm"]) for r in ref if not isinstance(r, Exception)]
    for s, r in zip(sized, ref):
        if isinstance(r, Exception):
            assert isinstance(s, mlib.Mp3sError) and s.code == r.code                # (both are refused by the front end)
        else:
            assert (s["n_rows"], s["valid_rows"], s["n_frames"], s["channels"]) == (len(r["pcm"]), 0, r["n_frames"], r["channels"])
    largest = max(s["n_rows"] for s in sized if not isinstance(s, Exception))
    assert largest == max(rows)
    first_rows = [0, 1, 1153, 0, 7, 23040, min(rows) + 5, 3]          # 0, odd, a stream's whole frames (the repeated frame is left), behind the end
    with Dev(ctx) as dev:
        check_decode_batch(ctx, mlib, files, ref, min(rows) - 101, first_rows, channels, fmt, dev)
        check_decode_batch(ctx, mlib, files, ref, largest, [0] * len(names), channels, fmt, dev)


@gpu
def test_decode_batch_refusals(ctx, mlib, orc):
    files = file_list(mlib)
    some = [files["cbr"], files["refused"], files["mono"]]
    with Dev(ctx) as dev:
        nbytes = 3 * 2 * 64 * 4
        d_out, read = dev.padded(nbytes)
        with pytest.raises(mlib.Mp3sError) as e:                     # without per_file the refused file fails the call
            ctx.decode_batch(some, d_out, nbytes, 64)
        assert e.value.code == mlib.E_UNSUPPORTED
        with pytest.raises(mlib.Mp3sError) as e:                     # a null file before any work at all
            ctx.decode_batch([files["cbr"], None], d_out, nbytes, 64)
        assert e.value.code == mlib.E_ARG
        d_out, read = dev.padded(nbytes)
        with pytest.raises(mlib.Mp3sError) as e:                     # too small: nothing is touched
            ctx.decode_batch(some, d_out, nbytes - 1, 64, per_file=True)
        assert e.value.code == mlib.E_ARG and (read() == 0x55).all()
        with pytest.raises(mlib.Mp3sError) as e:
            ctx.decode_batch(some, d_out, nbytes, 64, first_rows=[0, -1, 0], per_file=True)
        assert e.value.code == mlib.E_ARG and (read() == 0x55).all()


@gpu
@pytest.mark.parametrize("opts", OPTIONS, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_decode_batch_under_options(ctx, mlib, orc, opts):
    files = file_list(mlib)
    ref = decoded_streams(ctx, mlib, orc, files)
    first_rows = [0, 1, 1153, 0, 7, 23040, 0, 3]
    with Dev(ctx) as dev, options(ctx, **opts):
        check_decode_batch(ctx, mlib, files, ref, 30000, first_rows, 2, "f32", dev)


# ------------------------------------------------------------------------------------------------ batch in
E_ROWS = (3456, 2305, 700)
E_T = 3500
TOO_LONG = "does not fit " * 150


def encode_tensor(channels, fmt):
    pcm = synth_pcm(4, seed=77)                                      # int16 [4608][2]
    x = np.zeros((len(E_ROWS) + 1, channels, E_T), dtype=np.int16)
    for b in range(x.shape[0]):
        x[b] = np.roll(pcm, 311 * b, axis=0)[:E_T].T[:channels]
    if fmt == "i16":
        return x
    f = x.astype(np.float32) / np.float32(32768) + np.float32(0.25 / 32768)
    f[:, :, 5::97] = np.float32(1.5)                                 # clamped
    f[:, :, 9::101] = np.rint(f[:, :, 9::101] * 32768) / 32768 + np.float32(0.5 / 32768)   # ties
    f[:, :, E_T - 20:] = np.nan
    return f


@gpu
@pytest.mark.parametrize("channels,fmt,rate,kbps", [(2, "i16", 44100, 128), (1, "f32", 48000, 320)])
@pytest.mark.parametrize("hide", ["none", "messages"])
def test_encode_batch_is_encode_pcm_of_the_model_frames(ctx, mlib, channels, fmt, rate, kbps, hide):
    x = encode_tensor(channels, fmt)
    lengths = list(E_ROWS) + [0]                                     # the last item: n_rows outside [1, T]
    messages = None if hide == "none" else ["a", TOO_LONG, None, "never looked at"]
    bits = [None] * 4 if messages is None else [None if m is None else np.array(mlib.message_frame(m), dtype=np.uint8) for m in messages]
    with Dev(ctx) as dev:
        d_in = dev.put(x)
        got = ctx.encode_batch(d_in, len(lengths), channels, fmt, E_T, lengths, rate, kbps, messages=messages, per_file=True)
        assert isinstance(got[3], mlib.Mp3sError) and got[3].code == mlib.E_ARG
        with pytest.raises(mlib.Mp3sError) as e:                     # ... which fails the call without per_file
            ctx.encode_batch(d_in, len(lengths), channels, fmt, E_T, lengths, rate, kbps, messages=messages)
        assert e.value.code == mlib.E_ARG
        with pytest.raises(mlib.Mp3sError) as e:
            ctx.encode_batch(d_in, 3, channels, fmt, E_T, lengths[:3], 22050, kbps)
        assert e.value.code == mlib.E_UNSUPPORTED
    for k, n in enumerate(E_ROWS):
        want = ctx.encode_pcm(M.frames(x[k], n), rate, kbps, bits[k])
        g = got[k]
        assert bytes(g["data"]) == want["mp3"], k
        assert (g["hide_offset"], g["too_long"], g["n_frames"], g["kbps"], g["sampling_rate"], g["channels"]) == \
            (want["hide_offset"], want["too_long"], (n + 1151) // 1152, kbps, rate, 2), k
    if messages is not None:
        assert got[1]["too_long"] and 0 < got[1]["hide_offset"] < len(bits[1]) and got[0]["hide_offset"] > 0


@gpu
def test_round_trip_on_the_device(ctx, mlib):
    data = stream_bytes("cbr")
    ref = ctx.decode_streams([data], mlib.MP3S_PCM_I16)[0]
    T = len(ref["pcm"])
    with Dev(ctx) as dev:
        d, read = dev.padded(2 * T * 2)
        info = ctx.decode_batch([data], d, 2 * T * 2, T, channels=2, fmt="i16")[0]
        assert info["valid_rows"] == info["n_rows"] == T == ctx.batch_rows([data])[0]["n_rows"]
        got = ctx.encode_batch(d, 1, 2, "i16", T, [T], 44100, 320)[0]
        assert np.array_equal(read().view(np.int16).reshape(2, T), ref["pcm"].T)
    assert bytes(got["data"]) == ctx.encode_pcm(ref["pcm"], 44100, 320, None)["mp3"]


# ------------------------------------------------------------------------------------------------ torch
@gpu
def test_tensors_decode_and_encode(ctx, mlib, orc):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no torch.cuda")
    from mp3stego import tensors
    files = file_list(mlib)
    names = [n for n in files if n not in ("refused", "none")]
    ref = [r for n, r in zip(files, decoded_streams(ctx, mlib, orc, files)) if n in names]
    mp3s = [files[n] for n in names]
    batch, lengths, infos = tensors.decode(mp3s, ctx=ctx)
    want, valid = M.batch([r["pcm"] for r in ref], [0] * len(ref), max(len(r["pcm"]) for r in ref), 2, "f32")
    assert batch.dtype == torch.float32 and batch.device == torch.device("cuda", ctx.device) and tuple(batch.shape) == want.shape
    assert batch.cpu().numpy().tobytes() == want.tobytes() and lengths.dtype == torch.int64 and lengths.tolist() == valid
    assert [i["sampling_rate"] for i in infos] == [r["sampling_rate"] for r in ref]
    # out= is reused, with work of torch's stream pending on it
    out = torch.empty((len(mp3s), 1, 5000), dtype=torch.int16, device=batch.device)
    out.fill_(77)
    again, lengths, _ = tensors.decode(mp3s, first_rows=[9] * len(mp3s), out=out, ctx=ctx)
    want, valid = M.batch([r["pcm"] for r in ref], [9] * len(ref), 5000, 1, "i16")
    assert again is out and out.cpu().numpy().tobytes() == want.tobytes() and lengths.tolist() == valid
    with_bad, lengths, infos = tensors.decode(mp3s[:2] + [None], rows=100, dtype=torch.int16, channels=2, ctx=ctx, per_file=True)
    assert isinstance(infos[2], mlib.Mp3sError) and lengths.tolist() == [100, 100, 0] and not with_bad[2].any()
    # the three refusals, in both directions
    wrong = [torch.empty((len(mp3s), 2, 64), dtype=torch.float64, device=batch.device), torch.empty((len(mp3s), 2, 64), dtype=torch.float32),
             torch.empty((len(mp3s), 2, 128), dtype=torch.float32, device=batch.device)[:, :, ::2]]
    for t in wrong:
        with pytest.raises(ValueError):
            tensors.decode(mp3s, out=t, ctx=ctx)
        with pytest.raises(ValueError):
            tensors.encode(t, [64] * len(mp3s), 44100, ctx=ctx)
    # a stereo float batch back into MP3 files: encode_pcm of the model's frames
    stereo = [k for k, r in enumerate(ref) if r["sampling_rate"] == 44100][:2]
    sub = batch[stereo].contiguous()
    n = [int(valid_k) for valid_k in (len(ref[k]["pcm"]) for k in stereo)]
    got = tensors.encode(sub, torch.tensor(n), 44100, bitrate=128, messages=["tensor", None], ctx=ctx)
    for g, k, rows in zip(got, stereo, n):
        want = ctx.encode_pcm(M.frames(sub[stereo.index(k)].cpu().numpy(), rows), 44100, 128,
                              np.array(mlib.message_frame("tensor"), dtype=np.uint8) if k == stereo[0] else None)
        assert bytes(g["data"]) == want["mp3"] and g["hide_offset"] == want["hide_offset"]
