"""ctypes binding of the C-ABI in include/mp3s.h: the calls.  What mirrors the header -- constants, records, the prototype table, lib()
and check() -- is mp3stego/_abi.py and is re-exported here; Context, Pipe, StreamIndex and the host helpers below are what calls it.

This is the only place the Python side touches native code.  There is no CPU fallback: if the
shared library is missing, or no MI355X is visible, the first call that needs the transforms raises.

Lifetimes, the one rule every call here follows:
  - what a native call reads (byte strings, the numpy views of them, pointer and length arrays) is held in locals of the calling
    method until the call returns, and in Pipe._keep[ticket] until the job is collected.  The helpers that build such arguments
    (_file_list, _pair_lists, _message, _message_list, _hide_bits, _hide_bits_list, _encode_args) return what has to stay alive
    explicitly, beside the pointers; the caller binds it to a name, and that name is the keep-alive.
  - a result that looks into library memory (_view_owned, _owned_bytes) holds an _Owner, which frees the mp3s_buf when the last such
    result is gone; a result that is copied (_view, C.string_at) is made inside `with _Owner(owner):`, which frees it at the end.
  - device memory a method allocates for the length of one call comes from Context.device_scope(), which frees it on the way out.
"""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import *  # noqa: F401,F403
from ._abi import _HERE, _lock  # noqa: F401

_EMPTY = C.c_char()          # where an empty file's pointer points (a null pointer is an argument error)
_PCM_DTYPES = {MP3S_PCM_I16: np.int16, MP3S_PCM_F32: np.float32, MP3S_PCM_F64: np.float64}


def __getattr__(name):
    if name == "_lib":       # the loaded library, cached by _abi.lib()
        return _abi._lib
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _addr(p):
    """a device address as ctypes takes it: a c_void_p (Context.alloc), an int (an address with an offset, a tensor's data_ptr()) or None"""
    if p is None:
        return None
    return C.c_void_p(p.value if isinstance(p, C.c_void_p) else int(p))


def select_patterns():
    """the 32 bytes every message array of a selection call starts with (include/mp3s.h mp3s_select_patterns)"""
    out = np.zeros(32, dtype=np.uint8)
    lib().mp3s_select_patterns(out.ctypes.data)
    return out


def select_plan(segs, cap):
    """-> (spans, ent_unit, ent_cursor) for the CHAIN_SEG_DTYPE records `segs` (include/mp3s.h mp3s_select_plan)"""
    segs = np.ascontiguousarray(segs, dtype=CHAIN_SEG_DTYPE)
    spans = np.zeros(len(segs), dtype=SELECT_SPAN_DTYPE)
    n = lib().mp3s_select_plan(segs.ctypes.data, len(segs), spans.ctypes.data, None, None, cap)
    if n < 0:
        check(n)
    unit, cursor = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
    if n:
        check(lib().mp3s_select_plan(segs.ctypes.data, len(segs), spans.ctypes.data, unit.ctypes.data, cursor.ctypes.data, n) - n)
    return spans, unit[:n], cursor[:n]


def device_count():
    """HIP devices this process can open (mp3s_device_count); touches the HIP runtime"""
    n = C.c_int()
    check(lib().mp3s_device_count(C.byref(n)))
    return n.value


# ---- arguments: every helper returns what has to stay alive beside the pointers it hands out
def _file_list(files, none_is_null=False):
    """a list of byte strings as the arrays of a list-of-files call -> (n, what has to stay alive beside them, pointers, lengths).
    An empty file points at _EMPTY: a null pointer is an argument error, whatever numpy calls the address of an empty array.
    none_is_null: a file that is None travels as a null pointer of length 0, which its entry of the answer speaks for"""
    n = len(files)
    bufs = [None if none_is_null and f is None else np.frombuffer(f, dtype=np.uint8) for f in files]
    ptrs = (C.c_void_p * n)(*[None if b is None else b.ctypes.data if len(b) else C.addressof(_EMPTY) for b in bufs])
    lens = (C.c_size_t * n)(*[0 if b is None else len(b) for b in bufs])
    return n, (files, bufs), ptrs, lens


def _pair_lists(mp3s_a, mp3s_b, none_is_null=False):
    """two lists of byte strings as the arrays of a pair-list call -> (n, what has to stay alive beside them, a's pointers and lengths,
    b's).  none_is_null: as for _file_list"""
    n, keep_a, pa, la = _file_list(mp3s_a, none_is_null)
    _, keep_b, pb, lb = _file_list(mp3s_b, none_is_null)
    return n, (keep_a, keep_b), pa, la, pb, lb


def _message(message, empty_is_null=False):
    """one message as (the buffer to keep alive, pointer, length in bytes).  The library tells two spellings apart and both are in use:
    the list, block and chunked calls take None (clear: a null pointer) or a str, "" being a one-byte buffer of length 0;
    empty_is_null (hide_message, recode_to_fd, message_frame): a str only, "" being a null pointer of length 0"""
    if message is None and not empty_is_null:
        return None, None, 0
    m = message.encode("utf-8")
    if empty_is_null and not m:
        return None, None, 0
    mb = np.frombuffer(m or b"\0", dtype=np.uint8)
    return mb, mb.ctypes.data, len(m)


def _message_list(messages):
    """one message (or None) per file as the arrays of a list call -> (the buffers to keep alive, pointers, lengths), each message as
    _message spells it; messages=None (nothing anywhere) -> three None"""
    if messages is None:
        return None, None, None
    n = len(messages)
    bufs, ptrs, lens = zip(*[_message(t) for t in messages]) if n else ((), (), ())
    return bufs, (C.c_void_p * n)(*ptrs), (C.c_size_t * n)(*lens)


def _hide_bits(hide_bits):
    """one 0/1 array (None or empty: nothing is hidden) as (the array to keep alive, pointer, length)"""
    if hide_bits is None or not len(hide_bits):
        return None, None, 0
    hb = np.ascontiguousarray(hide_bits, dtype=np.uint8)
    return hb, hb.ctypes.data, len(hb)


def _hide_bits_list(hide_bits, messages, n, what="file"):
    """hide_bits (one 0/1 array or None per file) or messages (one str or None per file, framed with message_frame) as the arrays of a
    list call -> (the arrays to keep alive, pointers, int32 lengths); three None with neither"""
    if hide_bits is not None and messages is not None:
        raise ValueError("hide_bits or messages, not both")
    if messages is not None:
        hide_bits = [None if m is None else np.array(message_frame(m), dtype=np.uint8) for m in messages]
    if hide_bits is None:
        return None, None, None
    if len(hide_bits) != n:
        raise ValueError(f"one bit string (or None) per {what}")
    hbs, ptrs, lens = zip(*[_hide_bits(h) for h in hide_bits]) if n else ((), (), ())
    return hbs, (C.c_void_p * n)(*ptrs), (C.c_int32 * n)(*lens)


def _encode_args(wavs, bitrate, hide_bits, messages):
    """the argument arrays of mp3s_encode_files / mp3s_pipe_submit_encode (+ everything that has to stay alive beside them)"""
    n = len(wavs)
    rates = [int(bitrate)] * n if np.isscalar(bitrate) else [int(b) for b in bitrate]
    if len(rates) != n:
        raise ValueError("one bitrate per file")
    hbs, hptr, hlen = _hide_bits_list(hide_bits, messages, n)
    _, keep, files, lens = _file_list(wavs)
    return n, files, lens, (C.c_int32 * n)(*rates), hptr, hlen, (keep, hbs)


# ---- results: one builder per shape
class _Owner:
    """keeps an mp3s_buf alive for the numpy arrays that look into it (no copy of large results); as a `with` block, for results that
    are copies: the buffer is freed when the block ends"""

    def __init__(self, handle):
        self.handle = handle

    def free(self):
        if self.handle:
            lib().mp3s_buf_free(self.handle)
            self.handle = None
    __del__ = free

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def _view_owned(ptr, dtype, shape, owner):
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    if n == 0 or not ptr:
        return np.zeros(shape, dtype=dtype)
    buf = (C.c_char * n).from_address(ptr)
    buf._mp3s_owner = owner                    # the array's base is `buf`; `buf` keeps the owner
    return np.frombuffer(buf, dtype=dtype).reshape(shape)


def _view(ptr, dtype, shape):
    return _view_owned(ptr, dtype, shape, None).copy()


def _owned_bytes(ptr, n, own):
    """read-only bytes-like view (compare, hash, write, len, slice) of n bytes of a library buffer that `own` keeps
    alive: a 40 MB file is handed over, not copied"""
    if not n:
        return b""
    raw = (C.c_char * n).from_address(ptr)
    raw._mp3s_owner = own
    return memoryview(raw).cast("B").toreadonly()


def _per_file(out, status, make, n=None, what="file"):
    """the answer of a list-of-files call, one entry per file (per pair: what="pair"): make(out[i]), or the Mp3sError status[i] names"""
    return [Mp3sError(status[i], f"{what} {i}") if status[i] else make(out[i]) for i in range(len(status) if n is None else n)]


def _file_dict(f, own, data="view", bits="view", hide=True):
    """the dict of an mp3s_file.  data: "view" = a read-only view of the library's buffer that holds `own`, "copy" = bytes, "len" = no
    "data" but its length as "len" (the calls that write to a file descriptor); bits: "view" (holds `own`), "copy", or None = no "bits";
    hide=False: a call that hides nothing, "too_long" / "hide_offset" are False / 0 whatever the record holds"""
    n = f.len
    d = {"len" if data == "len" else "data": n if data == "len" else _owned_bytes(f.data, n, own) if data == "view" else C.string_at(f.data, n) if n else b"",
         "kbps": f.kbps, "sampling_rate": f.sampling_rate, "channels": f.channels, "n_frames": f.n_frames,
         "too_long": bool(f.too_long) if hide else False, "hide_offset": f.hide_offset if hide else 0}
    if bits is not None:
        d["bits"] = _view_owned(f.bits, np.uint8, (f.n_bits,), own) if bits == "view" else _view(f.bits, np.uint8, (f.n_bits,))
    return d


def _block_dict(b, own=None):
    """the dict of an mp3s_block; "mp3" is a copy, or with `own` a read-only view of the library's buffer that holds it"""
    f = b.file
    return {"total_frames": b.total_frames, "first_frame": b.first_frame, "n_frames": b.n_frames, "is_last": bool(b.is_last),
            "carry_used": bool(b.carry_used), "carry_out": b.carry_out.to_array(),
            "mp3": _owned_bytes(f.data, f.len, own) if own is not None else C.string_at(f.data, f.len) if f.len else b"",
            "kbps": f.kbps, "sampling_rate": f.sampling_rate, "too_long": bool(f.too_long), "hide_offset": f.hide_offset}


def _decoded_dict(d, out_format, own):
    """the dict of an mp3s_decoded: "pcm" looks into the library's buffer (no 46 MB copy per 10k frames) and holds `own`, "bits" is a copy"""
    return {"n_frames": d.n_frames, "channels": d.nch, "sampling_rate": d.sampling_rate, "bit_rate": d.bit_rate,
            "pcm": _view_owned(d.pcm, _PCM_DTYPES[out_format], (d.n_rows, d.nch), own), "bits": _view(d.bits, np.uint8, (d.n_bits,))}


def _batch_info_dict(x):
    """the dict of an mp3s_pcm_batch_info; an mp3s_pcm_batch_info_at adds what the resampler did"""
    return {"channels" if k == "nch" else k: getattr(x, k) for k, _ in x._fields_ if k != "reserved"}


def _with_hide_fields(out, took, diff, hidden):
    """out[i] = diff[k] + "too_long" and "hide_offset" of hidden[i] for i = took[k] (an exception in diff[k] as it is) -> out"""
    for i, d in zip(took, diff):
        if not isinstance(d, Exception):
            d = dict(d, too_long=hidden[i]["too_long"], hide_offset=hidden[i]["hide_offset"])
        out[i] = d
    return out


def _close_quietly(self):
    """the __del__ of everything here that has a close()"""
    try:
        self.close()
    except Exception:
        pass


class _DeviceScope:
    """device buffers for the length of a `with` block (Context.device_scope): what alloc / to_device make through it is freed when the
    block ends, whatever raised and wherever -- a later allocation that fails included"""

    def __init__(self, ctx):
        self.ctx, self.made = ctx, []

    def alloc(self, nbytes):
        self.made.append(self.ctx.alloc(nbytes))
        return self.made[-1]

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        self.ctx.upload(p, arr)
        return p

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        while self.made:
            self.ctx.free(self.made.pop())
        return False


class Context:
    """One context = one HIP device + one stream (one process per GPU)."""

    def __init__(self, device=None):
        if device is None:
            device = int(os.environ.get("MP3STEGO_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        h = C.c_void_p()
        check(lib().mp3s_ctx_create(int(device), C.byref(h)))
        self.handle = h
        self.device = int(device)

    def close(self):
        if self.handle:
            for p in list(getattr(self, "_pipes", ())):      # a pipe works on its context's stream: it goes first
                p.close()
            lib().mp3s_ctx_destroy(self.handle)
            self.handle = None

    OPTIONS = {"select": 1, "redo": 2, "fast_imdct": 3, "pipe_tail": 4, "chunk_frames": 5, "device_parse": 6, "file_pipeline": 7,
               "scan_threads": 8, "first_chunk_frames": 9, "file_up": 10, "huf_lanes": 11, "numa": 12, "float_fast": 13, "fail_chunk": 14, "fused_decode": 15, "fused_encode": 16, "pipe_dec": 17, "rate_signals": 18, "pipe_signals": 19, "wav_import": 20, "wav_resample": 21, "analysis_shared": 0}

    def set_option(self, name, value):
        """options of the context (include/mp3s.h MP3S_OPT_*); returns the value the option had"""
        old = self.get_option(name)
        check(lib().mp3s_ctx_set_option(self.handle, self.OPTIONS[name], int(value)))
        return old

    def run_stats(self):
        """what became of this context's one-file calls: dict(files, chunks, reruns, resolved, fallbacks) + how the streams of its
        own pipe were chosen: rehearsal_us, rehearsals, lanes, queue_shared (mp3s_ctx_run_stats)"""
        a = (C.c_int64 * 9)()
        check(lib().mp3s_ctx_run_stats(self.handle, a))
        return dict(zip(("files", "chunks", "reruns", "resolved", "fallbacks", "rehearsal_us", "rehearsals", "lanes", "queue_shared"), list(a)))

    def host_share(self):
        """what this rank holds of the host: dict(pinned_pooled_bytes, pinned_pool_cap_bytes, local_world_size, cpus_allowed,
        gpu_node_cpus) (mp3s_ctx_host_share)"""
        return host_share(self.handle)

    def get_option(self, name):
        v = C.c_int64()
        check(lib().mp3s_ctx_get_option(self.handle, self.OPTIONS[name], C.byref(v)))
        return v.value

    __del__ = _close_quietly

    def device_name(self):
        buf = C.create_string_buffer(256)
        check(lib().mp3s_device_name(self.handle, buf, 256))
        return buf.value.decode()

    def device_pci(self):
        """the device's PCI address as sysfs spells it (mp3s_device_pci)"""
        buf = C.create_string_buffer(64)
        check(lib().mp3s_device_pci(self.handle, buf, 64))
        return buf.value.decode()

    def sync(self):
        check(lib().mp3s_sync(self.handle))

    # ---- device memory helpers (benchmarks, resident pipelines)
    def alloc(self, nbytes):
        p = C.c_void_p()
        check(lib().mp3s_dev_alloc(self.handle, int(nbytes), C.byref(p)))
        return p

    def free(self, p):
        check(lib().mp3s_dev_free(self.handle, p))

    def upload(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        check(lib().mp3s_dev_upload(self.handle, dptr, arr.ctypes.data, arr.nbytes))

    def download(self, dptr, dtype, shape):
        out = np.empty(shape, dtype=dtype)
        check(lib().mp3s_dev_download(self.handle, out.ctypes.data, dptr, out.nbytes))
        return out

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        self.upload(p, arr)
        return p

    def device_scope(self):
        """`with ctx.device_scope() as dev:` -- dev.alloc / dev.to_device as above, everything made through dev freed when the block ends"""
        return _DeviceScope(self)

    def parse_frames(self, data: bytes, walked, want_tsel=True):
        """side info + main-data gather of a walked stream on the device: -> dict(side, hdr, blob, tsel, status)"""
        n = walked["n_frames"]
        with self.device_scope() as dev:
            d_img = dev.to_device(np.frombuffer(data, dtype=np.uint8))
            d_refs, d_streams = dev.to_device(walked["refs"]), dev.to_device(walked["stream"])
            d_side, d_hdr, d_blob = dev.alloc(n * 104), dev.alloc(n * 8), dev.alloc(walked["blob_len"] + 16)
            d_tsel = dev.alloc(n * 8) if want_tsel else None
            d_st = dev.to_device(np.zeros(4, dtype=np.int32))
            check(lib().mp3s_parse_frames_dev(self.handle, d_img, 0, d_refs, d_streams, n, 0, d_side, d_hdr, d_blob, d_tsel, d_st))
            return {"side": self.download(d_side, FRAME_SIDE_DTYPE, (n,)), "hdr": self.download(d_hdr, FRAME_HDR_DTYPE, (n,)),
                    "blob": self.download(d_blob, np.uint8, (walked["blob_len"],)),
                    "tsel": self.download(d_tsel, np.uint64, (n,)) if want_tsel else None,
                    "status": int(self.download(d_st, np.int32, (4,))[0])}

    def reveal_bits(self, data: bytes, walked):
        """the stego bits of a walked stream on the device (mp3s_reveal_bits_dev, one stream): -> (packed uint8 array: eight bits
        to a byte, MSB first, the last byte zero-padded; n_bits)"""
        n = walked["n_frames"]
        room = (12 * n + 31) // 32 * 4
        with self.device_scope() as dev:
            d_img = dev.to_device(np.frombuffer(data, dtype=np.uint8))
            d_refs, d_streams = dev.to_device(walked["refs"]), dev.to_device(walked["stream"])
            d_off, d_packed, d_out = dev.to_device(np.zeros(1, dtype=np.uint32)), dev.alloc(room), dev.alloc(8)
            check(lib().mp3s_reveal_bits_dev(self.handle, d_img, 0, d_refs, d_streams, 1, d_off, d_packed, d_out, C.c_void_p(d_out.value + 4)))
            n_bits, status = (int(v) for v in self.download(d_out, np.int32, (2,)))
            if status:
                raise Mp3sError(E_MALFORMED, f"k_reveal refused the stream's frame references (status {status})")
            return self.download(d_packed, np.uint8, (room,))[:(n_bits + 7) // 8].copy(), n_bits

    def wait_for(self, other):
        """work submitted to this context from now on starts after everything submitted to `other` so far"""
        check(lib().mp3s_ctx_wait(self.handle, other.handle))

    def wait_last(self, other):
        """... after what `other`'s order event was last recorded behind (the last wait_for(.., other), or other's last rate loop with the option
        rate_signals): no new record in other's queue"""
        check(lib().mp3s_ctx_wait_last(self.handle, other.handle))

    def timer_start(self):
        check(lib().mp3s_timer_start(self.handle))

    def timer_stop(self):
        ms = C.c_float()
        check(lib().mp3s_timer_stop(self.handle, C.byref(ms)))
        return ms.value

    def synth_mode(self, eps_scale=1.0):
        """guard of the fast int16 synthesis: 1 = proven bound, 0 = always the exact kernel, > 1 = wider (tests);
        returns the number of samples the guard has sent through the exact order since the last call"""
        n = C.c_int64()
        check(lib().mp3s_synth_mode(self.handle, float(eps_scale), C.byref(n)))
        return n.value

    def guard_margin(self, n_samples):
        """probe of the int16 decode's guard (include/mp3s.h mp3s_debug_guard_margin): context manager; inside it every fused int16 decode of
        up to n_samples samples leaves its fast values and guard widths, read with .read() -> (x, eps) float64 arrays"""
        ctx = self

        class _Probe:
            def __enter__(self):
                self.n = int(n_samples)
                self.d_x, self.d_eps = ctx.alloc(self.n * 8), ctx.alloc(self.n * 8)
                check(lib().mp3s_dev_memset(ctx.handle, self.d_x, 0, self.n * 8))
                check(lib().mp3s_dev_memset(ctx.handle, self.d_eps, 0, self.n * 8))
                check(lib().mp3s_debug_guard_margin(ctx.handle, self.d_x, self.d_eps, self.n))
                return self

            def read(self, n=None):
                ctx.sync()
                n = self.n if n is None else int(n)
                return ctx.download(self.d_x, np.float64, (n,)), ctx.download(self.d_eps, np.float64, (n,))

            def __exit__(self, *exc):
                check(lib().mp3s_debug_guard_margin(ctx.handle, None, None, 0))
                ctx.free(self.d_x); ctx.free(self.d_eps)
                return False
        return _Probe()

    def bench_copy(self, nbytes=1 << 30, iters=20):
        """GB/s (read + write) of a plain device copy kernel"""
        g = C.c_double()
        check(lib().mp3s_bench_copy(self.handle, int(nbytes), int(iters), C.byref(g)))
        return g.value

    KERNELS = ("k_dec_imdct", "k_dec_synth", "k_enc_analysis", "k_enc_mdct", "k_rate_loop", "k_dec_huffman",
               "k_enc_pack", "k_chain", "k_wav_resample")

    def profile_enable(self, on=True):
        check(lib().mp3s_profile_enable(self.handle, 1 if on else 0))

    def profile_select(self, kernels=None):
        """time only the named kernels (None = all): every event pair costs stream time"""
        mask = 0xffffffff if kernels is None else sum(1 << self.KERNELS.index(k) for k in kernels)
        check(lib().mp3s_profile_select(self.handle, mask))

    def profile_collect(self):
        """{kernel: (total_ms, launches)} since profile_enable()"""
        nk = len(self.KERNELS)
        ms = np.zeros(nk, dtype=np.float64)
        cnt = np.zeros(nk, dtype=np.int64)
        check(lib().mp3s_profile_collect(self.handle, ms.ctypes.data, cnt.ctypes.data, nk))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(self.KERNELS)}

    # ---- batch entry points on host arrays
    def decode_transform(self, is_, si, hdr, nch, n_halo=0, out_format=MP3S_PCM_F64):
        is_ = np.ascontiguousarray(is_, dtype=np.int16)
        si = np.ascontiguousarray(si, dtype=GRANULE_SI_DTYPE)
        hdr = np.ascontiguousarray(hdr, dtype=FRAME_HDR_DTYPE)
        n = is_.shape[0]
        pcm = np.empty(((n - n_halo) * 1152, nch), dtype=_PCM_DTYPES[out_format])
        check(lib().mp3s_decode_transform(self.handle, is_.ctypes.data, si.ctypes.data, hdr.ctypes.data, n, nch, n_halo,
                                          out_format, pcm.ctypes.data))
        return pcm

    def encode_transform(self, pcm_i16, hdr=None):
        pcm_i16 = np.ascontiguousarray(pcm_i16, dtype=np.int16)
        n = pcm_i16.shape[0] // 1152
        if hdr is None:
            hdr = np.zeros(n, dtype=FRAME_HDR_DTYPE)
            hdr["nch"] = 2
        hdr = np.ascontiguousarray(hdr, dtype=FRAME_HDR_DTYPE)
        mdct = np.empty((n, 2, 2, 576), dtype=np.int32)
        check(lib().mp3s_encode_transform(self.handle, pcm_i16.ctypes.data, hdr.ctypes.data, n, mdct.ctypes.data))
        return mdct

    # ---- whole-stream pipelines
    def decode_stream(self, data: bytes, out_format=MP3S_PCM_I16):
        buf = np.frombuffer(data, dtype=np.uint8)
        owner, d = C.c_void_p(), Decoded()
        check(lib().mp3s_decode_stream(self.handle, buf.ctypes.data, len(data), out_format, C.byref(owner), C.byref(d)))
        return _decoded_dict(d, out_format, _Owner(owner))

    def decode_block(self, data: bytes, first_frame, n_frames, out_format=MP3S_PCM_I16, index=None):
        """frames [first_frame, first_frame + n_frames) of the stream (clipped to its end): one shard of a stream that is
        spread over several GPUs.  "bits", "bit_rate", "sampling_rate" describe the whole stream.  With an `index`
        (StreamIndex) only the block is scanned, and "bits" are those of the block's frames."""
        buf = np.frombuffer(data, dtype=np.uint8)
        owner, d = C.c_void_p(), Decoded()
        check(lib().mp3s_decode_block_indexed(self.handle, buf.ctypes.data, len(data), index.handle if index is not None else None,
                                              int(first_frame), int(n_frames), out_format, C.byref(owner), C.byref(d)))
        return _decoded_dict(d, out_format, _Owner(owner))

    def decode_streams(self, files, out_format=MP3S_PCM_I16, per_file=False):
        """Decode many MP3 files as one device batch (one Huffman + one transform launch per channel count).
        per_file=True: a file that cannot be decoded yields the Mp3sError it alone would raise, the others are unaffected;
        otherwise the first such file fails the call."""
        if len(files) == 0:
            return []
        n, _keep, ptrs, lens = _file_list(files)
        owner, d = C.c_void_p(), (Decoded * n)()
        status = (C.c_int32 * n)()                 # (stays zero without per_file: a failing file fails the call)
        check(lib().mp3s_decode_streams(self.handle, ptrs, lens, n, out_format, C.byref(owner), d, status if per_file else None))
        own = _Owner(owner)
        return _per_file(d, status, lambda x: _decoded_dict(x, out_format, own))

    def encode_pcm(self, pcm_i16, samplerate, bitrate, hide_bits=None):
        pcm_i16 = np.ascontiguousarray(pcm_i16, dtype=np.int16)
        nch = 1 if pcm_i16.ndim == 1 else pcm_i16.shape[1]
        _hb, hptr, nh = _hide_bits(hide_bits)
        owner, e = C.c_void_p(), Encoded()
        check(lib().mp3s_encode_pcm(self.handle, pcm_i16.ctypes.data, pcm_i16.shape[0], nch, samplerate, bitrate,
                                    hptr, nh, C.byref(owner), C.byref(e)))
        with _Owner(owner):
            return {"n_frames": e.n_frames, "too_long": bool(e.too_long), "hide_offset": e.hide_offset,
                    "mp3": _view(e.mp3, np.uint8, (e.mp3_len,)).tobytes(),
                    "gr": _view(e.gr, GR_OUT_DTYPE, (e.n_frames * 4,)),
                    "scfsi": _view(e.scfsi, np.int32, (e.n_frames, 2, 4)), "rate_passes": e.rate_passes}

    def encode_block(self, pcm_i16, lead_frames, first_frame, last_block, samplerate, bitrate, hide_bits=None, carry_in=None):
        """one contiguous block of a longer stream (include/mp3s.h mp3s_encode_block).  pcm_i16 holds lead_frames frames
        in front of the block's own; carry_in / "carry_out" are int64[17] = cursor + 4x4 chain."""
        pcm_i16 = np.ascontiguousarray(pcm_i16, dtype=np.int16)
        if pcm_i16.ndim != 2 or pcm_i16.shape[1] != 2:
            raise Mp3sError(E_UNSUPPORTED, "stereo PCM [rows][2] expected")
        _hb, hptr, nh = _hide_bits(hide_bits)
        cin = Carry.from_array(carry_in) if carry_in is not None else None
        cout, used, owner, e = Carry(), C.c_int32(0), C.c_void_p(), Encoded()
        check(lib().mp3s_encode_block(self.handle, pcm_i16.ctypes.data, pcm_i16.shape[0], int(lead_frames), int(first_frame),
                                      1 if last_block else 0, int(samplerate), int(bitrate), hptr, nh,
                                      C.byref(cin) if cin is not None else None, C.byref(cout), C.byref(used), C.byref(owner), C.byref(e)))
        with _Owner(owner):
            return {"n_frames": e.n_frames, "too_long": bool(e.too_long), "hide_offset": e.hide_offset,
                    "mp3": _view(e.mp3, np.uint8, (e.mp3_len,)).tobytes(), "gr": _view(e.gr, GR_OUT_DTYPE, (e.n_frames * 4,)),
                    "carry_out": cout.to_array(), "carry_used": bool(used.value), "rate_passes": e.rate_passes}

    # ---- whole files as byte strings (include/mp3s.h section vi)
    _owned_bytes = staticmethod(_owned_bytes)

    @staticmethod
    def _file(f, owner):
        return _file_dict(f, _Owner(owner))

    def decode_file(self, mp3: bytes):
        """MP3 bytes -> WAV bytes (+ kbps of the last header and the stego bits).  "data" is a read-only view of the
        library's buffer (bytes-like: compare, hash, write, len, slice), not a 46 MB-per-10k-frames copy."""
        buf = np.frombuffer(mp3, dtype=np.uint8)
        owner, f = C.c_void_p(), File()
        check(lib().mp3s_decode_file(self.handle, buf.ctypes.data, len(mp3), C.byref(owner), C.byref(f)))
        return _file_dict(f, _Owner(owner), bits="copy", hide=False)

    def encode_file(self, wav: bytes, bitrate=320, hide_bits=None):
        """WAV bytes -> MP3 bytes, with the reference's header checks and sample-count rules."""
        buf = np.frombuffer(wav, dtype=np.uint8)
        _hb, hptr, nh = _hide_bits(hide_bits)
        owner, f = C.c_void_p(), File()
        check(lib().mp3s_encode_file(self.handle, buf.ctypes.data, len(wav), int(bitrate), hptr, nh, C.byref(owner), C.byref(f)))
        return self._file(f, owner)

    def decode_file_to_fd(self, mp3: bytes, fd: int):
        """decode_file with the WAV written to the open file `fd` (bytes [0, length), cut to length; include/mp3s.h mp3s_decode_file_fd):
        the PCM of a file that goes through the stages as chunks is written chunk by chunk while the later chunks are on the device.
        Returns decode_file's dict without "data" (+ "len")."""
        buf = np.frombuffer(mp3, dtype=np.uint8)
        owner, f = C.c_void_p(), File()
        check(lib().mp3s_decode_file_fd(self.handle, buf.ctypes.data, len(mp3), int(fd), C.byref(owner), C.byref(f)))
        return _file_dict(f, _Owner(owner), data="len", hide=False)

    def hide_message(self, mp3: bytes, message: str):
        """decode + re-encode with "<count>#<message>" hidden; the PCM stays on the device in between."""
        buf = np.frombuffer(mp3, dtype=np.uint8)
        _mb, mptr, nm = _message(message, empty_is_null=True)
        owner, f = C.c_void_p(), File()
        check(lib().mp3s_hide_message(self.handle, buf.ctypes.data, len(mp3), mptr, nm, C.byref(owner), C.byref(f)))
        return self._file(f, owner)

    def clear_file(self, mp3: bytes):
        buf = np.frombuffer(mp3, dtype=np.uint8)
        owner, f = C.c_void_p(), File()
        check(lib().mp3s_clear_file(self.handle, buf.ctypes.data, len(mp3), C.byref(owner), C.byref(f)))
        return self._file(f, owner)

    def recode_to_fd(self, mp3: bytes, message, fd: int):
        """hide_message (message: str) / clear_file (None) with the result written to the open file `fd` (bytes [0, length), cut to
        length; include/mp3s.h mp3s_hide_message_fd / mp3s_clear_file_fd): a file that goes through the stages as chunks is written
        chunk by chunk while the later chunks are on the device.  Returns the dict of hide_message without "data" (+ "len")."""
        buf = np.frombuffer(mp3, dtype=np.uint8)
        f = File()
        if message is None:
            check(lib().mp3s_clear_file_fd(self.handle, buf.ctypes.data, len(mp3), int(fd), C.byref(f)))
        else:
            _mb, mptr, nm = _message(message, empty_is_null=True)
            check(lib().mp3s_hide_message_fd(self.handle, buf.ctypes.data, len(mp3), mptr, nm, int(fd), C.byref(f)))
        return _file_dict(f, None, data="len", bits=None)

    def reencode_block(self, mp3: bytes, message, rank, world, carry_in=None, index=None):
        """this rank's block of hide_message (message: str) / clear_file (None) on one stream spread over `world` ranks:
        decode + re-encode of the block on the device (include/mp3s.h mp3s_reencode_block).  carry_in: int64[17], None
        for rank 0."""
        buf = np.frombuffer(mp3, dtype=np.uint8)
        _mb, mptr, nm = _message(message)
        cin = Carry.from_array(carry_in) if carry_in is not None else None
        owner, b = C.c_void_p(), Block()
        check(lib().mp3s_reencode_block_indexed(self.handle, buf.ctypes.data, len(mp3), index.handle if index is not None else None,
                                                mptr, nm, int(rank), int(world),
                                                C.byref(cin) if cin is not None else None, C.byref(owner), C.byref(b)))
        with _Owner(owner):
            return _block_dict(b)

    def hide_message_chunked(self, mp3: bytes, message, chunk_frames):
        """hide_message (message: str) / clear_file (None) on a file of any length, chunk_frames frames at a time through the
        device: one index walk, every chunk scanned on its own and run on the real carry of the one in front of it"""
        buf = np.frombuffer(mp3, dtype=np.uint8)
        _mb, mptr, nm = _message(message)
        owner, f = C.c_void_p(), File()
        check(lib().mp3s_hide_message_chunked(self.handle, buf.ctypes.data, len(mp3), mptr, nm, int(chunk_frames), C.byref(owner), C.byref(f)))
        return self._file(f, owner)

    def decode_chunks(self, mp3: bytes, chunk_frames, out_format=MP3S_PCM_I16):
        """generator over the PCM of the stream, chunk_frames frames at a time: one index walk, then every chunk is scanned
        and decoded on its own (the repeated last frame of a stream that ends in a bad header comes with the last chunk)"""
        ix = StreamIndex(mp3)
        first = 0
        while first < max(ix.n_frames, 1):
            blk = self.decode_block(mp3, first, chunk_frames, out_format, index=ix)
            yield blk["pcm"]
            first += chunk_frames
            if ix.n_frames == 0:
                break

    def hide_messages(self, mp3s, messages):
        """hide_message / clear_file (message None) over a list of files as one device batch per (rate, bitrate).
        Returns one entry per file: the dict hide_message returns, or the Mp3sError that file alone would raise."""
        if len(mp3s) != len(messages):
            raise ValueError("one message (or None) per file")
        if len(mp3s) == 0:
            return []
        n, _keep, files, lens = _file_list(mp3s)
        _msgs, mptr, mlen = _message_list(messages)
        out, status, owner = (File * n)(), (C.c_int32 * n)(), C.c_void_p()
        check(lib().mp3s_hide_messages(self.handle, files, lens, n, mptr, mlen, C.byref(owner), out, status))
        with _Owner(owner):
            return _per_file(out, status, lambda f: _file_dict(f, None, data="copy", bits=None))

    def reveal_messages(self, mp3s, _max_streams=None):
        """reveal_message over a list of files as ONE device batch (mp3s_reveal_messages): the files the walk calls regular through
        k_reveal, the others through the host scan.  Returns one entry per file: a dict with the keys of reveal_message(), or the
        Mp3sError that file's scan raises.  _max_streams (test aid): at most that many streams to a launch."""
        if len(mp3s) == 0:
            return []
        n, _keep, files, lens = _file_list(mp3s)
        out, status, owner = (File * n)(), (C.c_int32 * n)(), C.c_void_p()
        if _max_streams is None:
            check(lib().mp3s_reveal_messages(self.handle, files, lens, n, C.byref(owner), out, status))
        else:
            check(lib().mp3s_debug_reveal_messages(self.handle, files, lens, n, int(_max_streams), C.byref(owner), out, status))
        with _Owner(owner):
            return _per_file(out, status, lambda f: _file_dict(f, None, data="copy", bits="copy", hide=False))

    def encode_files(self, wavs, bitrate=320, hide_bits=None, messages=None):
        """encode_file over a list of WAV files as one device batch per (sampling rate, bitrate).  bitrate: one int, or one per
        file; hide_bits: one 0/1 array (or None) per file; messages: one str (or None) per file, framed with message_frame -- a
        convenience over hide_bits.  Returns one entry per file: the dict encode_file returns, or the Mp3sError that file alone
        would raise."""
        if len(wavs) == 0:
            return []
        n, files, lens, kbps, hptr, hlen, _keep = _encode_args(wavs, bitrate, hide_bits, messages)
        out, status, owner = (File * n)(), (C.c_int32 * n)(), C.c_void_p()
        check(lib().mp3s_encode_files(self.handle, files, lens, n, kbps, hptr, hlen, C.byref(owner), out, status))
        own = _Owner(owner)
        return _per_file(out, status, lambda f: _file_dict(f, own))

    @staticmethod
    def _capacity(x, own):
        return {"bits": x.bits, "hide_offset": x.hide_offset, "text_bytes": x.text_bytes, "too_long": bool(x.too_long),
                "n_frames": x.n_frames, "kbps": x.kbps, "sampling_rate": x.sampling_rate, "channels": x.channels,
                "active_units": x.active_units, "fallback": x.fallback,
                "profile": _view_owned(x.profile, np.uint32, (x.n_frames,), own) if x.profile else None}

    def capacities(self, mp3s, messages=None, profile=False):
        """how many message bits each of a list of MP3 files takes (mp3s_capacity_files): the re-encode of hide_messages up to its chain
        check, counted by k_capacity -- no MP3 bytes are made.  messages: one str (or None: the clear capacity, an estimate) per file,
        or None for none anywhere; with a message "hide_offset" / "too_long" are those of hide_messages.  profile: "profile" = the
        per-frame running sum of the bits, uint32 [n_frames].  Returns one entry per file: a dict, or the Mp3sError hide_messages gives."""
        if messages is not None and len(mp3s) != len(messages):
            raise ValueError("one message (or None) per file")
        if len(mp3s) == 0:
            return []
        n, _keep, files, lens = _file_list(mp3s)
        _msgs, mptr, mlen = _message_list(messages)
        out, status, owner = (Capacity * n)(), (C.c_int32 * n)(), C.c_void_p()
        check(lib().mp3s_capacity_files(self.handle, files, lens, n, mptr, mlen, 1 if profile else 0, C.byref(owner), out, status))
        own = _Owner(owner)
        return _per_file(out, status, lambda x: self._capacity(x, own))

    def wav_capacities(self, wavs, bitrate=320, hide_bits=None, messages=None, profile=False):
        """capacities() for a list of WAV files (mp3s_capacity_wavs), arguments as for encode_files: the encode of encode_files up to
        its chain check.  With hide_bits / messages "hide_offset" / "too_long" are those of encode_files."""
        if len(wavs) == 0:
            return []
        n, files, lens, kbps, hptr, hlen, _keep = _encode_args(wavs, bitrate, hide_bits, messages)
        out, status, owner = (Capacity * n)(), (C.c_int32 * n)(), C.c_void_p()
        check(lib().mp3s_capacity_wavs(self.handle, files, lens, n, kbps, hptr, hlen, 1 if profile else 0, C.byref(owner), out, status))
        own = _Owner(owner)
        return _per_file(out, status, lambda x: self._capacity(x, own))

    def capacity_dev(self, gr, segs, profile=True):
        """test aid: k_capacity alone (mp3s_capacity_dev) on the GR_OUT_DTYPE records `gr` and the CHAIN_SEG_DTYPE streams `segs`
        -> (CAPACITY_SEG_DTYPE [len(segs)], uint32 [frames] or None)"""
        gr = np.ascontiguousarray(gr, dtype=GR_OUT_DTYPE)
        segs = np.ascontiguousarray(segs, dtype=CHAIN_SEG_DTYPE)
        n_frames = len(gr) // 4
        with self.device_scope() as dev:
            d_gr, d_segs = dev.to_device(gr if len(gr) else np.zeros(1, dtype=GR_OUT_DTYPE)), dev.to_device(segs)
            d_out = dev.alloc(len(segs) * CAPACITY_SEG_DTYPE.itemsize)
            d_prof = dev.alloc(max(n_frames, 1) * 4) if profile else None
            check(lib().mp3s_capacity_dev(self.handle, d_gr, d_segs, len(segs), d_out, d_prof))
            return (self.download(d_out, CAPACITY_SEG_DTYPE, (len(segs),)),
                    self.download(d_prof, np.uint32, (n_frames,)) if profile else None)

    @staticmethod
    def _table_audit(x, own):
        r = {k: getattr(x, k) for k in TABLE_AUDIT_FIELDS}
        r["payload_bits"] = x.last_forced + 1
        r["verdict"] = "foreign" if x.foreign > 0 else ("carries" if x.forced > 0 else "clean")
        r["profile"] = _view_owned(x.profile, np.uint32, (x.n_frames,), own) if x.profile else None
        return r

    def table_audits(self, mp3s, profile=False):
        """does each of a list of MP3 files carry a payload, and how much (mp3s_table_audit_files): the code book the reference's
        encoder would choose for every region from its values alone is computed again on the device from the Huffman-decoded
        spectrum; a region whose book is that choice transformed by a bit was forced by a message bit.  No transform runs, no PCM
        exists.  mp3s: byte strings (None: a null file, which gets its code).  Returns one entry per file: a dict with the fields of
        mp3s_table_audit (include/mp3s.h, vi-e) plus "payload_bits" = last_forced + 1, a lower bound on the bits hidden (about half the
        bits of a random message force nothing), and "verdict": "foreign" when some region is FOREIGN (the file was not written by
        this encoder and the audit does not speak for it), else "carries" when some region is FORCED, else "clean"; or the Mp3sError
        that file's front end raises.  profile: "profile" = uint32 [n_frames], natural | forced << 4 | foreign << 8 | empty << 12."""
        if len(mp3s) == 0:
            return []
        n, _keep, files, lens = _file_list(mp3s, none_is_null=True)
        out, status, owner = (TableAudit * n)(), (C.c_int32 * n)(), C.c_void_p()
        check(lib().mp3s_table_audit_files(self.handle, files, lens, n, 1 if profile else 0, C.byref(owner), out, status))
        own = _Owner(owner)
        return _per_file(out, status, lambda x: self._table_audit(x, own))

    def table_audit_dev(self, is_, side, segs, nch, units=True, profile=True):
        """test aid: the two audit kernels alone (mp3s_table_audit_dev) on int16 [n_frames][2][2][576] samples, FRAME_SIDE_DTYPE
        [n_frames] side records and TABLE_AUDIT_SEG_DTYPE streams -> (TABLE_AUDIT_DTYPE [len(segs)], TABLE_AUDIT_UNIT_DTYPE
        [n_frames][4] (unit ch * 2 + gr) or None, uint32 [n_frames] or None)"""
        is_ = np.ascontiguousarray(is_, dtype=np.int16)
        side = np.ascontiguousarray(side, dtype=FRAME_SIDE_DTYPE)
        segs = np.ascontiguousarray(segs, dtype=TABLE_AUDIT_SEG_DTYPE)
        n_frames = len(side)
        if is_.size != n_frames * 2304:
            raise ValueError("is_ must hold 2304 samples per side record")
        with self.device_scope() as dev:
            d_is, d_side, d_segs = dev.to_device(is_), dev.to_device(side), dev.to_device(segs)
            d_out = dev.alloc(len(segs) * TABLE_AUDIT_DTYPE.itemsize)
            d_units = dev.alloc(n_frames * 4 * TABLE_AUDIT_UNIT_DTYPE.itemsize) if units else None
            d_prof = dev.alloc(n_frames * 4) if profile else None
            check(lib().mp3s_table_audit_dev(self.handle, d_is, d_side, n_frames, int(nch), d_segs, len(segs), d_units, d_out, d_prof))
            return (self.download(d_out, TABLE_AUDIT_DTYPE, (len(segs),)),
                    self.download(d_units, TABLE_AUDIT_UNIT_DTYPE, (n_frames, 4)) if units else None,
                    self.download(d_prof, np.uint32, (n_frames,)) if profile else None)

    @staticmethod
    def _distortion(x, own):
        return {"err2": x.err2, "sig2": x.sig2, "n_samples": x.n_samples, "n_diff": x.n_diff, "first_diff": x.first_diff,
                "rows_a": x.rows_a, "rows_b": x.rows_b, "max_abs": x.max_abs, "channels": x.channels, "sampling_rate": x.sampling_rate,
                "n_frames": x.n_frames, "snr_db": x.snr_db, "psnr_db": x.psnr_db,
                "profile": _view_owned(x.profile, PCM_FRAME_DIFF_DTYPE, (x.n_frames,), own) if x.profile else None}

    def pcm_distortions(self, mp3s_a, mp3s_b, profile=False):
        """the exact int16 PCM difference of mp3s_a[i] against mp3s_b[i] (mp3s_pcm_distortion_files): both lists are decoded on the
        device, compared there at lag 0 over their common prefix, and a record per pair comes down -- no PCM does.  A cover file and
        its stego file are not sample-aligned (the codec's delay); compare the clear re-encode with the hide re-encode of one input
        (hide_distortions).  profile: "profile" = a PCM_FRAME_DIFF_DTYPE record per compared frame.  Returns one entry per pair: a
        dict (the fields of mp3s_pcm_distortion), or the Mp3sError of the pair."""
        if len(mp3s_a) != len(mp3s_b):
            raise ValueError("one file of b per file of a")
        if len(mp3s_a) == 0:
            return []
        n, _keep, fa, la, fb, lb = _pair_lists(mp3s_a, mp3s_b)
        out, status, owner = (PcmDistortion * n)(), (C.c_int32 * n)(), C.c_void_p()
        check(lib().mp3s_pcm_distortion_files(self.handle, fa, la, fb, lb, n, 1 if profile else 0, C.byref(owner), out, status))
        own = _Owner(owner)
        return _per_file(out, status, lambda x: self._distortion(x, own), what="pair")

    def hide_distortions(self, mp3s, messages, profile=False):
        """what hiding `messages` in `mp3s` changes in the audio: hide_messages without any message (the clear re-encode) and with the
        messages, then pcm_distortions(clear, hidden) over the files both calls took.  Returns one entry per file: the dict of
        pcm_distortions + "too_long" and "hide_offset" of the hide call, or the exception either call gave for the file."""
        if len(mp3s) != len(messages):
            raise ValueError("one message (or None) per file")
        clear = self.hide_messages(mp3s, [None] * len(mp3s))
        hidden = self.hide_messages(mp3s, messages)
        took = [i for i, (c, h) in enumerate(zip(clear, hidden)) if not isinstance(c, Exception) and not isinstance(h, Exception)]
        diff = self.pcm_distortions([clear[i]["data"] for i in took], [hidden[i]["data"] for i in took], profile)
        return _with_hide_fields([c if isinstance(c, Exception) else h for c, h in zip(clear, hidden)], took, diff, hidden)

    def pcm_diff_dev(self, pcm, pairs, nch):
        """test aid: k_pcm_diff_frames + k_pcm_diff_pairs alone (mp3s_pcm_diff_dev) on the int16 buffer `pcm` ([frames][1152][nch]) and
        the PCM_PAIR_DTYPE records `pairs` -> (PCM_FRAME_DIFF_DTYPE [frame records: max(out_first + n_frames)], PCM_PAIR_DIFF_DTYPE [len(pairs)]);
        frame records no pair names come back as 0xFF bytes"""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        pairs = np.ascontiguousarray(pairs, dtype=PCM_PAIR_DTYPE)
        n_rec = int((pairs["out_first"].astype(np.int64) + pairs["n_frames"]).max()) if len(pairs) else 0
        with self.device_scope() as dev:
            d_pcm = dev.to_device(pcm if pcm.size else np.zeros(8, dtype=np.int16))
            d_pairs = dev.to_device(pairs)
            d_frames, d_out = dev.alloc(max(n_rec, 1) * 32), dev.alloc(len(pairs) * 40)
            check(lib().mp3s_dev_memset(self.handle, d_frames, 0xFF, max(n_rec, 1) * 32))
            check(lib().mp3s_pcm_diff_dev(self.handle, d_pcm, int(nch), d_pairs, pairs.ctypes.data, len(pairs), d_frames, d_out))
            return self.download(d_frames, PCM_FRAME_DIFF_DTYPE, (n_rec,)), self.download(d_out, PCM_PAIR_DIFF_DTYPE, (len(pairs),))

    def pcm_alignments(self, mp3s_a, mp3s_b, max_lag=2304, search_rows=4608, lags=None, profile=False):
        """mp3s_a[i] against mp3s_b[i] across a re-encode's delay (mp3s_pcm_alignment_files): both lists are decoded on the device, the
        lag L in [-max_lag, +max_lag] that minimises the squared error of a[i + L] - b[i] over a window of search_rows rows in the middle
        of the pair is found there by exhaustive search (lags = a list: taken as given, nothing is searched), and the pair is compared
        at that lag over its whole overlap.  For a = stego and b = cover a positive lag means the stego audio comes later.  Returns one
        entry per pair: the dict of pcm_distortions at the lag (n_frames = chunks of 1152 rows of the overlap) + "lag", "n_best" (lags
        that reach the minimum; 0: not searched), "err2_best", "err2_at_0", "search_first", "search_rows", "scores"; with profile, "profile" is
        a PCM_FRAME_DIFF_DTYPE record per chunk and "scores" the uint64 [2 max_lag + 1] scores of a searched pair (both None without); or
        the pair's Mp3sError."""
        if len(mp3s_a) != len(mp3s_b) or (lags is not None and len(lags) != len(mp3s_a)):
            raise ValueError("one file of b (and one lag, when given) per file of a")
        if len(mp3s_a) == 0:
            return []
        n, _keep, fa, la, fb, lb = _pair_lists(mp3s_a, mp3s_b, none_is_null=True)
        given = None if lags is None else (C.c_int32 * n)(*[int(x) for x in lags])
        out, status, owner = (PcmAlignment * n)(), (C.c_int32 * n)(), C.c_void_p()
        check(lib().mp3s_pcm_alignment_files(self.handle, fa, la, fb, lb, n, int(max_lag), int(search_rows), given, 1 if profile else 0,
                                             C.byref(owner), out, status))
        own = _Owner(owner)

        def entry(x):
            d = self._distortion(x.at_lag, own)
            g = x.lag
            d.update(lag=g.lag, n_best=g.n_best, err2_best=g.err2_best, err2_at_0=g.err2_at_0, search_first=g.search_first, search_rows=g.search_rows)
            d["scores"] = _view_owned(x.scores, np.uint64, (2 * int(max_lag) + 1,), own) if x.scores else None
            return d
        return _per_file(out, status, entry, what="pair")

    def stego_distortions(self, mp3s, messages, max_lag=2304, search_rows=4608, profile=False):
        """how far the file handed on is from the file one started with: hide_messages, then pcm_alignments(stego, cover) over the files
        the hide call took.  Returns one entry per file: the dict of pcm_alignments + "too_long" and "hide_offset" of the hide call, or
        the exception either call gave for the file."""
        if len(mp3s) != len(messages):
            raise ValueError("one message (or None) per file")
        hidden = self.hide_messages(mp3s, messages)
        took = [i for i, h in enumerate(hidden) if not isinstance(h, Exception)]
        diff = self.pcm_alignments([hidden[i]["data"] for i in took], [mp3s[i] for i in took], max_lag, search_rows, None, profile)
        return _with_hide_fields(list(hidden), took, diff, hidden)

    def pcm_align_dev(self, pcm, runs, nch, max_lag, search_rows, lags=None):
        """test aid: the three passes of k_pcmalign.hpp + k_pcm_diff_pairs alone (mp3s_pcm_align_dev) on the int16 buffer `pcm`
        ([rows][nch]) and the PCM_RUN_PAIR_DTYPE records `runs` -> (scores uint64 [len(runs)][2 max_lag + 1] or None with given lags,
        PCM_LAG_DTYPE [len(runs)], PCM_FRAME_DIFF_DTYPE [chunk records: max(out_first + bound)], PCM_PAIR_DIFF_DTYPE [len(runs)]);
        what no pass writes (scores of a pair that is not searched, chunk records past an overlap) comes back as 0xFF bytes"""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16).reshape(-1)
        runs = np.ascontiguousarray(runs, dtype=PCM_RUN_PAIR_DTYPE)
        n, n_lags = len(runs), 2 * int(max_lag) + 1
        bound = (np.minimum(runs["a_rows"], runs["b_rows"]).astype(np.int64) + 1151) // 1152
        n_rec = int((runs["out_first"].astype(np.int64) + bound).max()) if n else 0
        given = None if lags is None else np.ascontiguousarray(lags, dtype=np.int32)
        padded = np.zeros((pcm.size + 15) // 8 * 8 + 8, dtype=np.int16)   # (a whole dword behind the last row)
        padded[:pcm.size] = pcm
        with self.device_scope() as dev:
            d_pcm, d_runs = dev.to_device(padded), dev.to_device(runs)
            d_scores, d_lags = (dev.alloc(n * n_lags * 8) if given is None else None), dev.alloc(n * 40)
            d_frames, d_out = dev.alloc(max(n_rec, 1) * 32), dev.alloc(n * 40)
            check(lib().mp3s_dev_memset(self.handle, d_frames, 0xFF, max(n_rec, 1) * 32))
            if d_scores is not None:
                check(lib().mp3s_dev_memset(self.handle, d_scores, 0xFF, n * n_lags * 8))
            check(lib().mp3s_pcm_align_dev(self.handle, d_pcm, int(nch), d_runs, runs.ctypes.data, n, int(max_lag), int(search_rows),
                                           None if given is None else given.ctypes.data, d_scores, d_lags, d_frames, d_out))
            return (None if d_scores is None else self.download(d_scores, np.uint64, (n, n_lags)), self.download(d_lags, PCM_LAG_DTYPE, (n,)),
                    self.download(d_frames, PCM_FRAME_DIFF_DTYPE, (n_rec,)), self.download(d_out, PCM_PAIR_DIFF_DTYPE, (n,)))

    # ---- PCM batches in the caller's device memory (include/mp3s.h section vi-f)
    def pcm_batch_dev(self, d_pcm, nch, d_items, items, channels, fmt, rows, d_out):
        """test aid: k_pcm_batch alone (mp3s_pcm_batch_dev), asynchronous on the context's stream.  d_pcm, d_items and d_out are device
        addresses (Context.alloc / to_device, or an int: an address with an offset), `items` the PCM_BATCH_ITEM_DTYPE records d_items
        holds; interleaved int16 rows of nch samples -> planar [slots][channels][rows] of fmt ("i16" / "f32")"""
        items = np.ascontiguousarray(items, dtype=PCM_BATCH_ITEM_DTYPE)
        check(lib().mp3s_pcm_batch_dev(self.handle, _addr(d_pcm), int(nch), _addr(d_items), items.ctypes.data, len(items), int(channels),
                                       BATCH_FORMATS[fmt], int(rows), _addr(d_out)))

    def pcm_unbatch_dev(self, d_in, channels, fmt, rows, d_items, items, d_pcm):
        """test aid: k_pcm_unbatch alone (mp3s_pcm_unbatch_dev), asynchronous on the context's stream: planar [slots][channels][rows] at
        d_in -> int16 frames [frames][1152][2] at d_pcm, by the PCM_UNBATCH_ITEM_DTYPE records `items` (d_items: the same on the device)"""
        items = np.ascontiguousarray(items, dtype=PCM_UNBATCH_ITEM_DTYPE)
        check(lib().mp3s_pcm_unbatch_dev(self.handle, _addr(d_in), int(channels), BATCH_FORMATS[fmt], int(rows), _addr(d_items),
                                         items.ctypes.data, len(items), _addr(d_pcm)))

    def pcm_batch_resample_dev(self, d_pcm, nch, items, channels, fmt, rows, d_out):
        """test aid: k_pcm_batch_resample alone (mp3s_pcm_batch_resample_dev), asynchronous on the context's stream: pcm_batch_dev with
        the resampler in front.  `items`: PCM_RESAMPLE_ITEM_DTYPE records on the host (n_rows in input rows, first_row in output rows,
        every item with its own ratio L / M in lowest terms; 1 / 1 is a copy), all of them in ONE launch"""
        items = np.ascontiguousarray(items, dtype=PCM_RESAMPLE_ITEM_DTYPE)
        check(lib().mp3s_pcm_batch_resample_dev(self.handle, _addr(d_pcm), int(nch), items.ctypes.data, len(items), int(channels),
                                                BATCH_FORMATS[fmt], int(rows), _addr(d_out)))

    def decode_batch(self, mp3s, d_out, out_bytes, rows, first_rows=None, channels=2, fmt="f32", per_file=False, samplerate=None):
        """Decode a list of MP3 files into the caller's device memory as ONE planar batch [len(mp3s)][channels][rows] of fmt ("f32":
        int16 / 32768, or "i16") at the device address d_out (mp3s_pcm_batch_decode_files): file i's rows from first_rows[i] (0) on
        into slot i, zeros behind its last row; no PCM comes down.  Returns one dict per file: n_frames, channels, sampling_rate,
        bit_rate, n_rows, first_row, valid_rows (the rows of the slot that are samples).  per_file=True: a file that cannot be
        decoded (None included) yields the Mp3sError it alone would raise and a zeroed slot, the others are unaffected; otherwise
        the first such file fails the call.  d_out=None: the sizing call -- only the front end runs, valid_rows is 0.
        samplerate (None: nothing is resampled, the call and the dicts above): every slot at that sampling rate, each file resampled
        by its own ratio on the device (mp3s_pcm_batch_decode_files_at); first_rows, n_rows and valid_rows then count rows at
        `samplerate`, sampling_rate stays the file's own and the dicts gain in_rows (the rows the file decodes to), out_rate, L and M
        (out_rate / sampling_rate in lowest terms).  A file whose rate the resampler refuses for `samplerate` fails like any other."""
        n = len(mp3s)
        if n == 0:
            return []
        _, _keep, ptrs, lens = _file_list(mp3s, none_is_null=True)
        first = None
        if first_rows is not None:
            if len(first_rows) != n:
                raise ValueError("one first row per file")
            first = (C.c_int64 * n)(*[int(x) for x in first_rows])
        status = (C.c_int32 * n)()
        if samplerate is not None:
            info = (PcmBatchInfoAt * n)()
            check(lib().mp3s_pcm_batch_decode_files_at(self.handle, ptrs, lens, n, int(samplerate), first, int(rows), int(channels), BATCH_FORMATS[fmt],
                                                       _addr(d_out), int(out_bytes), info, status if per_file else None))
        else:
            info = (PcmBatchInfo * n)()
            check(lib().mp3s_pcm_batch_decode_files(self.handle, ptrs, lens, n, first, int(rows), int(channels), BATCH_FORMATS[fmt], _addr(d_out),
                                                    int(out_bytes), info, status if per_file else None))
        return _per_file(info, status, _batch_info_dict)

    def batch_rows(self, mp3s, per_file=False, samplerate=None):
        """the sizing call of decode_batch: the dicts it returns ("n_rows" = the rows file i decodes to, at `samplerate` when one is
        given), from the host front end alone"""
        return self.decode_batch(mp3s, None, 0, 0, per_file=per_file, samplerate=samplerate)

    def encode_batch(self, d_in, n_items, channels, fmt, rows, lengths, samplerate, bitrate=320, hide_bits=None, messages=None, per_file=False,
                     resample=0):
        """Encode the items of a planar batch [n_items][channels][rows] of fmt at the device address d_in as ONE device batch
        (mp3s_pcm_batch_encode): item i is its first lengths[i] rows (1 .. rows), the last frame zero-filled, mono into both channels,
        float32 rounded to int16 half-even.  hide_bits / messages as for encode_files.  Whatever wrote d_in must have finished.
        Returns the dicts encode_files returns; per_file=True: an item that fails (a length outside 1 .. rows) yields its Mp3sError,
        otherwise the first such item fails the call.
        resample (0: the batch must be at 32 000 / 44 100 / 48 000 Hz, today's call): the batch is at ANY rate `samplerate` and is
        resampled on the device to the rate the "wav_resample" option's value would pick for it -- 1: the auto rule (a supported
        rate stays, 16 000 -> 32 000, 22 050 -> 44 100 ...), or 32000 / 44100 / 48000 forced (mp3s_pcm_batch_encode_at); the dicts'
        sampling_rate is that target and the bitrate is checked against it."""
        n = int(n_items)
        if len(lengths) != n:
            raise ValueError("one length per item")
        _hbs, hptr, hlen = _hide_bits_list(hide_bits, messages, n, what="item")
        nr = (C.c_int64 * max(n, 1))(*[int(x) for x in lengths])
        out, status, owner = (File * max(n, 1))(), (C.c_int32 * max(n, 1))(), C.c_void_p()
        if resample:
            check(lib().mp3s_pcm_batch_encode_at(self.handle, _addr(d_in), n, int(channels), BATCH_FORMATS[fmt], int(rows), nr, int(samplerate),
                                                 int(resample), int(bitrate), hptr, hlen, C.byref(owner), out, status if per_file else None))
        else:
            check(lib().mp3s_pcm_batch_encode(self.handle, _addr(d_in), n, int(channels), BATCH_FORMATS[fmt], int(rows), nr, int(samplerate),
                                              int(bitrate), hptr, hlen, C.byref(owner), out, status if per_file else None))
        own = _Owner(owner)
        return _per_file(out, status, lambda f: _file_dict(f, own), n=n)

    # ---- QMDCT on the device (include/mp3s.h section vi-g)
    @staticmethod
    def _qmdct_features(x):
        """the dict of an mp3s_qmdct_features (a ctypes record or a numpy one): the arrays are copies, channels 0 .. channels - 1"""
        r = np.frombuffer(bytes(x), dtype=QMDCT_FEATURES_DTYPE)[0] if isinstance(x, C.Structure) else x
        nch = int(r["channels"])
        ch = r["ch"][:nch]
        return {"hist": ch["hist"].copy(), "intra": ch["intra"].copy(), "inter": ch["inter"].copy(), "max_abs": ch["max_abs"].copy(),
                "bandwidth": ch["bandwidth"].copy(), "n_frames": int(r["n_frames"]), "n_granules": 2 * int(r["n_frames"]), "channels": nch,
                "sampling_rate": int(r["sampling_rate"]), "kbps": int(r["kbps"]), "n_lines": int(r["n_lines"])}

    def qmdct_features(self, mp3s, lines=576):
        """Markov and histogram features of the quantised MDCT coefficients of a list of MP3 files (mp3s_qmdct_features_files), the
        input of general MP3 steganalysis, computed on the device from the Huffman-decoded spectrum; no transform runs.  With
        a = |q| over the granule rows of a channel and the lines k < lines: "hist" int64 [channels, 16] counts min(a, 15), "intra" /
        "inter" [channels, 9, 9] count the pairs of consecutive differences of a along a row / down the rows, clipped to +-QMDCT_T
        (include/mp3s.h, vi-g, has the exact definitions), "max_abs" and "bandwidth" [channels]; beside them n_frames, n_granules,
        channels, sampling_rate, kbps, n_lines.  Counts, not probabilities.  mp3s: byte strings (None: a null file, which gets its
        code).  Returns one entry per file: that dict, or the Mp3sError of the file."""
        if len(mp3s) == 0:
            return []
        n, _keep, files, lens = _file_list(mp3s, none_is_null=True)
        out, status = (QmdctFeatures * n)(), (C.c_int32 * n)()
        check(lib().mp3s_qmdct_features_files(self.handle, files, lens, n, int(lines), out, status))
        return _per_file(out, status, self._qmdct_features)

    def qmdct_features_dev(self, is_, segs, nch, lines=576):
        """test aid: k_qmdct_features alone (mp3s_qmdct_features_dev) on int16 [n_frames][2][2][576] samples and TABLE_AUDIT_SEG_DTYPE
        streams -> QMDCT_FEATURES_DTYPE [len(segs)]; the records are filled with 0xFF bytes before the call"""
        is_ = np.ascontiguousarray(is_, dtype=np.int16)
        segs = np.ascontiguousarray(segs, dtype=TABLE_AUDIT_SEG_DTYPE)
        n_frames = is_.size // 2304
        if is_.size != n_frames * 2304:
            raise ValueError("is_ must hold 2304 samples per frame")
        with self.device_scope() as dev:
            d_is, d_segs = dev.to_device(is_ if is_.size else np.zeros(8, dtype=np.int16)), dev.to_device(segs)
            d_out = dev.alloc(max(len(segs), 1) * QMDCT_FEATURES_DTYPE.itemsize)
            check(lib().mp3s_dev_memset(self.handle, d_out, 0xFF, max(len(segs), 1) * QMDCT_FEATURES_DTYPE.itemsize))
            check(lib().mp3s_qmdct_features_dev(self.handle, d_is, n_frames, int(nch), d_segs, segs.ctypes.data, len(segs), int(lines), d_out))
            return self.download(d_out, QMDCT_FEATURES_DTYPE, (len(segs),))

    def qmdct_batch_dev(self, is_, items, nch, channels, granules, guard_rows=2):
        """test aid: k_qmdct_batch alone (mp3s_qmdct_batch_dev) on int16 [n_frames][2][2][576] samples and QMDCT_BATCH_ITEM_DTYPE
        items -> (batch int16 [slots][channels][granules][576], slots = 1 + the largest slot; guard rows in front of and behind it as
        they came back).  Batch and guards are filled with 0x5A bytes before the call."""
        is_ = np.ascontiguousarray(is_, dtype=np.int16)
        items = np.ascontiguousarray(items, dtype=QMDCT_BATCH_ITEM_DTYPE)
        slots = int(items["slot"].max()) + 1 if len(items) else 1
        body, guard = slots * int(channels) * int(granules) * 1152, int(guard_rows) * 1152
        with self.device_scope() as dev:
            d_is, d_items = dev.to_device(is_ if is_.size else np.zeros(8, dtype=np.int16)), dev.to_device(items)
            d_all = dev.alloc(body + 2 * guard)
            check(lib().mp3s_dev_memset(self.handle, d_all, 0x5A, body + 2 * guard))
            check(lib().mp3s_qmdct_batch_dev(self.handle, d_is, int(nch), d_items, items.ctypes.data, len(items), int(channels), int(granules),
                                             _addr(d_all.value + guard)))
            got = self.download(d_all, np.int16, ((body + 2 * guard) // 2,))
        g = guard // 2
        return got[g:g + body // 2].reshape(slots, int(channels), int(granules), 576), (got[:g], got[g + body // 2:])

    def qmdct_batch(self, mp3s, d_out, out_bytes, granules, first_granules=None, channels=2, per_file=False):
        """The quantised MDCT coefficients of a list of MP3 files in the caller's device memory as ONE batch int16 [len(mp3s)][channels]
        [granules][576] at the device address d_out (mp3s_qmdct_batch_decode_files; 16-byte aligned): file i's granule rows from
        first_granules[i] (0) on into slot i, zeros behind its last row and in plane 1 of a mono file; nothing comes down.  Returns one
        dict per file: n_frames, channels, sampling_rate, bit_rate, n_granules, first_granule, valid_granules.  per_file=True: a file
        that fails (None, damage, a stereo file with channels=1) yields its Mp3sError and a zeroed slot, the others are unaffected;
        otherwise the first such file fails the call.  d_out=None: the sizing call -- only the front end runs."""
        n = len(mp3s)
        if n == 0:
            return []
        _, _keep, ptrs, lens = _file_list(mp3s, none_is_null=True)
        first = None
        if first_granules is not None:
            if len(first_granules) != n:
                raise ValueError("one first granule per file")
            first = (C.c_int64 * n)(*[int(x) for x in first_granules])
        info, status = (QmdctBatchInfo * n)(), (C.c_int32 * n)()
        check(lib().mp3s_qmdct_batch_decode_files(self.handle, ptrs, lens, n, first, int(granules), int(channels), _addr(d_out), int(out_bytes),
                                                  info, status if per_file else None))
        return _per_file(info, status, _batch_info_dict)

    def debug_wav_gather(self, wavs):
        """test aid: the PCM buffer k_wav_gather makes of these WAV files, int16 [frames of all files][1152][2]"""
        n, files, lens, _, _, _, _keep = _encode_args(wavs, 128, None, None)
        if self.get_option("wav_resample"):          # the frames at the target rate
            cap = sum(wav_resample_info(w, 128, self.get_option("wav_resample"))["n_frames"] for w in wavs)
        elif self.get_option("wav_import"):          # a frame of mono 8-bit samples is 1 152 bytes of its file
            cap = sum(wav_import_info(w, 128)["n_frames"] for w in wavs)
        else:
            cap = sum(len(w) for w in wavs) // 4608 + n
        pcm, got = np.zeros((cap, 1152, 2), dtype=np.int16), C.c_int64()
        check(lib().mp3s_debug_wav_gather(self.handle, files, lens, n, pcm.ctypes.data, cap, C.byref(got)))
        return pcm[:got.value]


class Pipe:
    """Asynchronous host-fed pipeline (include/mp3s.h section vii): `depth` jobs in flight, host scan || upload || kernels ||
    download.  A job is the argument list of Context.hide_messages; results come back in submission order and are byte
    for byte what hide_messages returns.  The context belongs to the pipe until close()."""

    def __init__(self, ctx, depth=4, max_job_bytes=8 << 20, scan_threads=3, max_files=1024):
        h = C.c_void_p()
        check(lib().mp3s_pipe_create(ctx.handle, int(depth), int(max_job_bytes), int(scan_threads), C.byref(h)))
        self.handle, self.ctx, self.depth = h, ctx, int(depth)
        if not hasattr(ctx, "_pipes"):
            ctx._pipes = []
        ctx._pipes.append(self)                 # Context.close() closes its pipes first
        self._keep = {}                         # ticket -> the buffers the job borrows
        self._out, self._status, self._cap = (File * max_files)(), (C.c_int32 * max_files)(), max_files

    def _submitted(self, rc, ticket, keep):
        """the end of every submit: None when every slot is taken, else the ticket, with `keep` held until the job is collected"""
        if rc == E_BUSY:
            return None
        check(rc)
        self._keep[ticket.value] = keep
        return ticket.value

    def submit(self, mp3s, messages):
        """-> ticket, or None when `depth` jobs are in flight (collect one first).  messages: one str (or None = clear)
        per file, or None = clear all."""
        n = len(mp3s)
        if messages is not None and n != len(messages):
            raise ValueError("one message (or None) per file")
        if n > self._cap:
            raise ValueError(f"{n} files in one job, the pipe was made for {self._cap} (max_files)")
        _, keep, files, lens = _file_list(mp3s)
        msgs, mptr, mlen = _message_list(messages)
        t = C.c_int64()
        rc = lib().mp3s_pipe_submit(self.handle, files, lens, n, mptr, mlen, C.byref(t))
        return self._submitted(rc, t, (keep, msgs, files, lens, mptr, mlen))

    def submit_decode(self, mp3s):
        """a decode job (MP3 -> WAV bytes + stego bits per file) -> ticket, or None when every slot is taken"""
        n = len(mp3s)
        if n > self._cap:
            raise ValueError(f"{n} files in one job, the pipe was made for {self._cap} (max_files)")
        _, keep, files, lens = _file_list(mp3s)
        t = C.c_int64()
        rc = lib().mp3s_pipe_submit_decode(self.handle, files, lens, n, C.byref(t))
        return self._submitted(rc, t, (keep, files, lens))

    def submit_encode(self, wavs, bitrate=320, hide_bits=None, messages=None):
        """an encode job (WAV -> MP3 per file; the arguments of Context.encode_files) -> ticket, or None when every slot is taken"""
        if len(wavs) > self._cap:
            raise ValueError(f"{len(wavs)} files in one job, the pipe was made for {self._cap} (max_files)")
        n, files, lens, kbps, hptr, hlen, keep = _encode_args(wavs, bitrate, hide_bits, messages)
        t = C.c_int64()
        rc = lib().mp3s_pipe_submit_encode(self.handle, files, lens, n, kbps, hptr, hlen, C.byref(t))
        return self._submitted(rc, t, (keep, files, lens, hptr))

    def submit_block(self, mp3, message, rank, world, carry_in=None):
        """a block job: rank `rank` of `world`'s share of hide_message (message: str) / clear_file (None) on one stream (the
        arguments of Context.reencode_block) -> ticket, or None when every slot is taken.  collect() hands out the dict
        Context.reencode_block returns."""
        buf = np.frombuffer(mp3, dtype=np.uint8)
        mb, mptr, nm = _message(message)
        cin = Carry.from_array(carry_in) if carry_in is not None else None
        t = C.c_int64()
        rc = lib().mp3s_pipe_submit_block(self.handle, buf.ctypes.data, len(mp3), mptr, nm,
                                          int(rank), int(world), C.byref(cin) if cin is not None else None, C.byref(t))
        return self._submitted(rc, t, (mp3, buf, mb))

    def collect(self):
        """-> (ticket, [per file: the dict Context.hide_message returns, or the Mp3sError that file alone would raise]);
        None when nothing is in flight.  "data" is a read-only view of the library's page-locked result block.
        For a block job: (ticket, the dict Context.reencode_block returns, "mp3" being such a view)."""
        kind = lib().mp3s_pipe_next_is_block(self.handle)
        if kind == E_BUSY:
            return None
        if kind == 1:
            t, owner, b = C.c_int64(), C.c_void_p(), Block()
            rc = lib().mp3s_pipe_collect_block(self.handle, C.byref(t), C.byref(owner), C.byref(b))
            self._keep.pop(t.value, None)
            check(rc)
            return t.value, _block_dict(b, _Owner(owner))
        t, owner, nf = C.c_int64(), C.c_void_p(), C.c_int32()
        rc = lib().mp3s_pipe_collect(self.handle, C.byref(t), C.byref(owner), self._out, self._status, self._cap, C.byref(nf))
        if rc == E_BUSY:
            return None
        if rc == E_ARG:                         # (the job stays in flight: nothing of it may be released)
            check(rc)
        self._keep.pop(t.value, None)
        check(rc)
        own = _Owner(owner)
        return t.value, _per_file(self._out, self._status, lambda f: _file_dict(f, own, bits="copy"), nf.value)

    def stats(self):
        s = PipeStats()
        check(lib().mp3s_pipe_get_stats(self.handle, C.byref(s)))
        return {k: getattr(s, k) for k, _ in PipeStats._fields_}

    def close(self):
        if self.handle:
            if self.ctx.handle:                 # (a context that is gone took its streams with it)
                lib().mp3s_pipe_destroy(self.handle)
            self.handle = None
            self._keep.clear()
            if self in getattr(self.ctx, "_pipes", ()):
                self.ctx._pipes.remove(self)

    __del__ = _close_quietly


class StreamIndex:
    """resume points of a stream (mp3s_index_stream): blocks of it are then scanned on their own"""

    def __init__(self, data: bytes):
        self._data = data
        buf = np.frombuffer(data, dtype=np.uint8)
        h, info = C.c_void_p(), IndexInfo()
        check(lib().mp3s_index_stream(buf.ctypes.data, len(data), C.byref(h), C.byref(info)))
        self.handle = h
        self.n_frames, self.channels, self.sampling_rate, self.bit_rate = info.n_frames, info.nch, info.sampling_rate, info.bit_rate
        self.dup_last_frame, self.gpu_ok = info.dup_last_frame, bool(info.gpu_ok)

    def scan_range(self, first_frame, n_frames):
        """scan_stream for these frames only"""
        buf = np.frombuffer(self._data, dtype=np.uint8)
        owner, p = C.c_void_p(), Scanned()
        check(lib().mp3s_scan_range(buf.ctypes.data, len(self._data), self.handle, int(first_frame), int(n_frames), C.byref(owner), C.byref(p)))
        with _Owner(owner):
            return _scanned_dict(p)

    def close(self):
        if self.handle:
            lib().mp3s_index_free(self.handle)
            self.handle = None

    __del__ = _close_quietly


def reveal_message(mp3: bytes):
    """MP3 bytes -> the hidden text as the reference writes it to the .txt (host scan only, no GPU)."""
    buf = np.frombuffer(mp3, dtype=np.uint8)
    owner, f = C.c_void_p(), File()
    check(lib().mp3s_reveal_message(buf.ctypes.data, len(mp3), C.byref(owner), C.byref(f)))
    r = Context._file(f, owner)
    r["data"] = bytes(r["data"])               # a message, not a file: plain bytes
    return r


def capacity_text_bytes(bits):
    """the longest ASCII message, in bytes, whose frame "<n>#..." takes at most bits + 1 message bits (mp3s_capacity_text_bytes)"""
    return int(lib().mp3s_capacity_text_bytes(int(bits)))


def wav_parse(data: bytes, bitrate=320):
    """WAV header with the reference's checks (raises Mp3sError; code E_EXIT carries the reference's sys.exit text)."""
    buf = np.frombuffer(data, dtype=np.uint8)
    w = WavInfo()
    check(lib().mp3s_wav_parse(buf.ctypes.data if len(data) else None, len(data), int(bitrate), C.byref(w)))
    return {k: getattr(w, k) for k, _ in WavInfo._fields_}


def wav_import_info(data: bytes, bitrate=320):
    """WAV header by the rules of the "wav_import" option (include/mp3s.h mp3s_wav_import_info): chunk walk over the whole file, mono /
    stereo, 8/16/24/32-bit PCM, float32, extensible.  -> dict(format, channels, samplerate, bits_per_sample, block_align, bitrate,
    data_offset, n_samples, n_frames); raises Mp3sError (E_EXIT carries the reference's text where it has one).  No GPU."""
    buf = np.frombuffer(data, dtype=np.uint8)
    w = WavImport()
    check(lib().mp3s_wav_import_info(buf.ctypes.data if len(data) else None, len(data), int(bitrate), C.byref(w)))
    return {k: getattr(w, k) for k, _ in WavImport._fields_}


def wav_resample_info(data: bytes, bitrate=320, mode=1):
    """what a WAV file of any sampling rate is to the encode calls under the "wav_resample" option (include/mp3s.h
    mp3s_wav_resample_info; mode = the option's value 1 / 32000 / 44100 / 48000) -> dict(in=<the dict of wav_import_info at the file's own
    rate>, out_rate, L, M, taps, half, n_out, n_frames); raises Mp3sError like wav_import_info.  No GPU."""
    buf = np.frombuffer(data, dtype=np.uint8)
    w = WavResample()
    check(lib().mp3s_wav_resample_info(buf.ctypes.data if len(data) else None, len(data), int(bitrate), int(mode), C.byref(w)))
    out = {k: getattr(w, k) for k, _ in WavResample._fields_ if k != "in_"}
    out["in"] = {k: getattr(w.in_, k) for k, _ in WavImport._fields_}
    return out


def pcm_resample_plan(in_rate, out_rate):
    """the ratio the PCM batch calls resample in_rate -> out_rate with (include/mp3s.h mp3s_pcm_resample_plan) -> dict(L, M, taps, half):
    out_rate / in_rate = L / M in lowest terms, taps = 2 * half per phase; L = M = 1: not resampled.  Raises Mp3sError (E_UNSUPPORTED)
    for a ratio the resampler refuses.  The table is wav_resample_taps(L, M).  No GPU."""
    r = PcmResampleRatio()
    check(lib().mp3s_pcm_resample_plan(int(in_rate), int(out_rate), C.byref(r)))
    return {k: getattr(r, k) for k, _ in PcmResampleRatio._fields_}


def wav_resample_taps(L, M):
    """the integer tap table the device uses for the ratio L / M: int32 [L][T] (include/mp3s.h mp3s_wav_resample_taps).  No GPU."""
    taps = np.zeros(max(1, int(L)) * 256, dtype=np.int32)
    t = C.c_int32()
    check(lib().mp3s_wav_resample_taps(int(L), int(M), taps.ctypes.data, taps.size, C.byref(t)))
    return taps[:int(L) * t.value].reshape(int(L), t.value).copy()


def wav_resample_default():
    """the default of the "wav_resample" option for a context created now (MP3S_WAV_RESAMPLE, as mp3s_ctx_create reads it)"""
    try:
        v = int(os.environ.get("MP3S_WAV_RESAMPLE", "") or 0)
    except ValueError:
        return 0
    return v if v in (1, 32000, 44100, 48000) else 0


def wav_import_default():
    """the default of the "wav_import" option for a context created now (MP3S_WAV_IMPORT, as mp3s_ctx_create reads it)"""
    v = os.environ.get("MP3S_WAV_IMPORT", "")
    try:
        return bool(v) and int(v) != 0
    except ValueError:
        return False


def wav_header(n_rows, nch, rate):
    out = (C.c_uint8 * 44)()
    check(lib().mp3s_wav_header(int(n_rows), int(nch), int(rate), out))
    return bytes(out)


def message_frame(message: str):
    """'<character count>#<message>' as UTF-8 bits, MSB first (uint8 0/1)."""
    _mb, mptr, nm = _message(message, empty_is_null=True)
    owner, p, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    check(lib().mp3s_message_frame(mptr, nm, C.byref(owner), C.byref(p), C.byref(n)))
    with _Owner(owner):
        return _view(p.value, np.uint8, (n.value,))


def message_reveal(bits):
    """The reference's reveal parse of a stego bit string -> the bytes it writes to the .txt."""
    b = np.ascontiguousarray(bits, dtype=np.uint8)
    owner, p, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    check(lib().mp3s_message_reveal(b.ctypes.data if len(b) else None, len(b), C.byref(owner), C.byref(p), C.byref(n)))
    with _Owner(owner):
        return _view(p.value, np.uint8, (n.value,)).tobytes()


def parse_stream(data: bytes):
    """Host front end only (no GPU): Huffman-decoded spectra, side records, stego bits."""
    buf = np.frombuffer(data, dtype=np.uint8)
    owner, p = C.c_void_p(), Parsed()
    check(lib().mp3s_parse_stream(buf.ctypes.data, len(data), C.byref(owner), C.byref(p)))
    with _Owner(owner):
        n = p.n_frames
        return {"n_frames": n, "channels": p.nch, "sampling_rate": p.sampling_rate, "bit_rate": p.bit_rate,
                "dup_last_frame": p.dup_last_frame, "is": _view(p.is_, np.int16, (n, 2, 2, 576)),
                "si": _view(p.si, GRANULE_SI_DTYPE, (n, 2, 2)), "hdr": _view(p.hdr, FRAME_HDR_DTYPE, (n,)),
                "bits": _view(p.bits, np.uint8, (p.n_bits,)),
                "table_select": _view(p.table_select, np.int32, (n, 2, 2, 3)),
                "frame_size": _view(p.frame_size, np.int32, (n,))}


def _scanned_dict(p):
    """the dict of an mp3s_scanned, every array a copy"""
    n = p.n_frames
    return {"n_frames": n, "channels": p.nch, "sampling_rate": p.sampling_rate, "bit_rate": p.bit_rate,
            "dup_last_frame": p.dup_last_frame, "gpu_ok": bool(p.gpu_ok), "max_part2_3_length": p.max_part2_3_length,
            "side": _view(p.side, FRAME_SIDE_DTYPE, (n,)), "hdr": _view(p.hdr, FRAME_HDR_DTYPE, (n,)),
            "blob": _view(p.blob, np.uint8, (p.blob_len,)), "bits": _view(p.bits, np.uint8, (p.n_bits,)),
            "frame_size": _view(p.frame_size, np.int32, (n,))}


def scan_stream(data: bytes):
    """Host byte-level scan only (no GPU): frame side info + main-data blob for the device Huffman kernel."""
    buf = np.frombuffer(data, dtype=np.uint8)
    owner, p = C.c_void_p(), Scanned()
    check(lib().mp3s_scan_stream(buf.ctypes.data, len(data), C.byref(owner), C.byref(p)))
    with _Owner(owner):
        return _scanned_dict(p)


def walk_stream(data: bytes):
    """Host walk from frame header to frame header (no GPU): what the device-side parser (Context.parse_frames_dev) needs.
    regular == False: the stream needs scan_stream (false syncs, inherited header fields, pointers in front of the file)."""
    buf = np.frombuffer(data, dtype=np.uint8)
    owner, w = C.c_void_p(), Walked()
    check(lib().mp3s_walk_stream(buf.ctypes.data, len(data), C.byref(owner), C.byref(w)))
    with _Owner(owner):
        if not w.regular:
            return {"regular": False}
        n = w.n_frames
        stream = np.zeros(1, dtype=STREAM_REF_DTYPE)
        C.memmove(stream.ctypes.data, C.byref(w.stream), 40)
        return {"regular": True, "n_frames": n, "channels": w.nch, "sampling_rate": w.sampling_rate, "bit_rate": w.bit_rate,
                "dup_last_frame": w.dup_last_frame, "max_part2_3_length": w.max_part2_3_length, "any_silent": bool(w.any_silent),
                "blob_len": w.blob_len, "refs": _view(w.refs, FRAME_REF_DTYPE, (n,)), "stream": stream,
                "tables": _view(w.tables, np.uint8, (n, 4))}


def walk_rate(data: bytes, seconds=1.0):
    """frames per second one host thread walks `data` at (mp3s_debug_walk_rate: the host's share of a pipe job, no device)"""
    buf = np.frombuffer(data, dtype=np.uint8)
    r, n = C.c_double(), C.c_int64()
    check(lib().mp3s_debug_walk_rate(buf.ctypes.data, len(data), float(seconds), C.byref(r), C.byref(n)))
    return r.value, n.value


def stego_bits(tsel, nch, carry=None):
    """stego bits from the per-frame table-index words the device parser leaves (mp3s_stego_bits); -> (bits, carry)"""
    tsel = np.ascontiguousarray(tsel, dtype=np.uint64)
    carry = np.zeros(4, dtype=np.uint8) if carry is None else np.ascontiguousarray(carry, dtype=np.uint8).copy()
    owner, bits, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
    check(lib().mp3s_stego_bits(tsel.ctypes.data, len(tsel), nch, carry.ctypes.data, C.byref(owner), C.byref(bits), C.byref(n)))
    with _Owner(owner):
        return _view(bits.value, np.uint8, (n.value,)), carry


def rate_frames(samplerate, bitrate, nch, n_frames):
    out = np.zeros(n_frames, dtype=RATE_FRAME_DTYPE)
    pad = np.zeros(n_frames, dtype=np.int32)
    check(lib().mp3s_rate_frames(samplerate, bitrate, nch, n_frames, out.ctypes.data, pad.ctypes.data))
    return out, pad


def format_stream(samplerate, bitrate, ix, gr, scfsi):
    ix = np.ascontiguousarray(ix, dtype=np.int16)
    gr = np.ascontiguousarray(gr, dtype=GR_OUT_DTYPE)
    scfsi = np.ascontiguousarray(scfsi, dtype=np.int32)
    n = ix.shape[0]
    owner, mp3, ln = C.c_void_p(), C.c_void_p(), C.c_size_t()
    check(lib().mp3s_format_stream(samplerate, bitrate, n, ix.ctypes.data, gr.ctypes.data, scfsi.ctypes.data,
                                   C.byref(owner), C.byref(mp3), C.byref(ln)))
    with _Owner(owner):
        return _view(mp3.value, np.uint8, (ln.value,)).tobytes()


def debug_tables():
    """Host copy of the device constant tables as a numpy record (tests only)."""
    n = C.c_size_t()
    p = lib().mp3s_debug_tables(C.byref(n))
    assert n.value == DEV_TABLES_DTYPE.itemsize, (n.value, DEV_TABLES_DTYPE.itemsize)
    return _view(p, DEV_TABLES_DTYPE, (1,))[0]


def host_share(handle=None):
    """mp3s_ctx_host_share; without a context handle: the host's side alone (gpu_node_cpus 0), no GPU needed"""
    st = HostShare()
    check(lib().mp3s_ctx_host_share(handle, C.byref(st)))
    return {k: int(getattr(st, k)) for k, _ in HostShare._fields_ if k != "reserved"}


_default_ctx = None


def default_context():
    """Process-wide context, created on first use (raises without a GPU)."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx
