"""MP3 lists as torch tensors that never leave the GPU (include/mp3s.h section vi-f).

decode() leaves a list of MP3 files in a device tensor [B, C, T] -- channels first, planar, float32 = int16 / 32768 or int16 -- and
encode() makes MP3 files (with hidden messages, if asked) of such a tensor.  The samples do not cross PCIe in either direction: the
library's kernels read and write the tensor's memory.  decode(samplerate=...) leaves every slot at ONE sampling rate whatever the files'
rates are (16 kHz for a model, say), and encode(resample=...) takes a tensor at any rate: both resample on the device, with the exact
integer polyphase filter of the "wav_resample" option.  qmdct() (section vi-g) leaves the quantised MDCT coefficients of the list -- what
a hidden payload lives in -- in an int16 device tensor [B, C, granules, 576]: the front half of the decode, no transform.

This is the only module of the package that imports torch, and it does so when a function is first called: the C library and
mp3stego._lib stay torch-free.  The library works on its context's own stream; both functions synchronise torch's current stream of
the device before the call, and the library's stream has been synchronised when they return.
"""
from mp3stego import _lib


def _torch():
    import torch
    return torch


def _formats(torch):
    return {torch.int16: "i16", torch.float32: "f32"}


def _check(torch, t, ctx, what):
    """the tensor the library is handed: [B, C, T], int16 or float32, contiguous, on the context's device"""
    if not isinstance(t, torch.Tensor) or t.dim() != 3:
        raise ValueError(f"{what}: a tensor [B, C, T] is expected")
    if t.dtype not in _formats(torch):
        raise ValueError(f"{what}: dtype {t.dtype}, int16 or float32 is expected")
    if not t.is_contiguous():
        raise ValueError(f"{what}: the tensor is not contiguous")
    if t.device.type != "cuda" or t.device.index != ctx.device:
        raise ValueError(f"{what}: the tensor is on {t.device}, the context works on cuda:{ctx.device}")
    if t.shape[1] not in (1, 2):
        raise ValueError(f"{what}: {t.shape[1]} channels, 1 or 2 are expected")


def _rate(value, what):
    if isinstance(value, bool) or not isinstance(value, int) or value <= 0:
        raise ValueError(f"{what}: a positive integer number of Hz is expected, not {value!r}")
    return value


def decode(mp3s, rows=None, first_rows=None, channels=2, dtype=None, ctx=None, out=None, per_file=False, samplerate=None):
    """Decode the MP3 files `mp3s` (byte strings; None: a missing file) into one device tensor.

    Returns (batch, lengths, infos): batch [len(mp3s), channels, T] of dtype (torch.float32, the default: int16 / 32768, or torch.int16)
    on the context's device, file i's rows from first_rows[i] (0) on in batch[i], zeros behind them; lengths: an int64 CPU tensor of
    the rows of each slot that are samples; infos: the dicts of Context.decode_batch (per_file=True: the Mp3sError of a file that
    cannot be decoded, whose slot is zero and whose length is 0; otherwise such a file fails the call).
    rows=None sizes T as the largest n_rows - first_row of the list, which costs one more run of the host front end over the files
    (Context.batch_rows); say rows when you know it.  A stereo file into channels=1 is (l + r) / 2, a mono file into channels=2 goes
    into both planes.  samplerate=None: nothing is resampled, infos[i]["sampling_rate"] says what the rows of a slot are.
    samplerate=16000 (any rate in Hz): every file is resampled on the device to that rate, each by its own ratio; rows, first_rows and
    lengths then count rows at `samplerate`, T is sized from them, and infos[i] gains in_rows, out_rate, L and M.  A file whose rate
    the resampler refuses for `samplerate` (more than 1280 phases or 256 taps) fails like a file that cannot be decoded.
    out= reuses a tensor of the caller's ([len(mp3s), C, T]: channels, dtype and rows are taken from it); the work torch's current
    stream has pending on it is waited for first."""
    torch = _torch()
    ctx = ctx or _lib.default_context()
    n = len(mp3s)
    if n == 0:
        raise ValueError("an empty list")
    if samplerate is not None:
        samplerate = _rate(samplerate, "samplerate")
    device = torch.device("cuda", ctx.device)
    if out is not None:
        _check(torch, out, ctx, "out")
        if out.shape[0] != n:
            raise ValueError(f"out: {out.shape[0]} slots for {n} files")
        channels, dtype, rows = int(out.shape[1]), out.dtype, int(out.shape[2])
    else:
        dtype = dtype or torch.float32
        if dtype not in _formats(torch):
            raise ValueError(f"dtype {dtype}, int16 or float32 is expected")
        if rows is None:
            firsts = first_rows if first_rows is not None else [0] * n
            sized = ctx.batch_rows(mp3s, per_file=per_file, samplerate=samplerate)
            rows = max([1] + [s["n_rows"] - int(f) for s, f in zip(sized, firsts) if not isinstance(s, Exception)])
        out = torch.empty((n, int(channels), int(rows)), dtype=dtype, device=device)
    torch.cuda.current_stream(device).synchronize()       # (the memory may be a block torch's stream has not finished with)
    infos = ctx.decode_batch(mp3s, out.data_ptr(), out.numel() * out.element_size(), int(rows), first_rows, int(channels),
                             _formats(torch)[dtype], per_file, samplerate)
    lengths = torch.tensor([0 if isinstance(i, Exception) else i["valid_rows"] for i in infos], dtype=torch.int64)
    return out, lengths, infos


def qmdct(mp3s, granules=None, first_granules=None, channels=2, ctx=None, out=None, per_file=False):
    """The quantised MDCT coefficients of the MP3 files `mp3s` (byte strings; None: a missing file) as one device tensor: the int16 `is`
    values of the Huffman decode, the representation a hidden payload lives in and the input of learned steganalysis (include/mp3s.h,
    section vi-g).  No transform runs and nothing comes down.

    Returns (batch, infos): batch int16 [len(mp3s), channels, granules, 576] on the context's device, file i's granule rows (two a
    frame, lines as they lie in the stream: short blocks are not reordered) from first_granules[i] (0) on in batch[i], zeros behind
    them and in plane 1 of a mono file; infos: the dicts of Context.qmdct_batch, "valid_granules" the rows of a slot that are spectra
    (per_file=True: the Mp3sError of a file that fails, whose slot is zero; otherwise such a file fails the call).  A stereo file has
    no one-channel spectrum: with channels=1 it fails.  granules=None sizes the tensor as the largest n_granules - first_granule of
    the list, which costs one more run of the host front end over the files; say granules when you know it.
    out= reuses a tensor of the caller's ([len(mp3s), C, granules, 576] int16, contiguous); the work torch's current stream has
    pending on it is waited for first."""
    torch = _torch()
    ctx = ctx or _lib.default_context()
    n = len(mp3s)
    if n == 0:
        raise ValueError("an empty list")
    device = torch.device("cuda", ctx.device)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dim() != 4 or out.dtype != torch.int16 or out.shape[3] != 576 or out.shape[1] not in (1, 2):
            raise ValueError("out: an int16 tensor [B, C, granules, 576] with 1 or 2 channels is expected")
        if not out.is_contiguous():
            raise ValueError("out: the tensor is not contiguous")
        if out.device.type != "cuda" or out.device.index != ctx.device:
            raise ValueError(f"out: the tensor is on {out.device}, the context works on cuda:{ctx.device}")
        if out.shape[0] != n:
            raise ValueError(f"out: {out.shape[0]} slots for {n} files")
        channels, granules = int(out.shape[1]), int(out.shape[2])
    else:
        if granules is None:
            firsts = first_granules if first_granules is not None else [0] * n
            sized = ctx.qmdct_batch(mp3s, None, 0, 0, channels=int(channels), per_file=per_file)
            granules = max([1] + [s["n_granules"] - int(f) for s, f in zip(sized, firsts) if not isinstance(s, Exception)])
        out = torch.empty((n, int(channels), int(granules), 576), dtype=torch.int16, device=device)
    torch.cuda.current_stream(device).synchronize()       # (the memory may be a block torch's stream has not finished with)
    infos = ctx.qmdct_batch(mp3s, out.data_ptr(), out.numel() * 2, int(granules), first_granules, int(channels), per_file)
    return out, infos


def encode(batch, lengths, samplerate, bitrate=320, messages=None, hide_bits=None, ctx=None, per_file=False, resample=0):
    """Encode the items of the device tensor `batch` [B, C, T] (int16, or float32 in [-1, 1): clamp(rint(x * 32768))) as MP3 files:
    item i is batch[i, :, :lengths[i]], its last frame zero-filled, a mono item in both channels of the (stereo) file.  messages /
    hide_bits as for Context.encode_files.  torch's current stream is synchronised before the call, so what wrote the batch there has
    finished; the batch may be reused when the call returns.  Returns the dicts of Context.encode_batch.
    resample=0: the batch is at 32 000, 44 100 or 48 000 Hz.  resample=1: the batch is at ANY rate `samplerate` and is resampled on the
    device to the MP3 rate the "wav_resample" option's auto rule picks (16 000 -> 32 000, 22 050 -> 44 100, a supported rate stays);
    resample=32000 / 44100 / 48000 forces the target.  The dicts' sampling_rate is the target."""
    torch = _torch()
    ctx = ctx or _lib.default_context()
    if resample not in (0, 1, 32000, 44100, 48000) or isinstance(resample, bool):
        raise ValueError(f"resample: 0, 1, 32000, 44100 or 48000 is expected, not {resample!r}")
    if resample:
        samplerate = _rate(samplerate, "samplerate")
    _check(torch, batch, ctx, "batch")
    lengths = [int(x) for x in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
    torch.cuda.current_stream(batch.device).synchronize()
    return ctx.encode_batch(batch.data_ptr(), batch.shape[0], batch.shape[1], _formats(torch)[batch.dtype], batch.shape[2], lengths,
                            samplerate, bitrate, hide_bits, messages, per_file, resample)
