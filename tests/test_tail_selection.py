"""A selection queued on a pipe's tail stream, followed at once by a rate loop that writes the same variant buffers (select_step /
rate_step, csrc/mp3s_api.cpp; enc_issue): jobs back to back through a pipe, with and without a tail stream and with the events as
records or as dispatch signals, give byte for byte what hide_messages gives on a fresh default context -- and all of them on the
device's own path, so that the test cannot pass by leaving it."""
import pytest

pytestmark = pytest.mark.gpu

FRAMES = (40, 60, 90, 130)
TEXT = "abcdefghijkl"
# the longest message of job k: they grow, so that the selection scratch (streams x reach) has to grow while a tail is in flight
LENGTHS = (1, 4, 6, 9, 11, 12)


def _message(k, i):
    """1 to 12 characters, another text for every job k and file i"""
    return (TEXT[k:] + TEXT[:k])[: max(1, LENGTHS[k] - i)]


@pytest.fixture(scope="module")
def jobs_and_reference(mlib):
    """six jobs, a list of one file and a list of all four taking turns; -> [(files, messages, what hide_messages gives)]"""
    from synth_pcm import synth_pcm
    ctx = mlib.Context(0)
    try:
        files = [bytes(ctx.encode_pcm(synth_pcm(n, seed=500 + n), 44100, 128)["mp3"]) for n in FRAMES]
        out = []
        for k in range(6):
            fl = files if k % 2 else [files[(k // 2) % len(files)]]
            msgs = [_message(k, i) for i in range(len(fl))]
            want = ctx.hide_messages(fl, msgs)
            for w, m in zip(want, msgs):
                assert not isinstance(w, Exception), (k, w)
                assert bytes(mlib.reveal_message(bytes(w["data"]))["data"]) == m.encode(), (k, m)
            out.append((fl, msgs, [bytes(w["data"]) for w in want]))
        return out
    finally:
        ctx.close()


@pytest.mark.parametrize("pipe_signals", (0, 2, 3))
@pytest.mark.parametrize("pipe_tail", (0, 1))
def test_selection_on_the_tail_in_front_of_the_next_rate_loop(mlib, jobs_and_reference, pipe_tail, pipe_signals):
    jobs = jobs_and_reference
    ctx = mlib.Context(0)
    try:
        ctx.set_option("pipe_tail", pipe_tail)
        ctx.set_option("pipe_signals", pipe_signals)
        pipe = mlib.Pipe(ctx, depth=3, scan_threads=2)
        try:
            got, nxt = [], 0
            while len(got) < len(jobs):
                while nxt < len(jobs) and pipe.submit(jobs[nxt][0], jobs[nxt][1]) is not None:   # back to back, as far as the depth allows
                    nxt += 1
                t, res = pipe.collect()
                assert t == len(got)
                got.append([r if isinstance(r, Exception) else bytes(r["data"]) for r in res])
            st = pipe.stats()
        finally:
            pipe.close()
    finally:
        ctx.close()
    for k, (res, (_, msgs, want)) in enumerate(zip(got, jobs)):
        assert res == want, (pipe_tail, pipe_signals, k)
        for data, m in zip(res, msgs):
            assert bytes(mlib.reveal_message(data)["data"]) == m.encode(), (pipe_tail, pipe_signals, k, m)
    # every job on the device's own path: none resolved by the host, none run again through the synchronous call
    assert st["collected"] == len(jobs) and st["fast"] == len(jobs) and st["resolved"] == 0 and st["slow"] == 0, st
