"""k_dec_stream at the edges of its runs and its set-up: int16 PCM through the default path against the oracle's, bit for bit.

A wave decodes `run` consecutive granules and primes itself with up to two granules in front of them (gi0 = -2, -1 or 0: as far as they
belong to the run's stream); a workgroup is four waves; the run's first inputs are asked for before the tables are staged, at addresses
clamped into the batch for a wave behind it.  launch_decode chooses the run length from the batch: 4 granules up to 8 192 granules, 5 from
there to 10 240 (dec_run_length).  So the small batches below are
     1 frame   2 granules: one wave, its run cut short by the batch's end;
     2 frames  one whole run;                 3 frames  a second run of two granules;
     5 frames  three runs, the last of two;   20 frames ten runs: two workgroups of four waves and one of two;
    21 frames  eleven runs, the last of two granules -- in every workgroup with fewer than four runs the other waves are behind the batch.
With whole frames and an even run length neither a run of one granule nor a stream that starts one granule in front of a run exists; both
need an odd run length, so the two-stream cases are batches of 4 100 to 4 103 frames (run = 5: run w starts at granule 5 w) whose
second stream starts on a run's first granule (frame 5 = granule 10, gi0 = 0), on its second (frame 3 = granule 6), one granule in front
of a run (frame 2 = granule 4, gi0 = -1) and further in front (gi0 = -2, every other run); 4 103 frames end in a run of one granule."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = (1, 2, 3, 5, 20, 21)
LONG_FRAMES = 4098                      # + 2, 3 or 5 frames in front: 8 200 .. 8 206 granules, run length 5


def i16_ref(orc, data):
    ref = orc.pcm_to_i16(orc.decode(data)["pcm"])
    ref.setflags(write=False)
    return ref


@pytest.fixture(scope="module")
def small_streams(orc):
    """(stream, the oracle's int16) per (mode, frames): long blocks, stereo and mono"""
    import frame_synth
    out = {}
    for mode in (0, 3):
        for n in SMALL:
            data = frame_synth.make_stream(700 + 10 * mode + n, n, mode=mode)
            out[(mode, n)] = (data, i16_ref(orc, data))
    return out


@pytest.fixture(scope="module")
def long_stream(orc):
    import frame_synth
    piece = frame_synth.make_stream(77, 6)
    data = frame_synth.concat(*([piece] * (LONG_FRAMES // 6)))
    return data, i16_ref(orc, data)


@pytest.fixture
def default_path(ctx):
    """the stream kernel at the proven bound, a one-file call as ONE batch (not as chunks through the context's pipe)"""
    if not (ctx.get_option("fused_decode") and ctx.get_option("fast_imdct")):
        pytest.skip("the stream kernel is switched off by this context's settings (tools/option_sweep.sh)")
    ctx.synth_mode(1.0)
    piped = ctx.get_option("file_pipeline")
    ctx.set_option("file_pipeline", 0)
    yield
    ctx.set_option("file_pipeline", piped)


@pytest.mark.parametrize("mode", (0, 3), ids=("stereo", "mono"))
@pytest.mark.parametrize("n", SMALL)
def test_small_batches_equal_the_oracle(ctx, mlib, default_path, small_streams, mode, n):
    data, ref = small_streams[(mode, n)]
    got = ctx.decode_stream(data, mlib.MP3S_PCM_I16)
    assert got["n_frames"] == n and ref.shape == (n * 1152, 1 if mode == 3 else 2)
    assert np.array_equal(got["pcm"], ref), (mode, n, int((np.asarray(got["pcm"]) != ref).sum()))


@pytest.mark.parametrize("front", (5, 3, 2), ids=("first_granule_of_a_run", "second_granule_of_a_run", "granule_in_front_of_a_run"))
def test_second_stream_starts_at_every_place_of_a_run(ctx, mlib, default_path, small_streams, long_stream, front):
    """two streams end to end in one batch (decode_streams: stream_first of the second = the first's frame count)"""
    a, ref_a = small_streams[(0, front)]
    b, ref_b = long_stream
    n_gran = 2 * (front + LONG_FRAMES)
    assert 8192 < n_gran <= 10240                                      # run length 5 (header comment)
    assert (2 * front) % 5 == {5: 0, 3: 1, 2: 4}[front]                 # where the second stream's first granule lies in its run
    got = ctx.decode_streams([a, b], mlib.MP3S_PCM_I16)
    assert np.array_equal(got[0]["pcm"], ref_a), front
    assert np.array_equal(got[1]["pcm"], ref_b), (front, int((np.asarray(got[1]["pcm"]) != ref_b).sum()))
    # ... and the other way round: the long stream in front, the batch's last run cut short (one granule of it left with 5 frames behind)
    got = ctx.decode_streams([b, a], mlib.MP3S_PCM_I16)
    assert np.array_equal(got[0]["pcm"], ref_b) and np.array_equal(got[1]["pcm"], ref_a), front


def test_short_and_mixed_blocks_keep_their_paths(ctx, mlib, orc, default_path):
    import frame_synth
    for seed, kw in ((31, dict(mode=1, mode_ext=2)), (33, dict(mode=3)), (34, dict(mode=0))):
        data = frame_synth.make_stream(seed, 21, block_types=(0, 1, 2, 3), allow_mixed=True, **kw)
        assert np.array_equal(ctx.decode_stream(data, mlib.MP3S_PCM_I16)["pcm"], i16_ref(orc, data)), seed


def test_guard_margin_of_these_batches(ctx, mlib, small_streams, long_stream):
    """r = |x_fast - x_exact| / eps_t, measured by the kernel's probe instantiation (tests/test_guard_margin.py): below 1 means the
    bound covers the sums.  The committed maximum over every stream kind is 0.039 (profiles/r06_guard_margin.json); a jump by an order
    of magnitude would mean the bound no longer describes the sums although every sample is still right.  Printed, and asserted < 1."""
    from test_guard_margin import margin
    worst = 0.0
    for name, data in (("21 frames stereo", small_streams[(0, 21)][0]), ("21 frames mono", small_streams[(3, 21)][0]), ("%d frames stereo" % LONG_FRAMES, long_stream[0])):
        n = ctx.decode_stream(data, mlib.MP3S_PCM_I16)["pcm"].size
        res = margin(ctx, mlib, lambda fmt: ctx.decode_stream(data, fmt)["pcm"], n)
        print("guard margin, %s: max r %.4f over %d samples, %d recomputed" % (name, res["max_r"], res["samples"], res["recomputed_by_fixup"]))
        worst = max(worst, res["max_r"])
    assert worst < 1.0, worst
