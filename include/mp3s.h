/*
 * mp3s.h -- C-ABI of the MI355X-native MP3 steganography hot path.
 *
 * Drop-in boundary for tomershay100/mp3-steganography-lib (mp3stego-lib 1.1.8).
 * The reference has no FFI layer: its boundary is the Python API re-exported at
 * reference mp3stego/__init__.py:1-4 (Decoder, Encoder, Steganography).  The
 * Python package shipped in mp3-steganography-lib_amd/mp3stego/ keeps that
 * surface and binds the entry points below with ctypes.
 * "replaces:" lines name the reference code each entry point stands in for.
 *
 * Conventions
 *   - every function returns MP3S_OK (0) or a negative MP3S_E_* code, never
 *     exits; mp3s_last_error() gives a message for the calling thread;
 *   - plain pointers + sizes, no C++/torch types; the caller owns all host
 *     buffers it passes in; buffers returned through mp3s_buf are owned by the
 *     library until mp3s_buf_free();
 *   - a context is bound to ONE HIP device (one process per GPU); calls on one
 *     context are serialised by the caller;
 *   - transforms run ONLY on the GPU: without a usable HIP device
 *     mp3s_ctx_create() fails with MP3S_E_NO_DEVICE and nothing falls back to
 *     the CPU.  The serial bit parsing / packing stages stay on the host by
 *     design.
 */
#ifndef MP3S_H
#define MP3S_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MP3S_OK 0
#define MP3S_E_NO_DEVICE (-1)   /* no HIP device / HIP runtime error at init */
#define MP3S_E_HIP (-2)         /* HIP runtime error during a call */
#define MP3S_E_ARG (-3)         /* bad argument (null, size, range) */
#define MP3S_E_MALFORMED (-4)   /* input the reference raises IndexError/KeyError on */
#define MP3S_E_UNSUPPORTED (-5) /* input the reference itself cannot process (mono encode, partial frame) */
#define MP3S_E_STEP_RANGE (-6)  /* quantizer step left the table (reference: IndexError) */
#define MP3S_E_NOMEM (-7)
#define MP3S_E_EXIT (-8)        /* the reference calls sys.exit(text) here; the text is in mp3s_last_error() */
#define MP3S_E_BUSY (-9)        /* mp3s_pipe_submit: every slot is taken, collect a result first; mp3s_pipe_collect: nothing pending */
#define MP3S_E_TABLES (-10)     /* a constant table built with this host's libm is not the one a kernel was compiled for (the encoder's analysis
                                 * filter: csrc/analysis_plan.h, csrc/analysis_sign_plan.h); the encode entry points refuse, decoding works */

#define MP3S_PCM_I16 0 /* (pcm*32767) truncated toward zero, low 16 bits: reference decoder/MP3_Parser.py:91 */
#define MP3S_PCM_F32 1
#define MP3S_PCM_F64 2 /* the reference's own float64 samples, bit for bit */

typedef struct mp3s_ctx mp3s_ctx;
typedef struct mp3s_buf mp3s_buf; /* library-owned result, released with mp3s_buf_free() */

/* ---------------------------------------------------------------- records (device + host layout) */

/* per granule*channel side record consumed by the decode transform
 * replaces: the arguments of re_quantize(), reference decoder/Frame.py:157-176 */
typedef struct {
    uint8_t global_gain, scalefac_scale, block_type, mixed_block_flag, preflag;
    uint8_t sub_block_gain[3];
    uint8_t scale_fac_l[22];
    uint8_t scale_fac_s[3][13];
    uint8_t pad[3];
} mp3s_granule_si; /* 72 bytes */

/* per frame record.  stream_first = index (in the batch) of the frame that starts the
 * stream this frame belongs to: overlap/fifo state is zero before it
 * (reference decoder/Frame.py:234-235, encoder/MP3_Encoder.py:528-534). */
typedef struct {
    uint8_t sr_idx;    /* 0 = 44.1 kHz, 1 = 48 kHz, 2 = 32 kHz (header bits) */
    uint8_t nch;
    uint8_t ms_stereo; /* JointStereo && (byte3 & 0x20): reference Frame.py:273 */
    uint8_t flags;
    uint32_t stream_first;
} mp3s_frame_hdr; /* 8 bytes */

/* per frame input of the rate loop */
typedef struct {
    int32_t max_bits;     /* min(mean_bits // nch, 4095): reference MP3_Encoder.py:894-912 */
    int32_t sr_idx;
    int32_t hide_end;     /* the message of this frame's stream ends at hide[hide_end]: a batch of streams keeps their
                           * messages back to back in one array (mp3s_rate_frames sets INT32_MAX = the array's end) */
    int32_t stream;       /* index of the frame's stream in the batch (into mp3s_chain_seg[]); mp3s_rate_frames sets 0 */
} mp3s_rate_frame; /* 16 bytes */

/* per granule*channel result of the rate loop
 * replaces: GrInfo as left by __iteration_loop, reference encoder/MP3_Encoder.py:81-103, 760-815 */
typedef struct {
    int32_t part2_3_length; /* WITHOUT stuffing (added by the host back end, MP3_Encoder.py:1097-1145) */
    int32_t big_values, count1, quantizer_step, region0_count, region1_count, count1table_select;
    int32_t table_select[3];
    int32_t address[3];     /* address1/2/3 as left behind (persist per (gr,ch) across frames) */
    int32_t n_tables;       /* number of non-zero table_select: advance of the hide cursor (:808-809) */
    int32_t flags;          /* MP3S_RF_* */
    int32_t reserved0;      /* the address1/2/3 the unit was given, a1 | a2 << 10 | a3 << 20 (0 without d_state_in) */
    int32_t xrmax;
    int32_t reserved;
} mp3s_gr_out; /* 72 bytes */
#define MP3S_RF_ACTIVE 1      /* xrmax != 0: outer loop ran */
#define MP3S_RF_USED_ADDR_IN 2 /* the incoming address1/2/3 were read before being overwritten */
#define MP3S_RF_STEP_RANGE 4  /* quantizer step left the table */
#define MP3S_RF_LOG_GUARD 8   /* reserved: never set since the band energies come from a table built with the host's libm */
#define MP3S_RF_LISTED 16     /* the device's chain check has put the unit on its list of re-runs (mp3s_chain_redo_dev): the list entry's wave is the
                               * unit's one writer in that launch, a re-run that follows its chain of inheriting units stops in front of it */

/* ---------------------------------------------------------------- context */
int mp3s_ctx_create(int device, mp3s_ctx **out);
/* how many HIP devices this process can open (what a launcher of one process per GPU sizes itself by); 0 and MP3S_OK
 * on a host without one */
int mp3s_device_count(int *n);
void mp3s_ctx_destroy(mp3s_ctx *ctx);
const char *mp3s_last_error(void);
const char *mp3s_version(void);
int mp3s_device_name(mp3s_ctx *ctx, char *buf, size_t n);
/* the device's PCI address as sysfs spells it ("0000:c5:00.0"): what a monitor thread that must not touch the GPU reads clocks and
 * power by (/sys/bus/pci/devices/<address>/...; bench.py's `sustained` region) */
int mp3s_device_pci(mp3s_ctx *ctx, char *buf, size_t n);
int mp3s_sync(mp3s_ctx *ctx);
/* Stream order between two contexts of one device: work submitted to ctx after this call starts only when everything
 * submitted to other before it has finished.  This is how a second context runs the bit-level front end of the next
 * batch (mp3s_huffman_decode_dev) under the transform kernels of the current one. */
int mp3s_ctx_wait(mp3s_ctx *ctx, mp3s_ctx *other);
/* The same without a new record on other: work submitted to ctx after this call starts when what other's order event was LAST
 * recorded behind has finished -- the previous mp3s_ctx_wait(.., other), or, with MP3S_OPT_RATE_SIGNALS, other's last rate loop.
 * (Never recorded: no wait.)  Several contexts can wait for one point of another's stream for the price of one packet there, or none. */
int mp3s_ctx_wait_last(mp3s_ctx *ctx, mp3s_ctx *other);
/* Options of a context (what used to be MP3S_* environment switches read in the middle of a job: the environment now only
 * provides the DEFAULTS, read once by mp3s_ctx_create -- the names in brackets -- so two contexts of one process can differ
 * and no job path calls getenv).  Set them while nothing is in flight on the context. */
#define MP3S_OPT_SELECT 1          /* 1: the message cursor is decided on the device (mp3s_rate_select_dev); 0: guessed cursors,
                                    * checked and resolved afterwards [MP3S_NO_SELECT=1 -> 0] */
#define MP3S_OPT_REDO 2            /* 1: the chain check's re-runs on the device (mp3s_chain_redo_dev) [MP3S_NO_REDO=1 -> 0] */
#define MP3S_OPT_FAST_IMDCT 3      /* 1: int16 decode through the mirrored, fused IMDCT behind the guard [MP3S_FAST_IMDCT=0 -> 0] */
#define MP3S_OPT_PIPE_TAIL 4       /* a pipe created on this context (mp3s_pipe_create; not the context's own, which runs the chunks of one file and takes
                                    * none) puts a job's tail (selection, chain check, bit packing) on a stream of its own: 0 never, 1 (default) the
                                    * candidate its rehearsal likes best unless that clearly loses, 2 only if the rehearsal is faster with one [MP3S_PIPE_TAIL] */
#define MP3S_OPT_CHUNK_FRAMES 5    /* frames per chunk when ONE file goes through the overlapped stages (mp3s_hide_message, mp3s_clear_file,
                                    * mp3s_decode_file, mp3s_decode_stream); 0 = chosen from the file's length [MP3S_CHUNK_FRAMES] */
#define MP3S_OPT_DEVICE_PARSE 6    /* 1: side info and main-data gather on the device (mp3s_parse_frames_dev) wherever the stream is
                                    * regular; 0: the host's byte-level scan everywhere [MP3S_DEVICE_PARSE=0 -> 0] */
#define MP3S_OPT_FILE_PIPELINE 7   /* 1: the one-file calls above run as chunks through overlapped stages; 0: scan, upload, kernels,
                                    * download one after the other as in round 2 [MP3S_FILE_PIPELINE=0 -> 0] */
#define MP3S_OPT_SCAN_THREADS 8    /* host threads a multi-file call may use for its front end; 0 = from the CPUs this process may
                                    * run on (sched_getaffinity, cgroup quota) divided by the ranks on this host [MP3S_SCAN_THREADS] */
#define MP3S_OPT_FIRST_CHUNK_FRAMES 9 /* frames of the first chunk of a one-file call (the device starts when it has been walked); 0 = chosen
                                       * from the file's length; never shorter than what the message can reach [MP3S_FIRST_CHUNK_FRAMES] */
#define MP3S_OPT_FILE_UP 10        /* 1: a one-file call uploads the whole file from the context's helper thread; 0: each chunk's piece from the
                                    * calling thread, as files above 1 GB go [MP3S_NO_FILE_UP=1 -> 0] */
#define MP3S_OPT_HUF_LANES 11      /* decoding lanes per wave of the Huffman kernel: 0 = picked from the launch's size (32 up to 8 192 frames,
                                    * 64 beyond), or 8 | 16 | 32 | 62 (64 lanes in workgroups of two waves) | 64 [MP3S_HUF_LANES] */
#define MP3S_OPT_NUMA 12           /* 1: a pipe's workers and page-locked staging are bound to the CPUs of the GPU's NUMA node [MP3S_NO_NUMA=1 -> 0] */
#define MP3S_OPT_FLOAT_FAST 13     /* 1: float32 output may take the mirrored, fused IMDCT and the split synthesis of the int16 path (no guard:
                                    * the error is below 1e-9 of full scale, the contract's tolerance is 1e-5 relative); 0 (default): the float
                                    * formats are bit-identical to the reference [MP3S_FLOAT_FAST=1 -> 1] */
#define MP3S_OPT_FAIL_CHUNK 14     /* test aid: the k-th chunk (k = value, counted from 1) of the next one-file call fails with MP3S_E_HIP after
                                    * its front end has been queued; the option clears itself when it fires */
#define MP3S_OPT_FUSED_DECODE 15   /* 1 (default): the fast decode paths (int16; float32 under MP3S_OPT_FLOAT_FAST) run requantisation .. synthesis as ONE
                                    * kernel, a wave-local stream with no array between IMDCT and synthesis (k_decode_stream.hpp; timed as dec_synth);
                                    * 0: two kernels with the subband samples in device memory [MP3S_FUSED_DECODE=0 -> 0] */
#define MP3S_OPT_FUSED_ENCODE 16   /* 1: analysis filter bank and MDCT as ONE kernel, the subband samples between them in LDS (k_enc_fused; timed as enc_analysis,
                                    * no encode scratch, 221 MB less traffic per 10 000 frames); 0 (default): two kernels with the samples in device memory --
                                    * measured faster: the one kernel's workgroup barriers and its 67 KB of LDS per workgroup cost more than the round trip
                                    * through memory [MP3S_FUSED_ENCODE=1 -> 1] */
#define MP3S_OPT_ANALYSIS_SHARED 0 /* 1 (default): the analysis filter bank (k_enc_analysis, k_enc_fused) computes a product once for coefficients that are equal
                                    * up to SIGN (csrc/analysis_sign_plan.h: 1 030 products per slot; the negated product follows exactly from the positive
                                    * one), wave by wave wherever no window sum it would negate is zero -- bit-identical; 0: every wave of a launch takes the
                                    * matrixing that shares equal coefficients only (1 516 products), which waves of silence and stream starts take either
                                    * way.  (Number 0: the slot the numbering had left free.) [MP3S_ANALYSIS_SHARED=0 -> 0] */
#define MP3S_OPT_PIPE_DEC 17      /* 1: a pipe created on this context runs the decode transform of job k + 1 on a stream of its own, under the encode
                                    * transforms and the rate loop of job k [MP3S_PIPE_DEC=0|1] */
#define MP3S_OPT_RATE_SIGNALS 18   /* 1: the dispatch of the rate loop (mp3s_rate_variants_dev, mp3s_rate_loop_dev) carries the context's order event as its
                                    * completion signal: another context's mp3s_ctx_wait_last(other, this) then waits for the rate loop without a
                                    * record packet of its own in this context's queue (a record or a wait between two kernels costs the stream 7-8 us
                                    * of nothing: tools/timeline.sh) [MP3S_RATE_SIGNALS=0|1, default 0] */
#define MP3S_OPT_PIPE_SIGNALS 19   /* bit 0: in a pipe and in the one-file calls the last decode dispatch carries the event the front end waits for as its own
                                    * completion signal, bit 1: the rate loop the event the tail stream waits for; 0 (default): event records behind them.
                                    * Measured (round 5, docs/LOG.md): 3 gives the pipe +1.5 % (18.0 -> 18.3 M frames/s) and now and then puts a context's
                                    * one-file calls into a slower order of its streams (1.1 -> 1.4 ms per 10 000 frames): off [MP3S_PIPE_SIGNALS=0..3] */
#define MP3S_OPT_WAV_IMPORT 20     /* 1: mp3s_encode_file, mp3s_encode_files and mp3s_pipe_submit_encode (a pipe keeps the value its context had when the pipe
                                    * was created) read their WAV files by the import rules of mp3s_wav_import_info -- RIFF chunk walk over the whole file,
                                    * mono and stereo, 8/16/24/32-bit PCM, float32, WAVE_FORMAT_EXTENSIBLE, any length; the samples become the encoder's
                                    * int16 stereo frames on the device (k_wav_import); 0 (default): the reference's reader, refusals and over-reads
                                    * (mp3s_wav_parse) [MP3S_WAV_IMPORT=1 -> 1] */
#define MP3S_OPT_WAV_RESAMPLE 21   /* the encode calls of MP3S_OPT_WAV_IMPORT resample files of other sampling rates on the device (k_wav_resample, rules at
                                    * mp3s_wav_resample_info).  0 (default): off, every call behaves as without the option.  1: a file whose rate is not
                                    * 32 000 / 44 100 / 48 000 Hz is resampled to the target of the auto rule, files at a supported rate are untouched.
                                    * 32000 / 44100 / 48000: every file not already at that rate is resampled to it.  Any other value: MP3S_E_ARG.  A
                                    * non-zero value implies the reader of MP3S_OPT_WAV_IMPORT for the encode calls; a pipe keeps the value its context had
                                    * when the pipe was created [MP3S_WAV_RESAMPLE=1|32000|44100|48000] */
#define MP3S_OPT_COUNT 22
/* what became of the one-file calls of this context (mp3s_hide_message, mp3s_clear_file, mp3s_decode_file, mp3s_decode_stream,
 * mp3s_hide_message_chunked): files that went through the overlapped stages as chunks, their chunks, chunks that were run
 * again because they depended on a carry the guess got wrong, chunks whose chains the host resolved, and files that took
 * the stages one after the other instead (streams the frame walk does not take, mono re-encodes, ...) */
typedef struct {
    int64_t files, chunks, reruns, resolved, fallbacks;
    /* the context's own pipe (made by its first one-file call): what choosing its streams took (microseconds; part of that first
     * call's time), the miniature jobs rehearsed, the choice and whether stages seem to share hardware queues -- mp3s_pipe_stats */
    int64_t rehearsal_us, rehearsals, lanes, queue_shared;
} mp3s_run_stats;
int mp3s_ctx_run_stats(mp3s_ctx *ctx, mp3s_run_stats *out);
/* What a rank of a multi-process launch holds of the host (all optional): page-locked bytes this PROCESS keeps pooled between calls and the
 * cap it keeps them under (the ranks of a host share its lockable memory: 4 GB / LOCAL_WORLD_SIZE, at least 1 GB), the ranks it believes
 * share the host, the CPUs it may run on, and how many of those lie on the NUMA node of the context's GPU (what a pipe's workers and
 * staging are bound to with MP3S_OPT_NUMA; 0 = unknown, nothing is bound).  ctx may be NULL: the host's side alone (gpu_node_cpus = 0),
 * what a rank would be told without a GPU in reach (the eight-rank CPU test, tests/test_distributed.py). */
typedef struct {
    uint64_t pinned_pooled_bytes, pinned_pool_cap_bytes;
    int32_t local_world_size, cpus_allowed, gpu_node_cpus, reserved;
} mp3s_host_share;
int mp3s_ctx_host_share(mp3s_ctx *ctx, mp3s_host_share *out);
int mp3s_ctx_set_option(mp3s_ctx *ctx, int option, int64_t value);
int mp3s_ctx_get_option(mp3s_ctx *ctx, int option, int64_t *value);
/* host copy of the constant tables uploaded to the device (struct DevTables of csrc/mp3s_tables.h), for tests */
const void *mp3s_debug_tables(size_t *bytes);
/* host (glibc) evaluation of the __calc_scfsi energies of one granule*channel: en[0..20] bands, en[21] total.
 * The kernel's tabulated energies are cross-checked against this in the tests. */
int mp3s_debug_scfsi_energies(const int32_t *xr576, int sr_idx, int32_t *en22);

/* A probe of the int16 decode's guard (reference decoder/MP3_Parser.py:91 truncates pcm * 32767, decoder/Frame.py:65-154 is the
 * order of the sums it truncates): while d_x / d_eps (device arrays of `capacity` doubles) are set, the fused int16 decode (k_dec_stream)
 * also leaves per sample of a call its fast value x -- fp64, before the truncation -- and the width eps its guard compared with (infinite
 * for a granule it does not vouch for at all), at the sample's index in the call's PCM.  |x - 32767 * exact fp64 PCM| / eps is the margin
 * of the bound (tests/test_guard_margin.py asserts <= 0.5).  NULL, NULL, 0 ends the probe.  Not for production calls: 16 bytes more per sample.
 * The probe is an instantiation of the stream kernel: while it is set, an int16 decode that would not run that kernel (MP3S_OPT_FUSED_DECODE or
 * MP3S_OPT_FAST_IMDCT off, mp3s_synth_mode with scale 0) returns MP3S_E_ARG instead of leaving the arrays as they were; float formats never fill them. */
int mp3s_debug_guard_margin(mp3s_ctx *ctx, double *d_x, double *d_eps, int64_t capacity);

/* host decode (scalefactors + Huffman) of ONE frame of a scanned stream: what the stream pipelines do with the frames the
 * device Huffman kernel flags (exact for streams the scan marks gpu_ok); exposed for the tests.  side = that frame's
 * record, blob = the stream's blob; is2304 = int16 [2][2][576], si4 = mp3s_granule_si [2][2] */
int mp3s_debug_parse_scanned_frame(const void *frame_side, const uint8_t *blob, int16_t *is2304, mp3s_granule_si *si4);

/* the host's share of a job of the overlapped stages, alone: the frame walk of `file` over and over for about `seconds`
 * (the frame table written into one reused buffer, table counts for the first 1 000 code books as a hide job asks for them);
 * *frames_per_s = what one thread sustains.  No device involved (round 4 ran it in N processes side by side: docs/LOG.md). */
int mp3s_debug_walk_rate(const uint8_t *file, size_t len, double seconds, double *frames_per_s, int64_t *frames_per_pass);

/* device memory owned by the caller through the context (for resident pipelines / benchmarks) */
int mp3s_dev_alloc(mp3s_ctx *ctx, size_t bytes, void **dptr);
int mp3s_dev_free(mp3s_ctx *ctx, void *dptr);
int mp3s_dev_upload(mp3s_ctx *ctx, void *dptr, const void *host, size_t bytes);
int mp3s_dev_download(mp3s_ctx *ctx, void *host, const void *dptr, size_t bytes);
int mp3s_dev_memset(mp3s_ctx *ctx, void *dptr, int value, size_t bytes);
/* device to device on the context's stream, asynchronous (e.g. a template of assumed cursors into place at the top of a step) */
int mp3s_dev_copy(mp3s_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);
/* HIP-event timer on the context's stream (the stream every kernel below is launched on) */
int mp3s_timer_start(mp3s_ctx *ctx);
int mp3s_timer_stop(mp3s_ctx *ctx, float *ms);
/* The int16 decode format takes FAST kernels -- an IMDCT of 18 sums and their mirror images, a synthesis by even / odd
 * splitting of the 32-point cosine sums (a sixth of the multiplications), both with fused multiply-adds -- behind a guard: a
 * sample whose value * 32767 lies within a proven bound of an integer is computed again from the Huffman output in the
 * reference's operation order (a fix-up kernel behind the synthesis), so the int16 PCM is the reference's, sample for sample
 * (derivation of the bound: DESIGN.md section 2; the float formats always run the exact kernels and are bit-identical to
 * the reference).
 * eps_scale: 1 = the proven bound (default), 0 = always the exact kernels, > 1 = a wider guard (tests: forces samples
 * through the exact path).  *exact_samples (optional) = samples the guard has sent there since the last call. */
int mp3s_synth_mode(mp3s_ctx *ctx, double eps_scale, int64_t *exact_samples);
/* a plain device-to-device copy kernel over `bytes` (read + write counted), `iters` launches timed with HIP events on the
 * context's stream: the HBM bandwidth a streaming kernel achieves on this device, to set beside the data-sheet peak */
int mp3s_bench_copy(mp3s_ctx *ctx, size_t bytes, int iters, double *gb_per_s);
/* per-kernel HIP-event timing on the same stream: enable, run, then collect the summed milliseconds and launch
 * counts of the kernels in this order: dec_imdct, dec_synth, enc_analysis, enc_mdct, rate_loop, dec_huffman,
 * enc_pack, chain (the pair of mp3s_chain_resolve_dev counts as one), wav_resample (mp3s_encode_files only).  n >= MP3S_N_KERNELS fills all of them; a caller with room for the first MP3S_N_KERNELS_MIN only
 * (the list as it was before wav_resample joined it at its end) gets those, n below that is MP3S_E_ARG */
#define MP3S_N_KERNELS 9
#define MP3S_N_KERNELS_MIN 8
int mp3s_profile_enable(mp3s_ctx *ctx, int on);
/* An event pair costs a few microseconds of stream time per launch: restrict the timing to the kernels in `mask` (bit k =
 * kernel k in the order above; all by default).  Takes effect with the next mp3s_profile_enable(ctx, 1). */
int mp3s_profile_select(mp3s_ctx *ctx, unsigned mask);
int mp3s_profile_collect(mp3s_ctx *ctx, double *total_ms, int64_t *launches, int n);

/* ---------------------------------------------------------------- (ii) decode transform batch
 * replaces: re_quantize, __ms_stereo, __reorder, __alias_reduction, imdct, __frequency_inversion,
 *           synth_filter_bank, __interleave -- reference decoder/Frame.py:65-218, 561-640 (and the
 *           (pcm*32767).astype(int16) of MP3_Parser.py:91 for MP3S_PCM_I16).
 * is  : int16 [n_frames][2 gr][2 ch][576]   (ch 1 ignored when nch == 1)
 * si  : mp3s_granule_si [n_frames][2][2]
 * hdr : mp3s_frame_hdr [n_frames]
 * pcm : [n_frames - n_halo][1152][nch] of the requested format
 * Frames are consecutive frames of one or more streams; the first n_halo frames only rebuild state
 * (a 1-frame halo is enough).  *_dev takes device pointers and is asynchronous on
 * the context's stream; the host variant uploads, runs, downloads and synchronises. */
int mp3s_decode_transform_dev(mp3s_ctx *ctx, const int16_t *d_is, const mp3s_granule_si *d_si,
                              const mp3s_frame_hdr *d_hdr, int n_frames, int nch, int n_halo, int out_format,
                              void *d_pcm);
int mp3s_decode_transform(mp3s_ctx *ctx, const int16_t *is, const mp3s_granule_si *si, const mp3s_frame_hdr *hdr,
                          int n_frames, int nch, int n_halo, int out_format, void *pcm);

/* ---------------------------------------------------------------- (iii) encode transform batch
 * replaces: __replace_samples, window_filter_sub_band, __mdct_sub (MDCT + alias butterflies)
 *           -- reference encoder/MP3_Encoder.py:321-370, 652-758.
 * pcm  : int16 [n_frames][1152][2] interleaved (stereo only: mono encode raises in the reference)
 * mdct : int32 [n_frames][2 ch][2 gr][576]  (the reference's __mdct_freq layout) */
int mp3s_encode_transform_dev(mp3s_ctx *ctx, const int16_t *d_pcm, const mp3s_frame_hdr *d_hdr, int n_frames,
                              int32_t *d_mdct);
int mp3s_encode_transform(mp3s_ctx *ctx, const int16_t *pcm, const mp3s_frame_hdr *hdr, int n_frames,
                          int32_t *mdct);

/* ---------------------------------------------------------------- (iv) rate-loop batch
 * replaces: __iteration_loop body per granule*channel: xrsq/xrabs/xrmax, __calc_scfsi energies,
 *           __bin_search_step_size, quantize, calc_run_len, count1_bit_count, __subdivide,
 *           __big_v_tab_select/__new_choose_table (+ IDX_TO_TRANSFORM_HUF hide swap), count_bit,
 *           big_v_bit_count, __inner_loop -- reference encoder/MP3_Encoder.py:171-318, 373-449, 760-1095,
 *           1147-1264.
 * Units are indexed u = (frame*2 + ch)*2 + gr, i.e. the reference's processing order (ch outer, gr inner).
 * mdct      : int32 [n_frames][2][2][576]
 * frames    : mp3s_rate_frame [n_frames]
 * hide_bits : n_hide bytes of 0/1 (NULL/0: not hiding); a unit reads hide_bits[i] only for i < min(n_hide,
 *             frames[frame].hide_end), so the messages of several streams can sit back to back in one array
 * cursor_in : int32 [n_units] hide-string index at the start of each unit (ignored when not hiding)
 * state_in  : int32 [n_units][4] address1, address2, address3, quantizerStepSize inherited from the same
 *             (gr,ch) of the previous frame (NULL = zeros)
 * unit_list : optional int32 [n_list] subset of units to (re)compute; NULL = all n_frames*4
 * ix        : int16 [n_frames][2][2][576] signed quantised spectrum (sign from mdct, :1272-1276)
 * out       : mp3s_gr_out [n_units]
 * en        : int32 [n_units][22] __calc_scfsi energies: 21 scalefactor bands + the granule total
 * The serial hide cursor / address chain is resolved by the caller (mp3s_encode_pcm does it):
 * run, prefix-sum n_tables, re-run the units whose assumed inputs were wrong, until none. */
int mp3s_rate_loop_dev(mp3s_ctx *ctx, const int32_t *d_mdct, const mp3s_rate_frame *d_frames, int n_frames,
                       const uint8_t *d_hide_bits, int n_hide, const int32_t *d_cursor_in, const int32_t *d_state_in,
                       const int32_t *d_unit_list, int n_list, int16_t *d_ix, mp3s_gr_out *d_out, int32_t *d_en);

/* ---------------------------------------------------------------- (iv-b) the serial chains of the rate loop, on the device
 * replaces: the two values the reference carries from unit to unit -- __hide_str_offset (reference
 *           encoder/MP3_Encoder.py:808-809, read at :1154-1168) and the address1/2/3 + quantizerStepSize a granule
 *           without big values inherits from the same (gr, ch) of the frame before (:1004-1006, :788-803).
 * mp3s_rate_loop_dev runs every unit on ASSUMED inputs (cursor_in, state_in).  This call scans the batch (segments =
 * streams), compares every unit's assumptions with the true chain, gives silent units the values they inherit (the
 * bit packer writes them into the side info) and leaves one verdict: verdict[0] = number of units that ran on wrong
 * assumptions that mattered (0: d_gr is final, mp3s_pack_frames_dev may run), verdict[1] = 1 if some quantizer step
 * left its table.  The host then reads 8 bytes instead of 72 per unit. */
typedef struct {
    int32_t first_frame, n_frames;   /* the stream's frames in the batch */
    int32_t hide_base;               /* its message is hide[hide_base .. hide_end) of the batch's message array */
    int32_t hide_begin;              /* cursor at its first unit: hide_base + the bits taken by the frames in front of a block */
    int32_t hide_end;
    int32_t reserved;
    int32_t chain_in[4][4];          /* per ch*2+gr: address1..3, quantizerStepSize the frames in front left (zeros: stream start) */
} mp3s_chain_seg; /* 88 bytes */
typedef struct {
    int64_t cursor;                  /* behind the stream's last unit, as an index into the batch's message array */
    int32_t chain[4][4];             /* the four chains as the stream leaves them */
    int32_t carry_used;              /* some unit looked at chain_in / the message was live at the first unit */
    int32_t reserved;
} mp3s_chain_seg_out; /* 80 bytes */
/* d_state_in NULL = zeros (as for mp3s_rate_loop_dev); d_verdict: 2 words; d_seg_out: [n_segs]; both written by the call */
int mp3s_chain_resolve_dev(mp3s_ctx *ctx, mp3s_gr_out *d_gr, const mp3s_rate_frame *d_frames, int n_frames,
                           const mp3s_chain_seg *d_segs, int n_segs, const int32_t *d_cursor_in, const int32_t *d_state_in,
                           int32_t *d_verdict, mp3s_chain_seg_out *d_seg_out);

/* The same check, and what it finds wrong put right on the device where that takes one more run: the units that read
 * inherited addresses other than the chain really holds (the first pass gives every unit zeros: SURVEY E7 -- the first
 * quiet granules behind a silence), or ran on another cursor, are listed on the device, run again on the cursor and
 * addresses the check found (results in place, d_cursor updated for them) and everything is checked once more.  The
 * verdict is the second check's: 0 = final.  What it still finds (a re-run changed what later units inherit, more than
 * 4 096 units listed, a row of inheriting units longer than one re-run follows) is left to the host as before -- or to
 * another call on the same buffers: every re-run records what it was given, so the call may be repeated and goes on
 * where the one before stopped (tests/test_chain_redo.py).  Operands as for mp3s_rate_loop_dev / mp3s_chain_resolve_dev;
 * every unit must have run without d_state_in (the records carry what they were given). */
int mp3s_chain_redo_dev(mp3s_ctx *ctx, const int32_t *d_mdct, const mp3s_rate_frame *d_frames, int n_frames,
                        const uint8_t *d_hide_bits, int n_hide, int32_t *d_cursor, const mp3s_chain_seg *d_segs, int n_segs,
                        int16_t *d_ix, mp3s_gr_out *d_gr, int32_t *d_en, int32_t *d_verdict, mp3s_chain_seg_out *d_seg_out);

/* ---------------------------------------------------------------- (iv-c) the message cursor, decided on the device
 * replaces: the same __hide_str_offset chain (reference encoder/MP3_Encoder.py:808-809, :1154-1168), without guessing:
 *           a unit sees the message only through the <= 3 bits at its cursor (__new_choose_table reads hide_str[offset] once per non-zero table, :1257-1263), so the first
 *           `reach` units of a hiding stream are run once per possibility -- the 8 three-bit patterns, "two bits left",
 *           "one bit left" -- as extra entries of the SAME rate-loop launch, every unit's own run (cursor behind every
 *           message) being the eleventh, and a small kernel walks the chain and copies the entry each unit really sees
 *           into its place.  mp3s_chain_resolve_dev still checks the result; a stream whose message reaches further than
 *           the plan covered fails that check and is resolved by the host as before.  The walk goes in rounds of 1 024
 *           units with the state carried from round to round, so a plan may cover any length of message (r02f; until
 *           then 2 048 units, about 700 message bytes).
 * The message array must start with the 32 pattern bytes of mp3s_select_patterns() (so hide_base >= 32), and d_cursor
 * must hold MP3S_NO_CURSOR for every unit of a planned stream before the call; the call overwrites the cursors of the
 * units it replaced with what they really saw (a later call with the same plan may find those there: they are exact). */
#define MP3S_SELECT_VARIANTS 10
/* The two "bits left" possibilities can only meet the units around the message's end: a unit never takes more than three
 * tables, so unit j's cursor is at most 3j bits behind the start, and "two bits left" needs 3j >= bits_left - 2.  A stream's
 * entries are therefore 8 rows of `reach` units (the patterns) and 2 rows of the units from MP3S_SELECT_TAIL_FIRST on:
 *   entry (v < 8, j) = first_entry + v * reach + j
 *   entry (v >= 8, j >= t) = first_entry + 8 * reach + (v - 8) * (reach - t) + (j - t),  t = MP3S_SELECT_TAIL_FIRST(bits left, reach)
 * with bits left = hide_end - hide_begin of the stream's mp3s_chain_seg. */
#define MP3S_SELECT_TAIL_FIRST(bits_left, reach) ((bits_left) < 2 ? 0 : (((bits_left) - 2) / 3 < (reach) ? ((bits_left) - 2) / 3 : (reach)))
#define MP3S_SELECT_ENTRIES(bits_left, reach) (8 * (reach) + 2 * ((reach) - MP3S_SELECT_TAIL_FIRST(bits_left, reach)))
#define MP3S_SELECT_MAX_REACH (1 << 18)
#define MP3S_NO_CURSOR 0x3fffffff     /* "behind every message": such a unit hides nothing */
typedef struct {
    int32_t first_entry;             /* the stream's first entry (layout: MP3S_SELECT_TAIL_FIRST above) */
    int32_t reach;                   /* its first `reach` units are planned (0: the stream is left to cursor_in as it is) */
} mp3s_select_span; /* 8 bytes */
void mp3s_select_patterns(uint8_t out[32]);
/* host only: spans[n_segs] and the entries (unit, cursor; capacity `cap` each) for the streams of segs.  A stream that does
 * not hide, or whose message could reach more than MP3S_SELECT_MAX_REACH units, or that does not fit into cap any more
 * gets reach 0.  Returns the number of entries. */
int mp3s_select_plan(const mp3s_chain_seg *segs, int n_segs, mp3s_select_span *spans, int32_t *ent_unit, int32_t *ent_cursor, int cap);
/* mp3s_rate_loop_dev over all units of the batch (no inherited state) with the entries behind them in the same launch, then
 * the selection.  d_ixv / d_env: int16 [n_entries][576], int32 [n_entries][22]; d_outv: MP3S_VARIANT_OUT_BYTES(n_entries) --
 * mp3s_gr_out [n_entries] followed by the entries' table counts, one byte each. */
#define MP3S_VARIANT_OUT_BYTES(n) ((size_t)(n) * sizeof(mp3s_gr_out) + (((size_t)(n) + 15) & ~(size_t)15))
int mp3s_rate_select_dev(mp3s_ctx *ctx, const int32_t *d_mdct, const mp3s_rate_frame *d_frames, int n_frames,
                         const uint8_t *d_hide_bits, int n_hide, int32_t *d_cursor, const mp3s_chain_seg *d_segs,
                         const mp3s_select_span *d_spans, int n_segs, int max_reach, const int32_t *d_ent_unit,
                         const int32_t *d_ent_cursor, int n_entries, int16_t *d_ix, mp3s_gr_out *d_out, int32_t *d_en,
                         int16_t *d_ixv, mp3s_gr_out *d_outv, int32_t *d_env);
/* The two halves of mp3s_rate_select_dev on their own, for callers that put the selection (two small launches) on another
 * context's stream than the rate loop -- e.g. with the chain check and the bit packing under the decode transforms of the
 * next batch (bench.py).  The caller orders the streams (mp3s_ctx_wait). */
int mp3s_rate_variants_dev(mp3s_ctx *ctx, const int32_t *d_mdct, const mp3s_rate_frame *d_frames, int n_frames,
                           const uint8_t *d_hide_bits, int n_hide, const int32_t *d_cursor, const int32_t *d_ent_unit,
                           const int32_t *d_ent_cursor, int n_entries, int16_t *d_ix, mp3s_gr_out *d_out, int32_t *d_en,
                           int16_t *d_ixv, mp3s_gr_out *d_outv, int32_t *d_env);
int mp3s_select_dev(mp3s_ctx *ctx, const uint8_t *d_hide_bits, int32_t *d_cursor, const mp3s_chain_seg *d_segs,
                    const mp3s_select_span *d_spans, int n_segs, int max_reach, const int32_t *d_ent_unit,
                    const int32_t *d_ent_cursor, int n_entries, int16_t *d_ix, mp3s_gr_out *d_out, int32_t *d_en,
                    int16_t *d_ixv, mp3s_gr_out *d_outv, int32_t *d_env);

/* ---------------------------------------------------------------- (vi) bit-level stages on the device
 * The serial bit parsing / packing of the reference is serial per granule only: granule boundaries are known from
 * the side info (decode) or from the rate loop (encode), so granules are decoded / packed in parallel.  The host
 * keeps the byte-level framing scan (sync, header, 17/32-byte side info, reservoir gather: mp3s_scan_stream). */

/* side info of one granule*channel as parsed from the stream (reference decoder/FrameSideInformation.py:62-137) */
typedef struct {
    uint16_t part2_3_length, big_values;
    uint8_t global_gain, scalefac_compress, window_switching, block_type, mixed_block_flag;
    uint8_t table_select[3];
    uint8_t region0_count, region1_count, preflag, scalefac_scale, count1table_select;
    uint8_t sub_block_gain[3];
} mp3s_unit_side; /* 20 bytes */

/* one frame for the Huffman kernel: where its main data sits in the blob + the parsed side info
 * flags & MP3S_FS_HOST_DECODED: the kernel skips the frame (the caller places host-decoded samples there afterwards: the
 * last frame of a stream written by the reference's encoder can lack up to 3 bytes of its main data) */
#define MP3S_FS_HOST_DECODED 1
typedef struct {
    uint32_t md_off, md_len;   /* byte offset (multiple of 4) and length of the frame's main data in the blob */
    uint8_t nch, sr_idx, ms_stereo, flags;
    uint8_t scfsi[2][4];
    mp3s_unit_side unit[2][2]; /* [gr][ch] */
    int32_t reserved;          /* index (in the batch) of the first frame of this frame's stream; the scan writes 0.  Negative when the
                                * side array holds records of the stream in FRONT of the batch (mp3s_stream_ref.side_back) */
} mp3s_frame_side; /* 104 bytes */

/* replaces: __unpack_scale_fac + __unpack_samples for every granule*channel of the batch -- reference
 * decoder/Frame.py:365-559 (linear code-book search there, two-level tables here; same prefix codes, same quirks D1/D2).
 * blob: main data of all frames (reservoir already gathered), each frame 4-byte aligned and followed by >= 8 zero
 * bytes; is / si as consumed by mp3s_decode_transform_dev; status: int32, OR of MP3S_HS_* on malformed input.
 * Streams whose scalefactors are inherited across frames (mixed blocks, scfsi behind a short granule 0: SURVEY D10;
 * mp3s_scan_stream reports them with gpu_ok = 0): the kernel walks back through the stream's side records to the granule
 * that wrote the entry last and reads it from that granule's bits, so d_side / d_blob must hold such a stream from its first
 * frame on and frame_side.reserved must name that frame's index relative to d_side[0] (0 for a single stream; negative for a
 * chunk whose predecessors' records lie in front of d_side in one file-wide array: the one-file calls, round 4).  Blocks of
 * such a stream that a rank decodes on its own are parsed on the host. */
#define MP3S_HS_BAD_REGION 1
#define MP3S_HS_BIG_VALUES 2
#define MP3S_HS_HINT 4 /* some part2_3_length exceeds max_part2_3_length: call again with a larger bound (or 0) */
#define MP3S_HS_OVERRUN 8 /* the big values of some granule run past its part2_3_length into the bits that follow: the
                           * reference decodes on (one bit cursor per frame); use mp3s_parse_stream for this stream */
/* max_part2_3_length: an upper bound on part2_3_length over the batch (the scan knows it: mp3s_scanned.max_part2_3_length),
 * or 0 for the format's limit of 4095.  It sizes the per-thread staging of the bit stream in LDS and with it the number of
 * resident wavefronts: 8 per CU for granules up to 900 bits, 2 at the limit. */
int mp3s_huffman_decode_dev(mp3s_ctx *ctx, const uint8_t *d_blob, const mp3s_frame_side *d_side, int n_frames, int nch,
                            int max_part2_3_length, int16_t *d_is, mp3s_granule_si *d_si, int32_t *d_status);

/* ---- the byte-level scan split in two: a walk from header to header on the host, everything else on the device
 * replaces: the same lines as mp3s_scan_stream -- reference decoder/MP3_Parser.py:68-80 and Frame.py:288-316 (the walk: frame
 *           sizes are a recurrence on the headers), decoder/FrameSideInformation.py:39-137 and Frame.py:318-363 (side info
 *           taken apart field by field, main data collected from where the bit reservoir left it: on the device, one
 *           wavefront per frame, from the file image as it is).
 * The walk takes REGULAR streams -- MPEG-1 Layer III frames whose reservoir pointers stay inside the file -- and reports
 * anything else (regular = 0: false syncs parsed as other layers, free-format headers that inherit fields, pointers in front
 * of the file): such a stream goes through mp3s_scan_stream, which follows the reference through every oddity. */
typedef struct {
    uint32_t file_off;         /* offset of the frame header in the byte image the device holds */
    uint32_t md_off;           /* where the frame's main data goes in the blob (multiple of 4) */
    uint16_t md_len;           /* ... and how long it is (reservoir bytes included) */
    uint16_t frame_size;       /* bytes the frame loop steps over (Frame.py:311-316) */
    uint16_t stream;           /* index into the batch's mp3s_stream_ref array */
    uint16_t flags;            /* MP3S_FS_HOST_DECODED: the Huffman kernel leaves the frame alone */
} mp3s_frame_ref; /* 16 bytes */
typedef struct {
    uint32_t base, end;        /* the stream's file image inside the batch's byte image: [base, end); bytes behind `end` read
                                * as zero (reference decoder/util.py:41-43) */
    uint32_t first_frame;      /* its first frame in the batch (mp3s_frame_side.reserved, mp3s_frame_hdr.stream_first) */
    uint32_t n_frames;
    uint16_t prev_size[9];     /* what Frame.__prev_frame_size holds in front of first_frame's gather (SURVEY D11 at a stream's start) */
    uint16_t side_back[2];     /* lo, hi: frames of this stream whose side records and main data lie in FRONT of d_side[first_frame] /
                                * below d_blob's offsets of this batch -- a chunk of a file whose earlier chunks left theirs in one
                                * file-wide array (round 4).  mp3s_frame_side.reserved becomes first_frame - side_back, and the
                                * Huffman kernel's walk for scalefactors inherited across frames goes back that far */
    uint16_t reserved;
} mp3s_stream_ref; /* 40 bytes */
typedef struct {
    int32_t regular;              /* 0: use mp3s_scan_stream for this stream (nothing else below is meaningful) */
    int32_t n_frames, nch, sampling_rate, bit_rate, dup_last_frame;
    int32_t max_part2_3_length;   /* over all granules: the bound mp3s_huffman_decode_dev wants */
    int32_t any_silent;           /* some granule has no code book in use (no big values, or book 0 in all its regions) */
    size_t blob_len;              /* bytes of blob the frames take */
    const mp3s_frame_ref *refs;   /* [n_frames]: file_off counted from the start of the file, md_off from 0, stream 0 */
    mp3s_stream_ref stream;       /* base 0, end = len, first_frame 0 */
    const uint8_t *tables;        /* [n_frames][4]: code books in use per granule in the encoder's unit order (frame, ch, gr); stereo only */
} mp3s_walked;
int mp3s_walk_stream(const uint8_t *file, size_t len, mp3s_buf **owner, mp3s_walked *out);
/* d_image[0] / d_blob[0] are byte image_base / md_base of what the references count in (a chunk of a long file brings its own
 * piece of both); d_tsel optional: per frame the twelve table indices, five bits each in the order the stego bits walk them
 * (channel, granule, region), the four window-switching flags above them -- mp3s_stego_bits turns them into the bits;
 * d_status: one zeroed word, MP3S_PS_* are OR-ed in.  Records as mp3s_scan_stream writes them, except table_select[2] of
 * window-switching granules and sub_block_gain of the others: a granule keeps those from the frame before,
 * nothing on the device reads them, they are zero here. */
#define MP3S_PS_INHERITS 1   /* scalefactors are inherited across frames somewhere (mp3s_scanned.gpu_ok == 0) */
#define MP3S_PS_MISMATCH 2   /* a frame's main data came out another length than its reference says */
int mp3s_parse_frames_dev(mp3s_ctx *ctx, const uint8_t *d_image, uint32_t image_base, const mp3s_frame_ref *d_refs,
                          const mp3s_stream_ref *d_streams, int n_frames, uint32_t md_base, mp3s_frame_side *d_side,
                          mp3s_frame_hdr *d_hdr, uint8_t *d_blob, uint64_t *d_tsel, int32_t *d_status);
/* replaces: __get_frame_huffman_tables + bit_from_huffman_tables -- reference decoder/Frame.py:676-685, decoder/util.py:67-81.
 * carry[4]: the third table index each (channel, granule) was left with by the frames in front (zeros at a stream's start), updated */
int mp3s_stego_bits(const uint64_t *tsel, int64_t n_frames, int nch, uint8_t carry[4], mp3s_buf **owner, const uint8_t **bits, size_t *n_bits);
/* The stego bits of a batch of walked streams in ONE launch (k_reveal: one workgroup per stream, one frame per thread, the frames of
 * a stream in tiles of MP3S_REVEAL_TILE) -- the reveal of a file needs nothing else of it.
 * replaces: __get_frame_huffman_tables + bit_from_huffman_tables for every frame of every stream -- reference decoder/Frame.py:676-685,
 *           decoder/util.py:67-81, with the index a window-switching granule keeps from the granule before it resolved on
 *           the device (a scan along the stream that restarts at every stream); no main data is read.
 * d_image / image_base / d_refs / d_streams as for mp3s_parse_frames_dev (base, end, first_frame, n_frames of a stream reference mean
 * what they mean there; d_refs[f].stream is the stream's index in d_streams), n_streams <= 65 535.  Stream s gets its bits packed
 * eight to a byte, MSB first, the last byte zero-padded, from byte d_out_off[s] of d_packed (a multiple of 4; whole dwords are written:
 * room for 4 * ceil(12 * n_frames / 32) bytes there), their count in d_n_bits[s] and d_status[s] = 0, or MP3S_RV_BAD_REF when one of
 * its frame references names another stream or a place outside [base, end): nothing is read there and the bits are not to be used. */
#define MP3S_REVEAL_TILE 256
#define MP3S_RV_BAD_REF 1
int mp3s_reveal_bits_dev(mp3s_ctx *ctx, const uint8_t *d_image, uint32_t image_base, const mp3s_frame_ref *d_refs,
                         const mp3s_stream_ref *d_streams, int n_streams, const uint32_t *d_out_off, uint8_t *d_packed,
                         int32_t *d_n_bits, int32_t *d_status);

/* replaces: __format_bitstream for every frame of the batch -- reference encoder/MP3_Encoder.py:1097-1145 (stuffing),
 * 1266-1547; one workgroup per frame, one wavefront per granule*channel, code lengths prefix-summed across lanes.
 * gr must be final (serial chain resolved, silent units carrying their inherited quantizer_step); en as written by
 * the rate loop (scfsi is decided here, :861-892); frame_off[f] = byte offset of frame f, padding[f] its padding bit.
 * Output bytes [frame_off[n_frames]]; the caller truncates the stream to a multiple of 4 bytes (E14). */
int mp3s_pack_frames_dev(mp3s_ctx *ctx, const int16_t *d_ix, const mp3s_gr_out *d_gr, const int32_t *d_en, int n_frames,
                         int samplerate, int bitrate_kbps, const uint32_t *d_frame_off, const uint8_t *d_padding,
                         uint8_t *d_mp3, int32_t *d_scfsi, int32_t *d_status);

/* ---------------------------------------------------------------- host stages (no GPU needed) */

/* replaces: the byte-level part of MP3Parser.parse_file: sync/header/side-info parse, frame sizes, reservoir gather,
 * stego bits -- reference decoder/MP3_Parser.py:25-85, Frame.py:244-263, 288-363, 676-685, FrameHeader.py,
 * FrameSideInformation.py.  No scalefactor / Huffman decoding (that is mp3s_huffman_decode_dev or mp3s_parse_stream). */
typedef struct {
    int32_t n_frames, nch, sampling_rate, bit_rate, n_bits, dup_last_frame;
    int32_t gpu_ok;               /* 0: scalefactors are inherited across frames somewhere -> use mp3s_parse_stream */
    int32_t max_part2_3_length;   /* over all granules: the bound mp3s_huffman_decode_dev wants */
    const mp3s_frame_side *side;  /* [n_frames] */
    const mp3s_frame_hdr *hdr;    /* [n_frames] */
    const uint8_t *blob;          /* main data of all frames */
    size_t blob_len;
    const uint8_t *bits;          /* stego bits 0/1 */
    const int32_t *frame_size;    /* [n_frames] */
} mp3s_scanned;
int mp3s_scan_stream(const uint8_t *file, size_t len, mp3s_buf **owner, mp3s_scanned *out);

void mp3s_buf_free(mp3s_buf *b);

/* replaces: MP3Parser.parse_file front end: header/side-info parse, reservoir reassembly, scalefactor
 * and Huffman decode, stego bit extraction -- reference decoder/MP3_Parser.py:25-85, Frame.py:244-263,
 * 288-559, 676-685, FrameHeader.py, FrameSideInformation.py, util.py:22-81, ID3 skip (ID3_Parser.py:95-131). */
typedef struct {
    int32_t n_frames, nch, sampling_rate, bit_rate; /* rate/bitrate of the LAST header */
    int32_t n_bits;          /* stego bits */
    int32_t dup_last_frame;  /* reference appends the last PCM frame once more after a bad header (D12) */
    const int16_t *is;       /* [n_frames][2][2][576] */
    const mp3s_granule_si *si;
    const mp3s_frame_hdr *hdr;
    const uint8_t *bits;     /* 0/1 */
    const int32_t *table_select; /* [n_frames][2 gr][2 ch][3] as parsed (for tests) */
    const int32_t *frame_size;   /* [n_frames] */
} mp3s_parsed;
int mp3s_parse_stream(const uint8_t *file, size_t len, mp3s_buf **owner, mp3s_parsed *out);

/* replaces: Encoder back end: padding/slot-lag replay, __resv_frame_end, __format_bitstream and the
 * 32-bit cache writer -- reference encoder/MP3_Encoder.py:623-636, 1097-1145, 1266-1552.
 * ix/gr/scfsi as produced by the rate loop for n_frames stereo frames. */
int mp3s_format_stream(int samplerate, int bitrate_kbps, int n_frames, const int16_t *ix, const mp3s_gr_out *gr,
                       const int32_t *scfsi /*[n_frames][2][4]*/, mp3s_buf **owner, const uint8_t **mp3, size_t *mp3_len);
/* per-frame padding / max_bits replay (reference MP3_Encoder.py:630-636, 894-912) */
int mp3s_rate_frames(int samplerate, int bitrate_kbps, int nch, int n_frames, mp3s_rate_frame *out, int32_t *padding);

/* ---------------------------------------------------------------- (v) whole-stream conveniences */
/* replaces: Decoder.decode up to (not including) the WAV write -- reference decoder/decoder.py:59-84 */
typedef struct {
    int32_t n_frames, nch, sampling_rate, bit_rate, n_bits;
    int64_t n_rows;      /* PCM rows = 1152 * (n_frames + dup_last_frame) */
    const void *pcm;     /* [n_rows][nch] in out_format */
    const uint8_t *bits; /* stego bits 0/1 */
} mp3s_decoded;
int mp3s_decode_stream(mp3s_ctx *ctx, const uint8_t *file, size_t len, int out_format, mp3s_buf **owner,
                       mp3s_decoded *out);
/* many streams in one call: the frames of all files form one batch (stream_first marks the starts), so
 * a corpus of short files costs one Huffman launch and one transform launch per channel count instead of one per file.
 * out[i] describes file i; every pointer lives in *owner.  status[i] = MP3S_OK or the code file i alone would have
 * failed with (its out[i] is zeroed, the other files are unaffected); with status == NULL the first such file fails the
 * whole call (its index is in mp3s_last_error()) -- the same rule as mp3s_hide_messages. */
int mp3s_decode_streams(mp3s_ctx *ctx, const uint8_t *const *files, const size_t *lens, int n_files, int out_format,
                        mp3s_buf **owner, mp3s_decoded *out, int32_t *status);

/* Frames [first_frame, first_frame + n_frames) of the stream (clipped to its end) -- the decode half of sharding one
 * stream over several GPUs.  The whole file is scanned on the host; only the block's main data plus one frame
 * in front of it goes to the device (IMDCT overlap and synthesis fifo reach back less than a frame: reference
 * decoder/Frame.py:151-153, 81-92).  Concatenating the blocks' PCM gives mp3s_decode_stream's.  n_frames / n_rows
 * describe the block; bits / bit_rate / sampling_rate the whole stream. */
int mp3s_decode_block(mp3s_ctx *ctx, const uint8_t *file, size_t len, int64_t first_frame, int64_t n_frames, int out_format,
                      mp3s_buf **owner, mp3s_decoded *out);

/* Index of a stream: ONE walk over its frames (headers, side info, reservoir pointers; no main data is copied) that leaves
 * a resume point every 256 frames.  With it a block of the stream is scanned on its own -- the ranks of a sharded stream
 * and the chunks of a streamed file pay for their own frames (plus at most 255 skipped ones), not for the whole file again
 * (reference: none -- it reads the whole file into memory, decoder/decoder.py:26-27, and loops over it once,
 * decoder/MP3_Parser.py:68-80).  The index is plain host data, bound to the file bytes it was made from. */
typedef struct mp3s_index mp3s_index;
typedef struct {
    int64_t n_frames;
    int32_t nch, sampling_rate, bit_rate;   /* of the LAST frame header, as mp3s_scan_stream reports them */
    int32_t dup_last_frame;
    int32_t gpu_ok;                         /* 0: a stream the host parser has to take (mp3s_scanned.gpu_ok): block calls then scan the whole file */
    int32_t reserved;
} mp3s_index_info;
int mp3s_index_stream(const uint8_t *file, size_t len, mp3s_index **index, mp3s_index_info *info);
void mp3s_index_free(mp3s_index *index);
/* mp3s_scan_stream for frames [first_frame, first_frame + n_frames) only (clipped to the stream): side records, main-data
 * blob, headers, frame sizes and the stego bits OF THESE FRAMES, identical to the corresponding part of the full scan */
int mp3s_scan_range(const uint8_t *file, size_t len, const mp3s_index *index, int64_t first_frame, int64_t n_frames, mp3s_buf **owner,
                    mp3s_scanned *out);
/* mp3s_decode_block with the block scanned on its own; out->bits / n_bits then describe the block's frames (the halo frame in
 * front included), not the whole stream.  index == NULL: exactly mp3s_decode_block. */
int mp3s_decode_block_indexed(mp3s_ctx *ctx, const uint8_t *file, size_t len, const mp3s_index *index, int64_t first_frame,
                              int64_t n_frames, int out_format, mp3s_buf **owner, mp3s_decoded *out);

/* replaces: Encoder.encode -- reference encoder/encoder.py:33-58, MP3_Encoder.py:596-618 */
typedef struct {
    int32_t n_frames;
    int32_t too_long;      /* hide_str_offset < len(hide_str) - 1 (encoder.py:50) */
    int64_t hide_offset;
    const uint8_t *mp3;
    size_t mp3_len;
    const mp3s_gr_out *gr; /* [n_frames*4] unit order (frame, ch, gr) */
    const int32_t *scfsi;  /* [n_frames][2][4] */
    int32_t rate_passes;   /* launches of the rate loop needed to resolve the serial chain */
} mp3s_encoded;
int mp3s_encode_pcm(mp3s_ctx *ctx, const int16_t *pcm, int64_t n_samples_per_ch, int nch, int samplerate,
                    int bitrate_kbps, const uint8_t *hide_bits, int n_hide, mp3s_buf **owner, mp3s_encoded *out);

/* One contiguous block of a longer stream, for a stream sharded over several GPUs.  What crosses a block
 * boundary in the reference encoder: < 1 frame of filter-bank / MDCT history (MP3_Encoder.py:356,685,747: `lead_frames`
 * = 1 frame of PCM in front of the block is transformed and dropped), the padding recurrence (:630-636: restarted from
 * frame 0 by `first_frame`), and two serial chains, passed explicitly: */
typedef struct {
    int64_t cursor;        /* message bits consumed by the frames in front of the block (MP3_Encoder.py:808-809) */
    int32_t chain[4][4];   /* per ch*2+gr: address1, address2, address3, quantizerStepSize as the frame in front left
                            * them (they are only re-written by granules that carry data: SURVEY E7) */
} mp3s_carry;
/* pcm        : int16 [(lead_frames + n) * 1152][2], n = the block's own frames; stereo only
 * first_frame: index of the block's first own frame in the stream;  last_block: the stream ends with this block
 * hide_bits  : the WHOLE message (cursors are absolute);  carry_in NULL = the block starts the stream
 * carry_out  : what the next block needs;  *carry_used = the block's bytes depend on carry_in (a caller that ran the
 *              block on a guessed carry_in re-runs it only if this is set and the guess was wrong)
 * out        : mp3 = the block's frames (concatenating the blocks gives the stream mp3s_encode_pcm produces),
 *              hide_offset counts from the start of the stream; too_long is meaningful for the last block */
int mp3s_encode_block(mp3s_ctx *ctx, const int16_t *pcm, int64_t n_samples_per_ch, int lead_frames, int64_t first_frame,
                      int last_block, int samplerate, int bitrate_kbps, const uint8_t *hide_bits, int n_hide,
                      const mp3s_carry *carry_in, mp3s_carry *carry_out, int32_t *carry_used, mp3s_buf **owner,
                      mp3s_encoded *out);

/* ---------------------------------------------------------------- (vi) files and messages */
/* Whole files as byte strings in, byte strings out: WAV and MP3 containers, message framing and the facade's three
 * operations inside the library, so that a binding in any language needs no code of its own for them.  Nothing here
 * touches the disk.  MP3S_E_EXIT = the reference would sys.exit(text); MP3S_E_UNSUPPORTED / MP3S_E_MALFORMED = it would
 * raise (IndexError / struct.error ...). */

/* replaces: WavReader.__read_header + check_bitrate_index -- reference encoder/WAV_Reader.py:30-111 */
typedef struct {
    int32_t channels, samplerate, bits_per_sample, bitrate;
    int64_t num_of_samples; /* per channel, from the data chunk size (float arithmetic as in the reference) */
    int64_t data_offset;    /* byte offset of the first sample */
    int64_t n_values;       /* int16 values the reference's np.fromfile call yields (up to 2x the declared count) */
} mp3s_wav_info;
int mp3s_wav_parse(const uint8_t *file, size_t len, int bitrate_kbps, mp3s_wav_info *out);
/* The opt-in reader (MP3S_OPT_WAV_IMPORT): what a WAV file is to the encode calls when the option is on.  No device, no context.
 *  - RIFF chunk walk from byte 12 over the whole file: id, little-endian size, payload, pad byte after an odd size (a zero byte; where
 *    a writer left it out -- the byte there is not zero -- the next chunk starts at once: the files the strict reader takes with an odd
 *    chunk and no pad byte stay readable, and the samples may lie at an ODD offset).  The first "fmt "
 *    and the first "data" count and "fmt " must come first; a chunk header cut by the end of the file ends the walk.  No RIFF/WAVE,
 *    no "fmt ", no "data": MP3S_E_EXIT "Bad WAVE file.".
 *  - "fmt " of 16, 18 or 40 bytes.  Tag 1 (PCM) with 8, 16, 24 or 32 bits, tag 3 (IEEE float) with 32 bits; tag 0xFFFE (extensible,
 *    40 bytes) takes the tag from the first two bytes of the sub-format GUID and the sample width from the container (wBitsPerSample)
 *    whatever wValidBitsPerSample says: valid bits are left-justified in the container.  block_align is computed (channels x bytes), the
 *    field in the file is not trusted.  Anything else: MP3S_E_EXIT with the reference's "compression used instead of PCM" / "samples
 *    not int8, int16 or int32 type" text (64-bit float: the latter).
 *  - 1 or 2 channels; 0 is MP3S_E_MALFORMED, more than 2 MP3S_E_UNSUPPORTED.  32 000 / 44 100 / 48 000 Hz and the bitrate table as
 *    for mp3s_wav_parse, same texts; files of other rates are resampled to one of the three under MP3S_OPT_WAV_RESAMPLE only
 *    (mp3s_wav_resample_info states the rules).
 *  - data bytes = min(declared size, bytes left in the file); a declared size of 0 or 0xFFFFFFFF means "to the end of the file".
 *    n_samples = data bytes / block_align (a cut last sample is dropped); none: MP3S_E_UNSUPPORTED "no samples".  Bytes behind the
 *    samples are never audio.
 *  - samples to int16 (little-endian input, no dither, no rounding for the integer formats): 8-bit unsigned (u - 128) << 8; 16-bit as
 *    is; 24-bit s >> 8 and 32-bit s >> 16 (arithmetic: the upper two bytes); float32 clamp(rint(x * 32768.0f), -32768, 32767),
 *    round-half-even, all in float32, NaN gives 0.
 *  - mono: the sample goes to BOTH channels.  The encoder is stereo-only, so a mono file becomes a stereo MP3 at the requested
 *    bitrate and mp3s_file.channels is 2.
 *  - the last frame is filled with zeros from sample n_samples on.
 * A 16-bit stereo file of whole frames that mp3s_wav_parse accepts gives the same bytes and fields with the option on as with it off. */
#define MP3S_WAV_U8 1
#define MP3S_WAV_S16 2
#define MP3S_WAV_S24 3
#define MP3S_WAV_S32 4
#define MP3S_WAV_F32 5
typedef struct {
    int32_t format;          /* MP3S_WAV_U8, _S16, _S24, _S32, _F32 */
    int32_t channels;        /* 1 or 2 */
    int32_t samplerate, bits_per_sample, block_align, bitrate;
    int64_t data_offset;     /* first sample byte, any alignment */
    int64_t n_samples;       /* per channel: data bytes present in the file / block_align */
    int64_t n_frames;        /* ceil(n_samples / 1152) */
} mp3s_wav_import;
int mp3s_wav_import_info(const uint8_t *file, size_t len, int bitrate_kbps, mp3s_wav_import *out);
/* The resampler of MP3S_OPT_WAV_RESAMPLE: what a WAV file of any sampling rate is to the encode calls.  No device, no context.  `mode` takes
 * the option's non-zero values (1 / 32000 / 44100 / 48000; anything else MP3S_E_ARG).  Everything but the rate is judged by the rules
 * of mp3s_wav_import_info, same codes and texts; the bitrate is checked against out_rate.  An extension beyond the reference.
 *  - target rate.  Forced mode: `mode`.  Auto (1): a supported rate stays; otherwise the candidates are the supported rates >= the
 *    file's rate (all three if it is above 48 000), the one with the smallest L wins, ties go to the highest rate:
 *    8000 -> 32000, 11025 -> 44100, 16000 -> 32000, 22050 -> 44100, 24000 -> 48000, 37800 -> 44100, 88200 -> 44100, 96000 -> 48000.
 *  - ratio.  g = gcd(in, out), L = out / g, M = in / g.  L > 1280, more than 256 taps or a rate of 0: MP3S_E_EXIT "Unsupported
 *    sampling frequency.".  L = M = 1: the file is not resampled and takes the path of MP3S_OPT_WAV_IMPORT.
 *  - filter.  rho = min(1, L / M), H = ceil(16 / rho), T = 2 H taps per phase.  Prototype h(t) = 0.95 rho sinc(0.95 rho t) w(t / H), t in
 *    input samples, sinc(x) = sin(pi x) / (pi x), w the 4-term Blackman-Harris window 0.35875 + 0.48829 cos(pi u) + 0.14128 cos(2 pi u)
 *    + 0.01168 cos(3 pi u) on (-1, 1], zero outside.
 *  - positions.  Output sample n sits at x = n M / L: i0 = floor(n M / L), p = n M mod L.  Tap k (0 <= k < T) multiplies input sample
 *    i0 - H + 1 + k; its t is k - H + 1 - p / L.
 *  - coefficients.  c[p][k] = rint(h(t) 2^15) in double; the residual 32768 - sum_k c[p][k] is added to the phase's largest tap (the
 *    first of equal ones), so DC gain is exactly 1.  sum_k |c[p][k]| of a phase exceeds 65535 (69 292 for L / M = 2 / 1), so ONE int32 sum
 *    could overflow on full-scale input: the device adds the taps k < 2 floor(H / 2) and the taps behind them apart and joins the two
 *    sums in 64 bits.  No table where sum |c| of either part exceeds 65535: 65535 x 32768 + 2^14 < 2^31, each part fits int32.
 *  - output.  y[n] = clamp((sum_k c[p][k] x[i0 - H + 1 + k] + 2^14) >> 15, -32768, 32767), arithmetic shift, x = 0 outside [0, n_in),
 *    n = 0 .. n_out - 1 with n_out = ceil(n_in L / M); the rest of the last frame is zero.  x is the int16 the import rules make of the
 *    file's sample; a mono file is computed once and written to both channels.
 * mp3s_file.sampling_rate of a result is out_rate, channels 2. */
typedef struct {
    mp3s_wav_import in;        /* as mp3s_wav_import_info, but samplerate = the file's own rate, n_samples / n_frames of the INPUT */
    int32_t out_rate, L, M;    /* out_rate / in_rate = L / M in lowest terms; L = M = 1: not resampled */
    int32_t taps, half;        /* T = 2 H taps per phase, H */
    int64_t n_out, n_frames;   /* ceil(n_in * L / M); ceil(n_out / 1152) */
} mp3s_wav_resample;
int mp3s_wav_resample_info(const uint8_t *file, size_t len, int bitrate_kbps, int mode, mp3s_wav_resample *out);
/* the integer tap table the device uses for the ratio L / M: taps[L][T], *T = taps per phase; cap = room in int32 values (MP3S_E_ARG with
 * *T set when it is too small, or for a ratio the resampler refuses) */
int mp3s_wav_resample_taps(int L, int M, int32_t *taps /* [L][T] */, int cap, int32_t *T);
/* replaces: scipy.io.wavfile.write header as used by MP3_Parser.write_to_wav -- reference decoder/MP3_Parser.py:86-93 */
int mp3s_wav_header(int64_t n_rows, int nch, int rate, uint8_t out44[44]);
/* replaces: str_to_binary_str(str(len(m)) + "#" + m) -- reference steganography.py:10-24, 42-50.  bits are 0/1 bytes. */
int mp3s_message_frame(const uint8_t *utf8, size_t n, mp3s_buf **owner, const uint8_t **bits, size_t *n_bits);
/* replaces: the reveal parse -- reference decoder/decoder.py:90-108.  text is what the reference writes to the .txt. */
int mp3s_message_reveal(const uint8_t *bits, size_t n_bits, mp3s_buf **owner, const uint8_t **text, size_t *n_text);

typedef struct {
    const uint8_t *data;  /* the produced file: WAV, MP3 or revealed text */
    size_t len;
    int32_t kbps;         /* bitrate of the last frame header / 1000 (decoder.py:110); the bitrate used when encoding */
    int32_t sampling_rate, channels, n_frames;
    int32_t too_long;     /* encode/hide: the message did not fit and was trimmed (encoder.py:50) */
    int32_t n_bits;       /* decode: stego bits found in the stream */
    int64_t hide_offset;  /* encode/hide: message bits consumed */
    const uint8_t *bits;  /* decode: the stego bits, 0/1 */
} mp3s_file;
/* replaces: Decoder(...).decode() -- reference decoder/decoder.py:59-84: MP3 bytes -> WAV bytes (int16) */
int mp3s_decode_file(mp3s_ctx *ctx, const uint8_t *mp3, size_t len, mp3s_buf **owner, mp3s_file *out);
/* the same with the WAV written to an open file (decoder/decoder.py:80-84 ends in scipy.io.wavfile.write(output_file_path, ...)): bytes
 * [0, out->len) of `fd` (pwrite), cut to that length; the PCM of a file that goes through the stages as chunks is written chunk by chunk
 * while the later chunks are on the device (same rule as mp3s_hide_message_fd for a file that held something).  out->data is NULL, out->bits
 * lives in *owner. */
int mp3s_decode_file_fd(mp3s_ctx *ctx, const uint8_t *mp3, size_t len, int fd, mp3s_buf **owner, mp3s_file *out);
/* replaces: Encoder(...).encode() -- reference encoder/encoder.py:21-58: WAV bytes -> MP3 bytes, hide_bits optional */
int mp3s_encode_file(mp3s_ctx *ctx, const uint8_t *wav, size_t len, int bitrate_kbps, const uint8_t *hide_bits,
                     int n_hide, mp3s_buf **owner, mp3s_file *out);
/* replaces: Steganography.hide_message / clear_file -- reference steganography.py:133-182: decode, then re-encode at
 * the stream's own bitrate with (hide) or without (clear) "<count>#<message>".  The int16 PCM never leaves HBM between
 * the two halves; the result is byte-identical to going through the temporary WAV file. */
int mp3s_hide_message(mp3s_ctx *ctx, const uint8_t *mp3, size_t len, const uint8_t *utf8, size_t n_msg, mp3s_buf **owner,
                      mp3s_file *out);
int mp3s_clear_file(mp3s_ctx *ctx, const uint8_t *mp3, size_t len, mp3s_buf **owner, mp3s_file *out);
/* The same two calls with the result written to an open file instead of handed back (the reference's hide_message / clear_file write
 * a file: steganography.py:137-162, 164-182 -- the last step of both is Encoder(...).encode() writing output_file_path,
 * encoder/encoder.py:53-57): bytes [0, out->len) of `fd` are the result (pwrite: the descriptor's position is not used or moved), the
 * file is cut to that length at the end; out->data is NULL.  A file that goes through the stages as chunks is written chunk by chunk, a
 * chunk's bytes while the chunks behind it are on the device -- if the file was EMPTY when the call began; a file that held something is
 * written at the end of a call that succeeded and is left as it was by one that did not (the reference has not touched its output when it
 * refuses a stream; whoever created an empty file for the call removes it after an error). */
int mp3s_hide_message_fd(mp3s_ctx *ctx, const uint8_t *mp3, size_t len, const uint8_t *utf8, size_t n_msg, int fd, mp3s_file *out);
int mp3s_clear_file_fd(mp3s_ctx *ctx, const uint8_t *mp3, size_t len, int fd, mp3s_file *out);
/* replaces: a loop of Steganography.hide_message / clear_file over a list of files.  All files with the
 * same sampling rate and bitrate go through the device as ONE batch (decode, transforms, rate loop, bit packing: the
 * streams' frames back to back, every serial chain restarting at a stream's first frame), so many short files cost
 * about what one long file of the same total length costs.  msgs[i] = UTF-8 message of file i, NULL = clear that file
 * (msgs itself NULL = clear all).  out[i] is byte-identical to what mp3s_hide_message / mp3s_clear_file give for file i
 * alone.  status[i] = MP3S_OK or the code file i alone would have failed with (its out[i] is zeroed); with status ==
 * NULL the first such code fails the whole call.  Either way mp3s_last_error() holds the text of the FIRST failing file.
 * This is the rule of every call that takes a list of files. */
int mp3s_hide_messages(mp3s_ctx *ctx, const uint8_t *const *mp3s, const size_t *lens, int n_files, const uint8_t *const *msgs,
                       const size_t *msg_lens, mp3s_buf **owner, mp3s_file *out, int32_t *status);
/* replaces: a loop of Encoder(...).encode() over a list of WAV files -- reference encoder/encoder.py:21-58 (WAV_Reader.py:30-111 for
 * each header, MP3_Encoder.py:596-618 for the frame loop).  All files with the same sampling rate and bitrate go through the
 * device as ONE batch: one upload of the WAV images as the caller holds them (no host copy of the samples; a data chunk at an odd
 * offset is put right on the device, k_wav_gather), transforms, rate loop with the message variants, chain check, bit packing, one
 * download -- many short files cost about what one long file of the same total length costs.  bitrate_kbps[i] = bitrate of file
 * i; hide_bits[i] / n_hide[i] = its message as 0/1 bytes, as for mp3s_encode_file (hide_bits NULL = nothing hidden anywhere).
 * out[i] is byte for byte and field for field what mp3s_encode_file gives for file i alone.  status[i] = MP3S_OK or the code file
 * i alone would have failed with (MP3S_E_EXIT with the reference's text for a rate or bitrate it refuses, MP3S_E_UNSUPPORTED for
 * mono and for a file that ends inside its last frame, MP3S_E_ARG), its out[i] zeroed; with status == NULL the first such code
 * fails the whole call -- the same rule as mp3s_hide_messages.
 * With MP3S_OPT_WAV_IMPORT the files are read by the rules of mp3s_wav_import_info instead (its codes and texts per file): mono or
 * stereo, 8/16/24/32-bit PCM or float32, any chunk layout, any length.  16-bit stereo files of whole frames still go through
 * k_wav_gather; everything else of a batch is converted to the int16 stereo frames of the same PCM buffer by ONE k_wav_import launch
 * (mono to both channels, the last frame zero-filled; the result is a stereo MP3, channels = 2).  Behind the PCM buffer nothing differs. */
int mp3s_encode_files(mp3s_ctx *ctx, const uint8_t *const *wavs, const size_t *lens, int n_files, const int32_t *bitrate_kbps,
                      const uint8_t *const *hide_bits, const int32_t *n_hide, mp3s_buf **owner, mp3s_file *out, int32_t *status);
/* test aid: the first device step of mp3s_encode_files alone -- the images of these WAV files (stereo, any supported rate; with
 * MP3S_OPT_WAV_IMPORT whatever mp3s_wav_import_info accepts, through k_wav_import) go up and
 * k_wav_gather lays their frames back to back; pcm = room for cap_frames frames of [1152][2] int16, *n_frames = the frames of all files
 * (np.fromfile + the frame slicing of reference encoder/WAV_Reader.py:108, MP3_Encoder.py:596-618, the over-read frame of E3 included) */
int mp3s_debug_wav_gather(mp3s_ctx *ctx, const uint8_t *const *wavs, const size_t *lens, int n_files, int16_t *pcm, int64_t cap_frames,
                          int64_t *n_frames);
/* The share of one rank in hiding a message in (utf8 != NULL) or clearing (NULL) ONE stream that is spread over `world`
 * ranks: the stream's PCM frames (repeated last frame included) are cut into `world` contiguous blocks, sizes
 * differing by at most one; this call decodes block `rank` -- one frame of decoder state and one frame of PCM in front of
 * it -- and re-encodes it without the PCM leaving HBM: mp3s_decode_block + mp3s_encode_block in one, with one host scan.
 * carry_in NULL is only valid for rank 0; the other ranks pass the carry_out of the rank before them -- or a guess, and
 * call again with the real one if carry_used says the block depended on it (see mp3s_encode_block).  file.data = the
 * block's frames; concatenated over the ranks they are the file mp3s_hide_message / mp3s_clear_file produce.  A rank
 * beyond the last frame gets n_frames = 0 and no data. */
typedef struct {
    int64_t total_frames, first_frame, n_frames; /* of the stream / of this rank's block */
    int32_t is_last, carry_used;
    mp3s_carry carry_out;
    mp3s_file file;                              /* too_long / hide_offset count from the start of the stream */
} mp3s_block;
int mp3s_reencode_block(mp3s_ctx *ctx, const uint8_t *mp3, size_t len, const uint8_t *utf8, size_t n_msg, int rank, int world,
                        const mp3s_carry *carry_in, mp3s_buf **owner, mp3s_block *out);
/* mp3s_reencode_block with the block scanned on its own (index == NULL: exactly mp3s_reencode_block) */
int mp3s_reencode_block_indexed(mp3s_ctx *ctx, const uint8_t *mp3, size_t len, const mp3s_index *index, const uint8_t *utf8, size_t n_msg,
                                int rank, int world, const mp3s_carry *carry_in, mp3s_buf **owner, mp3s_block *out);
/* mp3s_hide_message (utf8 != NULL) / mp3s_clear_file (NULL) on a file of any length in chunks of at most chunk_frames frames:
 * one index walk, then chunk after chunk through the device, each scanned on its own and run on the real carry of the one in
 * front of it (streaming for files larger than the device / page-locked buffers should take at once).  The
 * device and staging memory in use is that of one chunk; the result is byte-identical to the one-call functions. */
int mp3s_hide_message_chunked(mp3s_ctx *ctx, const uint8_t *mp3, size_t len, const uint8_t *utf8, size_t n_msg, int64_t chunk_frames,
                              mp3s_buf **owner, mp3s_file *out);
/* replaces: Steganography.reveal_massage -- reference steganography.py:103-131: MP3 bytes -> message text.  Only the
 * byte-level scan runs (table_select lives in the side info), so no device work and no context are needed.
 * More lenient than the reference in one respect: reveal_massage decodes every frame before it looks at the bits, so a
 * stream whose main data makes that decode raise (big_values > 288, region counts past the band table, ragged channel
 * counts are caught here too, Huffman-level damage is not) raises there and yields a message here.  The Python facade is
 * unaffected (Steganography.reveal_massage goes through mp3s_decode_file). */
int mp3s_reveal_message(const uint8_t *mp3, size_t len, mp3s_buf **owner, mp3s_file *out);
/* replaces: a loop of Steganography.reveal_massage over a list of files -- the counterpart of mp3s_hide_messages.  The files are
 * walked from header to header on the context's scan threads (MP3S_OPT_SCAN_THREADS); the ones the walk calls regular (mp3s_walk_stream)
 * go through the device as ONE batch whatever their sampling rates, bitrates and channel counts are -- nothing in the kernel depends on
 * them, unlike hide and encode: one upload of the file images as the caller holds them, k_reveal (mp3s_reveal_bits_dev), one download
 * of the packed bits and their counts.  (A list of more than 65 535 such files, or of 4 GiB of them, takes a launch per part: a frame
 * reference names its stream in 16 bits and its place in 32.)  Every other file -- irregular streams, files without a sync, empty
 * files -- is served by the byte-level scan on the host, into the same out[i].
 * out[i] of every file mp3s_scan_stream accepts is what mp3s_reveal_message returns for that file: data / len = mp3s_message_reveal
 * of the scan's bits, n_bits, bits (0/1 bytes, expanded on the host from the packed result), kbps, sampling_rate, channels, n_frames.
 * status[i] = MP3S_OK or the code mp3s_scan_stream fails with for file i (its out[i] is zeroed; MP3S_E_ARG for a null file); with
 * status == NULL the first such code fails the whole call -- the rule of mp3s_hide_messages.
 * The leniency of mp3s_reveal_message holds here as well: no main data is decoded, so a file whose Huffman data is damaged but whose
 * framing is sound yields its message, where the reference (and the facade, through mp3s_decode_file) refuses it. */
int mp3s_reveal_messages(mp3s_ctx *ctx, const uint8_t *const *mp3s, const size_t *lens, int n_files, mp3s_buf **owner, mp3s_file *out,
                         int32_t *status);
/* test aid: mp3s_reveal_messages with at most max_streams (1 .. 65 535) streams to a launch -- a short list in several launches */
int mp3s_debug_reveal_messages(mp3s_ctx *ctx, const uint8_t *const *mp3s, const size_t *lens, int n_files, int max_streams,
                               mp3s_buf **owner, mp3s_file *out, int32_t *status);

/* ---------------------------------------------------------------- (vi-b) how much fits: message capacity of MP3 and WAV files
 * replaces: hiding something and looking at too_long.  The message cursor of the reference (__hide_str_offset, reference
 *           encoder/MP3_Encoder.py:808-809, read at :1154-1168) advances by the number of non-zero table_select of every unit whose
 *           xrmax != 0; how far it gets over a stream is how many message bits the stream takes.
 * What capacity means here:
 *   bits        the sum of mp3s_gr_out.n_tables over the stream's units with MP3S_RF_ACTIVE, after the chain check has made the records
 *               final (what k_chain.hpp sums for hiding streams): the message bits the re-encode this call performed takes or would
 *               take.  It depends on that encode alone and is exact for it.
 *   without a message   the capacity of the CLEAR re-encode: mp3s_clear_file for an MP3, mp3s_encode_file without hide_bits for a WAV.
 *   with a message      the call does the hide encode without producing the file: hide_offset and too_long are exactly what
 *               mp3s_hide_messages / mp3s_encode_files report for that file and message, bits is the count of THAT encode.  For a
 *               message that does not fit, bits == hide_offset: the exact capacity under that message.
 *   the clear capacity is an ESTIMATE of the capacity under a message: a table swapped through IDX_TO_TRANSFORM_HUF changes a region's
 *               bit count, which can move the quantizer step and, rarely, which regions are empty.  It estimates the capacity under a
 *               particular message; it does not bound it.
 *   text_bytes  the largest n such that an ASCII message of n bytes, framed by mp3s_message_frame ("<n>#" + message), has
 *               n_hide - 1 <= bits -- the too_long rule of every hide call; 0 when not even "0#" fits (mp3s_capacity_text_bytes).
 * The encode runs up to the chain check and stops there: no bit packing, no MP3 bytes.  k_capacity (mp3s_capacity_dev) counts on the
 * device, and the verdict, the per-stream records and (on request) the profile come down in one small copy.  Message variants,
 * selection and the device's re-runs are those of the hide calls.  Where the verdict says that the guesses of the first pass did not
 * hold (mp3s_chain_resolve_dev: verdict != 0), the group goes through the full encode instead -- the host resolves the chains as for a
 * hide call -- and is counted on the host from the final records; `fallback` tells which way a file went. */
typedef struct {
    int64_t bits;                    /* of the stream */
    int32_t active_units;            /* its units with MP3S_RF_ACTIVE */
    int32_t reserved;                /* 0 */
} mp3s_capacity_seg; /* 16 bytes */
/* k_capacity alone, asynchronous on the context's stream: d_gr = the records of a batch (unit order frame, ch, gr; n_tables 0 .. 3),
 * d_segs = its streams (first_frame and n_frames are read), d_out [n_segs]; d_profile optional, uint32 [frames of the batch]: per frame
 * the inclusive running sum of its stream's bits up to and including that frame (it restarts at every stream's first frame; the last
 * frame's value equals bits; 12 bits a frame and fewer than 2^28 frames stay below 2^32).  A stream of 0 frames gets zeros. */
int mp3s_capacity_dev(mp3s_ctx *ctx, const mp3s_gr_out *d_gr, const mp3s_chain_seg *d_segs, int n_segs, mp3s_capacity_seg *d_out,
                      uint32_t *d_profile);
typedef struct {
    int64_t bits, hide_offset, text_bytes;
    int32_t too_long, n_frames, kbps, sampling_rate, channels, active_units;
    int32_t fallback;          /* 0: counted by k_capacity; 1: through the full path (verdict, or a file the batch does not take) */
    int32_t reserved;
    const uint32_t *profile;   /* [n_frames] running sum, or NULL */
} mp3s_capacity;
/* The capacity of a list of MP3 files: decoded and encoded per (sampling rate, bitrate) group exactly as mp3s_hide_messages does it (the
 * PCM never leaves HBM), msgs / msg_lens by its rules (msgs[i] NULL = no message: the clear capacity; msgs NULL = none anywhere).
 * status[i] and mp3s_last_error() follow the rule of every list call; a file mp3s_hide_messages refuses (a mono re-encode, an empty
 * file, no sync ...) gets the same code, its out[i] zeroed.  Every file that call takes goes through the batch here as well.
 * want_profile != 0: out[i].profile = the per-frame running sum (see mp3s_capacity_dev), owned by *owner. */
int mp3s_capacity_files(mp3s_ctx *ctx, const uint8_t *const *mp3s, const size_t *lens, int n_files, const uint8_t *const *msgs,
                        const size_t *msg_lens, int want_profile, mp3s_buf **owner, mp3s_capacity *out, int32_t *status);
/* ... and of a list of WAV files: read, laid out and brought to the device as mp3s_encode_files does it (MP3S_OPT_WAV_IMPORT and
 * MP3S_OPT_WAV_RESAMPLE apply as they do there, every refusal of the reader in force is the file's code here), bitrate_kbps / hide_bits /
 * n_hide by its rules.  kbps, sampling_rate, channels and n_frames are what the encode call would report. */
int mp3s_capacity_wavs(mp3s_ctx *ctx, const uint8_t *const *wavs, const size_t *lens, int n_files, const int32_t *bitrate_kbps,
                       const uint8_t *const *hide_bits, const int32_t *n_hide, int want_profile, mp3s_buf **owner, mp3s_capacity *out,
                       int32_t *status);
/* text_bytes of a bit count (host only, no context): "1#a" is 24 bits, so 0 below 23 */
int64_t mp3s_capacity_text_bytes(int64_t bits);

/* ---------------------------------------------------------------- (vi-c) what hiding changed: exact PCM difference of MP3 file pairs
 * replaces: decoding both files (mp3s_decode_streams), pulling every PCM sample to the host -- 4.6 KB per frame and file -- and
 *           subtracting in numpy.  Both PCM arrays are in HBM after the decode; they are compared there and a few bytes per pair come down.
 * Which pair to compare: a re-encode delays the audio by the codec's delay, so a cover file and its stego file are NOT sample-aligned
 * and their raw difference means nothing.  The meaningful pair is the CLEAR re-encode (mp3s_clear_file) against the HIDE re-encode
 * (mp3s_hide_message) of the same input: the same delay, frames and bitrate, only the swapped Huffman tables differ.  The calls below
 * compare any two lists pairwise at lag 0 (there is no lag argument); the Python facade's hide_distortions builds exactly that pair.
 * Everything is exact integer arithmetic on int16 PCM, [frame][1152][nch] interleaved; per sample d = a - b:
 *   err2 = sum d^2, sig2 = sum a^2, max_abs = max |d|, n_diff = samples with d != 0, first_diff = the smallest interleaved sample index
 *   with d != 0 (inside the frame: 0xFFFFFFFF for none; of a pair: counted from its first compared sample, -1 for none).
 * The results are bit for bit what numpy computes in int64. */
typedef struct { uint32_t a_first, b_first, n_frames, out_first; } mp3s_pcm_pair;            /* 16 bytes: frames of 1152 rows in d_pcm; records at d_frames[out_first ..] */
typedef struct { uint64_t err2, sig2; uint32_t max_abs, n_diff, first_diff, reserved; } mp3s_pcm_frame_diff;   /* 32 bytes */
typedef struct { uint64_t err2, sig2, n_diff; int64_t first_diff; uint32_t max_abs, reserved; } mp3s_pcm_pair_diff; /* 40 bytes */
/* the two kernels alone (k_pcmdiff.hpp), asynchronous on the context's stream: frames [a_first, a_first + n_frames) against frames
 * [b_first, ...) of d_pcm (int16, nch = 1 or 2, 16-byte aligned) for every pair; pass 1 writes the frame records of pair p to
 * d_frames[out_first .. out_first + n_frames) (the ranges of different pairs must not overlap), pass 2 the pair records d_out[n_pairs].
 * A pair of 0 frames gets a zero record with first_diff -1.  h_pairs is the same table on the host: the launch geometry needs the frame
 * counts (pass 1 runs one wave per compared frame, spread over the device whatever the mix of long and short pairs is); it is read
 * before the call returns, the table made from it travels on the stream from a buffer the context keeps -- a second call on the context
 * waits for the first one's table to have left.  Null pointers, n_pairs <= 0, another nch or a misaligned d_pcm: MP3S_E_ARG (checked
 * without a device). */
int mp3s_pcm_diff_dev(mp3s_ctx *ctx, const int16_t *d_pcm, int nch, const mp3s_pcm_pair *d_pairs, const mp3s_pcm_pair *h_pairs,
                      int n_pairs, mp3s_pcm_frame_diff *d_frames, mp3s_pcm_pair_diff *d_out);
typedef struct {
    uint64_t err2, sig2; int64_t n_samples, n_diff, first_diff, rows_a, rows_b;
    uint32_t max_abs; int32_t channels, sampling_rate, n_frames;   /* n_frames = frames compared = min of the two */
    double snr_db, psnr_db;
    const mp3s_pcm_frame_diff *profile;  /* [n_frames] or NULL */
} mp3s_pcm_distortion;
/* File a[i] against file b[i], for a list of pairs, on the frame of the list-of-files calls: all 2 n files are scanned on the host
 * threads; the valid pairs are grouped by channel count, and per group ONE decode batch (int16, as mp3s_decode_streams decodes) leaves
 * the PCM of all its A and B streams in one device buffer, the two kernels run behind it on the same stream, and one small copy brings
 * the pair records down -- and the frame records when want_profile != 0 (out[i].profile, owned by *owner).  No PCM comes down.
 * Streams of different length compare their common prefix: n_frames = the smaller frame count, n_samples = n_frames * 1152 * channels;
 * rows_a / rows_b = both lengths in rows, the frame the decoder repeats after a bad header included, as mp3s_decoded.n_rows counts it
 * (that frame is PCM like any other and is compared).  The host derives, in double, from the exact integers:
 *   snr_db = 10 log10(sig2 / err2), psnr_db = 10 log10(32767^2 n_samples / err2); both +infinity when err2 == 0.
 * status[i] / mp3s_last_error() by the rule of mp3s_hide_messages: a pair one of whose files fails its front end gets that file's code
 * (MP3S_E_ARG for a null file), a pair whose files differ in channel count or sampling rate MP3S_E_UNSUPPORTED with a text naming both
 * values; the other pairs are unaffected; with status == NULL the first failing pair's code fails the call. */
int mp3s_pcm_distortion_files(mp3s_ctx *ctx, const uint8_t *const *a, const size_t *a_lens, const uint8_t *const *b, const size_t *b_lens,
                              int n_pairs, int want_profile, mp3s_buf **owner, mp3s_pcm_distortion *out, int32_t *status);

/* ---------------------------------------------------------------- (vi-d) a cover file against its stego file: lag search, difference at the lag
 * replaces: decoding both files (mp3s_decode_streams), pulling every PCM sample to the host and a numpy loop over the lags.
 * A re-encode delays the audio, so a file and its re-encode (a cover file and its stego file, a 128 kbit/s re-encode and its 320 kbit/s
 * source) are not sample-aligned and section (vi-c), which has no lag argument, cannot judge them.  The calls below find the delay by
 * an exhaustive integer search on the device and compare at it.  PCM is int16, [row][nch] interleaved; a pair is a run A of rows_a
 * rows and a run B of rows_b rows.  Lag L pairs row i + L of A with row i of B, d = a[i+L] - b[i] per channel: for A = stego and
 * B = cover a positive lag means the stego audio comes later.
 * Search, with M = max_lag (0 .. MP3S_PCM_MAX_LAG) and search_rows >= 1: W = min(rows_a, rows_b) - 2M; a pair with W < 1 is not
 * searched.  Otherwise S = min(W, search_rows) and the window is B rows [s0, s0 + S), s0 = M + (W - S) / 2 -- the middle of the file:
 * the start of an MP3 is often silence, where every lag ties.  For every L in [-M, +M]
 *   score[L + M] = sum over rows i in [s0, s0 + S) and the channels of (a[i+L] - b[i])^2        (uint64, exact)
 * -- every lag sees the same B samples and the same count of samples.  The found lag minimises the score; among equal scores the
 * smaller |L| wins, between +k and -k the +k.  n_best = the lags that reach the minimum (> 1: the answer is ambiguous).
 * Comparison at a lag L, found or given: the overlap is B rows [i0, i1), i0 = max(0, -L), i1 = min(rows_b, rows_a - L),
 * n_rows = max(0, i1 - i0); over its interleaved samples the fields of mp3s_pcm_pair_diff as in (vi-c) (sig2 = sum a^2, first_diff
 * from the first compared sample, -1 for none), and one mp3s_pcm_frame_diff per chunk of 1152 rows counted from i0, the last chunk
 * possibly partial.  At L = 0 on runs of whole frames this is exactly what mp3s_pcm_diff_dev computes. */
#define MP3S_PCM_MAX_LAG 4608
typedef struct { uint32_t a_first, a_rows, b_first, b_rows, out_first, reserved; } mp3s_pcm_run_pair;   /* 24 bytes: ROWS of d_pcm; chunk records at d_frames[out_first ..] */
typedef struct {
    int32_t lag; uint32_t n_best;            /* n_best 0: not searched (the lag was given, or the pair is too short: lag 0) -- then the next four are 0 */
    uint64_t err2_best, err2_at_0;           /* score[lag + M], score[M] */
    uint32_t search_first, search_rows;      /* s0, S */
    uint32_t n_rows, n_chunks;               /* the overlap at the lag, ceil(n_rows / 1152) */
} mp3s_pcm_lag;                              /* 40 bytes */
/* the three passes alone (k_pcmalign.hpp) and k_pcm_diff_pairs behind them, asynchronous on the context's stream.  d_pcm is 16-byte
 * aligned (and readable up to the next multiple of 4 bytes behind its last row, as every device allocation is); the runs lie anywhere in it.
 * h_lags == NULL: search.  d_scores[n_pairs][2 max_lag + 1] gets every searched pair's scores (the row of a pair that is not searched
 * is left as it was), d_lags[n_pairs] the lag records.  A pair with W < 1 gets n_best = 0, lag 0 and its comparison at lag 0.
 * h_lags != NULL: lag h_lags[p] (|lag| <= MP3S_PCM_MAX_LAG) is taken for pair p, nothing is searched, max_lag and search_rows are
 * only checked and d_scores may be NULL.  Either way pair p's chunk records go to d_frames[out_first .. out_first + n_chunks); the
 * range must hold ceil(min(a_rows, b_rows) / 1152) records, the bound for every lag, and the ranges of different pairs must not overlap;
 * records of the range past n_chunks are left as they were.  d_out[n_pairs] gets the pair records.  h_runs is the same table on the
 * host, read (as h_lags is) before the call returns: the launch geometry needs the row counts.  Null pointers, n_pairs <= 0, another
 * nch, max_lag outside 0 .. MP3S_PCM_MAX_LAG, search_rows < 1, a given lag beyond +-MP3S_PCM_MAX_LAG or a misaligned d_pcm:
 * MP3S_E_ARG (checked without a device). */
int mp3s_pcm_align_dev(mp3s_ctx *ctx, const int16_t *d_pcm, int nch, const mp3s_pcm_run_pair *d_runs, const mp3s_pcm_run_pair *h_runs,
                       int n_pairs, int max_lag, int search_rows, const int32_t *h_lags /* NULL = search */, uint64_t *d_scores,
                       mp3s_pcm_lag *d_lags, mp3s_pcm_frame_diff *d_frames, mp3s_pcm_pair_diff *d_out);
typedef struct {
    mp3s_pcm_distortion at_lag;   /* as (vi-c), over the overlap at the lag: n_frames = chunks of 1152 rows, n_samples = n_rows * channels; profile [n_frames] or NULL */
    mp3s_pcm_lag lag;
    const uint64_t *scores;       /* [2 max_lag + 1] with want_profile when the pair was searched, else NULL */
} mp3s_pcm_alignment;             /* 96 + 40 + 8 = 144 bytes */
/* File a[i] against file b[i] on the frame of mp3s_pcm_distortion_files -- the same front end, grouping by channel count, one decode
 * batch per group and status rules --, the three passes behind the decode and ONE copy down: 80 bytes a pair, with want_profile also
 * 32 a chunk and 8 a score.  lags == NULL: every pair is searched; a pair too short for max_lag (W < 1) gets MP3S_E_UNSUPPORTED with
 * a text naming its rows and max_lag, the other pairs are unaffected.  lags != NULL: lags[i] is taken for pair i. */
int mp3s_pcm_alignment_files(mp3s_ctx *ctx, const uint8_t *const *a, const size_t *a_lens, const uint8_t *const *b, const size_t *b_lens,
                             int n_pairs, int max_lag, int search_rows, const int32_t *lags /* NULL = search */, int want_profile,
                             mp3s_buf **owner, mp3s_pcm_alignment *out, int32_t *status);

/* ---------------------------------------------------------------- (vi-e) table audit: does a file carry a payload, and how much
 * replaces: nothing in the reference -- its reveal reads the table indices as bits whether or not anything was hidden, so it cannot tell
 *           a clean file from a stego file, finds no payload hidden as raw bits and none behind a damaged "<n>#" frame.
 * The reference's encoder picks a region's code book in two steps (__new_choose_table, reference encoder/MP3_Encoder.py:1170-1264):
 * a NATURAL choice from the region's quantised values alone, then IDX_TO_TRANSFORM_HUF[(choice, bit)] (:419-449) when a message bit
 * is left.  A decoder sees the values exactly, so the natural choice is recomputed here from the Huffman-decoded spectrum, and every
 * region is classified.  Units are visited as the stego bits walk them: frame, channel, granule, region.
 *   a window-switching unit (this encoder writes none): every non-zero one of table_select[0..1] is one FOREIGN region; table_select[2]
 *     is not in the side info and is not counted (the carry of SURVEY D10 is not followed); window_units counts the unit.
 *   any other unit: with bv = big_values (taken as at most 288) and the frame's long-block band table (of the rate the frame runs at: a
 *     frame with the reserved rate bits keeps the rate of the frame before),
 *     e1 = sfb_long[min(region0_count + 1, 22)], e2 = sfb_long[min(region0_count + region1_count + 2, 22)], a3 = 2 bv,
 *     a1 = min(e1, a3), a2 = min(e2, a3); the regions are the lines [0, a1), [a1, a2), [a2, a3).  A region with t = table_select[r] == 0
 *     is not counted.
 *   Region 0 with e1 > a3 and region 1 with e2 > a3 reach behind the big values: EMPTY, whatever they hold.  The encoder chose their book
 *     from every line up to e1 / e2 (__subdivide, :998-1036, does not cut the two at 2 bv, and with bv == 0 leaves the bounds of an earlier
 *     call standing), and the lines behind the big values do not reach a decoder as the encoder held them (the reference's decoder reads a
 *     count1 quadruple in the opposite order), so the natural choice cannot be computed again there.
 *   m = max |is| over the region's lines, 0 without lines.  m == 0: EMPTY -- the region names a book and holds no value.
 *   m < 15:  nat = 15 if bits(15) <= bits(13), else 13.
 *   m >= 15: c0 = the first i in 15..23, c1 = the first i in 24..31 with linmax[i] >= m - 15; nat = c1 if bits(c1) < bits(c0), else c0.
 *     (|is| <= 8206 is what a stream can hold; above it c0 = 23 and c1 = 31.)
 *   bits(t) = the reference's count_bit (:234-261): per pair of absolute values (x, y), for t > 15 a value above 14 adds linbits[t] and
 *     becomes 15; then hlen_t[x * 16 + y] + (x != 0) + (y != 0).
 *   t == nat: NATURAL.  Otherwise t == transform[nat][b] (b = 0 looked at first): FORCED with bit b, bits(t) - bits(nat) excess bits.
 *   Anything else, every t outside {13, 15..31} included: FOREIGN -- no encoder of this family wrote the region.
 * `regions` counts every classified region, and its running value in front of a region is the region's index; first_forced and
 * last_forced are such indices.  Two quirks of the reference make that index differ from a position among the bits reveal returns:
 * EMPTY regions count as stego bits for reveal (one that reaches behind the big values may carry a message bit, which the audit does
 * not see; this encoder writes such regions where a unit has fewer big values than its first bands have lines, in quiet passages and at
 * low bit rates), and a window-switching unit contributes its carried third index to reveal's bits but not to `regions`.  For a stream
 * of this encoder the second does not happen and the index IS the position among the bits of mp3s_reveal_messages.
 * A file this encoder wrote without a message has no FORCED region, and behind a message's end there is none; a random message forces
 * about every second region it is judged in, so last_forced + 1 is a lower bound on the payload's bits.  Exact integer arithmetic
 * throughout. */
#define MP3S_TA_NONE 0     /* table 0: not counted */
#define MP3S_TA_NATURAL 1
#define MP3S_TA_FORCED 2
#define MP3S_TA_FOREIGN 3
#define MP3S_TA_EMPTY 4
typedef struct {
    uint8_t cls[3];        /* MP3S_TA_* per region */
    uint8_t forced_bits;   /* bit r: the message bit region r was forced with */
    uint8_t nat[3];        /* the natural book per region (0 where none was computed: NONE, EMPTY, window switching) */
    uint8_t window;        /* 1: a window-switching unit */
    int16_t excess[3];     /* bits(t) - bits(nat) of a FORCED region (negative where the bit made the region cheaper: 15 -> 13), else 0 */
    uint16_t reserved;     /* 0 */
} mp3s_table_audit_unit; /* 16 bytes */
typedef struct { int32_t first_frame, n_frames; } mp3s_table_audit_seg; /* 8 bytes: a stream's frames in the batch */
typedef struct {
    int64_t regions, natural, forced, forced_ones, foreign, empty, excess_bits;
    int64_t first_forced, last_forced;   /* region indices, -1 when nothing is forced */
    int32_t n_frames, channels, sampling_rate, kbps, window_units, reserved;
    const uint32_t *profile;             /* [n_frames]: natural | forced << 4 | foreign << 8 | empty << 12 of each frame (each <= 12), or NULL */
} mp3s_table_audit; /* 9 * 8 + 6 * 4 + 8 = 104 bytes */
/* the two kernels alone (k_table_audit.hpp), asynchronous on the context's stream: d_is = int16 [n_frames][2 gr][2 ch][576] and d_side
 * [n_frames] as mp3s_huffman_decode_dev takes and leaves them (of a side record big_values, table_select, the region counts and
 * window_switching of every unit and sr_idx are read; ch 1 is ignored when nch == 1), d_segs [n_segs] the streams.  k_table_audit_units
 * writes d_units [n_frames][4], unit ch * 2 + gr (zeros for ch 1 of a mono batch) -- optional: NULL takes a buffer the context keeps;
 * k_table_audit_streams writes d_out [n_segs] (n_frames and channels filled in, sampling_rate, kbps and profile 0) and, with d_profile
 * (optional, uint32 [n_frames], indexed by batch frame), the frames' words.  A stream of 0 frames gets zeros and -1 / -1.  Null
 * pointers, n_frames <= 0, n_segs <= 0 or another nch: MP3S_E_ARG (checked without a device); the segments must lie inside the batch. */
int mp3s_table_audit_dev(mp3s_ctx *ctx, const int16_t *d_is, const mp3s_frame_side *d_side, int n_frames, int nch,
                         const mp3s_table_audit_seg *d_segs, int n_segs, mp3s_table_audit_unit *d_units /* optional */,
                         mp3s_table_audit *d_out, uint32_t *d_profile /* optional */);
/* The audit of a list of MP3 files on the frame of the list-of-files calls: the files are scanned on the host threads and grouped by
 * channel count; per group ONE batch goes through the front half of the decode (upload, Huffman decode, the host's repair of frames the
 * kernel flags, host-parsed streams placed) and the two kernels behind it.  No transform runs, no PCM exists; 104 bytes per file come
 * down, and 4 a frame with want_profile != 0 (out[i].profile, owned by *owner).  sampling_rate and kbps are the last frame's, as in every list call.  A file without a
 * frame gets zeros and -1 / -1.  status[i] / mp3s_last_error() by the rule of every list call (MP3S_E_ARG for a null file). */
int mp3s_table_audit_files(mp3s_ctx *ctx, const uint8_t *const *mp3s, const size_t *lens, int n_files, int want_profile, mp3s_buf **owner,
                           mp3s_table_audit *out, int32_t *status);

/* ---------------------------------------------------------------- (vi-f) PCM batches in the caller's device memory
 * replaces: none -- the reference writes a WAV file (decoder/decoder.py) and reads one (encoder/WAV_Reader.py)
 * Every other call that produces or consumes audio moves the PCM across PCIe.  The calls below leave a decoded list of MP3 files in
 * device memory the CALLER owns (in practice a tensor) as one batch, and encode such a batch, for a caller whose next or previous step
 * runs on the same GPU.  The batch is [B][C][T], channels first, planar, row-major: element (b, c, t) at ((b * C) + c) * T + t; C is 1
 * or 2.  Two element formats, both made from the int16 decode (MP3S_PCM_I16, the reference's sample for sample):
 *   MP3S_BATCH_I16: int16.   MP3S_BATCH_F32: float32 = int16 / 32768 (exact; the convention of WAV loaders).
 * Nothing is resampled: rows are rows, and the records say which rate they run at -- but for the calls that take a rate, at the
 * section's end (mp3s_pcm_batch_decode_files_at, mp3s_pcm_batch_encode_at). */
#define MP3S_BATCH_I16 0
#define MP3S_BATCH_F32 1
typedef struct {
    int64_t src_row;    /* first row of the stream in d_pcm, in rows of nch int16 (streams start on frame boundaries) */
    int64_t n_rows;     /* rows the stream has there (>= 0) */
    int64_t first_row;  /* where the window starts inside the stream (>= 0; may lie at or behind n_rows) */
    int32_t slot;       /* b: the item's rows go to d_out[b][.][0..T) */
    int32_t reserved;
} mp3s_pcm_batch_item; /* 32 bytes */
/* k_pcm_batch alone (k_pcmbatch.hpp), asynchronous on the context's stream: interleaved rows -> planar batch.  With
 * valid = clamp(n_rows - first_row, 0, T), element (slot, c, t) for t < valid comes from row src_row + first_row + t of d_pcm (int16,
 * nch = 1 or 2 samples a row, aligned to a row); on the row's int16 values l and r:
 *   nch == out_channels: copy.   nch == 1, out_channels == 2: the sample into both planes.
 *   nch == 2, out_channels == 1: int16 (l + r) >> 1 in int32 (arithmetic shift, so floor: -1, 0 gives -1);
 *                                float32 (l + r) / 65536 (exact, and NOT the floored int16 / 32768).
 * For t >= valid the element is written as zero.  Every element of an item's slot has exactly one writer, nothing has to be cleared
 * beforehand and nothing outside [slot][0..C)[0..T) is touched; the slots of different items must differ.  Any T, any first_row and any
 * d_out aligned to an element are taken: 16-byte stores are used wherever a plane allows them, narrower ones at its ends.  h_items is
 * the same table on the host, read before the call returns; the launch geometry made from it travels on the stream from a buffer the
 * context keeps, by the rule of mp3s_pcm_diff_dev.  Null pointers, n_items <= 0, nch or out_channels outside {1, 2}, an unknown format,
 * T <= 0, a misaligned pointer or a negative field of an item: MP3S_E_ARG (checked without a device). */
int mp3s_pcm_batch_dev(mp3s_ctx *ctx, const int16_t *d_pcm, int nch, const mp3s_pcm_batch_item *d_items,
                       const mp3s_pcm_batch_item *h_items, int n_items, int out_channels, int out_format, int64_t T, void *d_out);
typedef struct { int64_t dst_frame, n_rows; int32_t slot, reserved; } mp3s_pcm_unbatch_item; /* 24 bytes */
/* k_pcm_unbatch alone, asynchronous on the context's stream: planar batch -> the encoder's frames.  d_pcm is [frames][1152][2] int16
 * (16-byte aligned); item k fills ceil(n_rows / 1152) frames from dst_frame on with rows [0, n_rows) of d_in[slot], 1 <= n_rows <= T.
 * Rows at and behind n_rows in the item's last frame are zero, whatever the tensor holds there.  A mono input goes into both channels
 * (as the WAV import does with a mono file: the encoder has no mono path).  float32 becomes clamp(rint(x * 32768), -32768, 32767),
 * rounding half to even, NaN -> 0 (the rule of mp3s_wav_import_info's float files).  The frames of different items must not overlap.
 * Argument checks as above, n_rows outside [1, T] included. */
int mp3s_pcm_unbatch_dev(mp3s_ctx *ctx, const void *d_in, int in_channels, int in_format, int64_t T,
                         const mp3s_pcm_unbatch_item *d_items, const mp3s_pcm_unbatch_item *h_items, int n_items, int16_t *d_pcm);
typedef struct { int32_t n_frames, nch, sampling_rate, bit_rate; int64_t n_rows, first_row, valid_rows; } mp3s_pcm_batch_info; /* 40 bytes */
/* A list of MP3 files into the caller's batch d_out [n_files][out_channels][T] (device memory, out_bytes of it): the files go through
 * the front of mp3s_decode_streams, per channel count ONE decode batch (int16) leaves the PCM in a device buffer of the context, and
 * one k_pcm_batch launch per batch writes file i's window [first_rows[i], first_rows[i] + T) into slot i (first_rows NULL: 0).  No PCM
 * comes down.  info[i]: the stream's header fields, n_rows as mp3s_decoded.n_rows counts them (the repeated last frame of a stream that
 * ends in a bad header included), first_row as given and valid_rows = clamp(n_rows - first_row, 0, T), the rows of slot i that are
 * samples; behind them the slot is zero.  status[i] by the rule of mp3s_decode_streams: with status a file that fails alone does not
 * spoil the others (a failing batch is run again file by file), without it the first failing file fails the call.  A failed file has a
 * zeroed info[i], a failed or frameless file valid_rows 0 and a zeroed slot.  Files of different sampling rates may share a batch.
 * out_bytes < n_files * out_channels * T * element size, a negative first_row: MP3S_E_ARG before anything is touched.
 * d_out == NULL is the sizing call: only the front end runs, info is filled (valid_rows 0), nothing is decoded; T and out_bytes are
 * ignored.  The call returns behind a synchronise of the context's stream: the batch is complete for any other stream. */
int mp3s_pcm_batch_decode_files(mp3s_ctx *ctx, const uint8_t *const *mp3s, const size_t *lens, int n_files, const int64_t *first_rows /* NULL: 0 */,
                                int64_t T, int out_channels, int out_format, void *d_out, size_t out_bytes, mp3s_pcm_batch_info *info, int32_t *status);
/* The items of a batch d_in [n_items][in_channels][T] in device memory as MP3 files: item i is rows [0, n_rows[i]) of slot i, its last
 * frame zero-filled (k_pcm_unbatch), all items at one sampling rate (32 000, 44 100 or 48 000) and one bitrate, refused as
 * mp3s_encode_pcm refuses them; hide_bits / n_hide as for mp3s_encode_files (NULL: nothing is hidden).  ONE encode batch; out[i] is
 * what mp3s_encode_pcm gives for the item's frames (stereo, channels = 2), owned by *owner.  An item with n_rows outside [1, T] gets
 * MP3S_E_ARG in its status and is left out of the batch; status / mp3s_last_error() by the rule of mp3s_encode_files.  The caller
 * guarantees that the work which produced d_in has finished before the call; the call returns when the MP3 bytes are on the host, so
 * d_in may be reused at once. */
int mp3s_pcm_batch_encode(mp3s_ctx *ctx, const void *d_in, int n_items, int in_channels, int in_format, int64_t T, const int64_t *n_rows,
                          int samplerate, int bitrate_kbps, const uint8_t *const *hide_bits, const int32_t *n_hide,
                          mp3s_buf **owner, mp3s_file *out, int32_t *status);
/* The same calls with a sampling rate: decoding writes every slot at ONE rate of the caller's choosing, encoding reads a batch at any
 * rate.  The calls above are unchanged ("nothing is resampled" holds for them); the filter, the tap table and the output rule are those
 * of mp3s_wav_resample_info, exactly.  An extension beyond the reference.
 *  - ratio.  For in_rate > 0 and out_rate > 0: g = gcd, L = out / g, M = in / g, H = 16 if L >= M, else ceil(16 M / L), T = 2 H taps per
 *    phase.  L > 1280, T > 256 or no table from mp3s_wav_resample_taps(L, M): MP3S_E_UNSUPPORTED.  L = M = 1: not resampled (a copy).
 *  - decode direction.  A stream of n_in decoded rows (int16, 1 or 2 channels) becomes n_out = ceil(n_in L / M) rows: every channel is
 *    resampled on its own by the output rule (x = 0 outside [0, n_in), the result clamped to int16).  The resampled int16 rows then go
 *    through exactly the rules of mp3s_pcm_batch_dev with n_rows := n_out and first_row counted in OUTPUT rows: copy, mono into both
 *    planes, (l + r) >> 1 / (l + r) / 65536, zeros from valid = clamp(n_out - first_row, 0, T) on.  A stereo stream into one plane is
 *    resampled per channel FIRST and mixed afterwards (the other order would round differently).
 *  - encode direction.  An item's int16 rows are what mp3s_pcm_unbatch_dev makes of it (float32 rounded half to even, mono into both
 *    channels); they are resampled to the target mp3s_wav_resample_info's rule picks for `mode` at the item's rate, the last frame
 *    is zero-filled and the frames are encoded as mp3s_encode_pcm encodes them at the target rate. */
typedef struct { int32_t L, M, taps, half; } mp3s_pcm_resample_ratio; /* 16 bytes: out / in = L / M in lowest terms, T = 2 H, H */
/* no device, no context.  A rate <= 0 or a null pointer: MP3S_E_ARG; a refused ratio: MP3S_E_UNSUPPORTED.  The table is
 * mp3s_wav_resample_taps(L, M, ...). */
int mp3s_pcm_resample_plan(int in_rate, int out_rate, mp3s_pcm_resample_ratio *out);
typedef struct {
    int64_t src_row;    /* first row of the stream in d_pcm, in rows of nch int16 */
    int64_t n_rows;     /* INPUT rows the stream has there (>= 0) */
    int64_t first_row;  /* where the window starts, in OUTPUT rows (>= 0; may lie at or behind ceil(n_rows L / M)) */
    int32_t slot;       /* b: the item's rows go to d_out[b][.][0..T) */
    int32_t L, M;       /* the item's own ratio, in lowest terms; 1 / 1: a copy */
    int32_t reserved;
} mp3s_pcm_resample_item; /* 40 bytes */
/* k_pcm_batch_resample alone (k_pcmresample.hpp), asynchronous on the context's stream: mp3s_pcm_batch_dev with the resampler in front,
 * ONE launch for all items whatever their ratios are.  The items are given on the host only and read before the call returns; what
 * the kernel needs of them travels on the stream with the launch geometry.  Every element of an item's slot has exactly one writer,
 * nothing outside it is touched, any T, first_row and element-aligned d_out are taken.  Argument checks as mp3s_pcm_batch_dev's (fields
 * above 2^40 are refused like negative ones); an item whose ratio the plan refuses or whose L, M are not in lowest terms:
 * MP3S_E_UNSUPPORTED.  All are answered without a device. */
int mp3s_pcm_batch_resample_dev(mp3s_ctx *ctx, const int16_t *d_pcm, int nch, const mp3s_pcm_resample_item *h_items, int n_items,
                                int out_channels, int out_format, int64_t T, void *d_out);
typedef struct {
    int32_t n_frames, nch, sampling_rate /* the file's own */, bit_rate;
    int64_t n_rows;             /* OUTPUT rows: ceil(in_rows L / M) */
    int64_t first_row, valid_rows, in_rows /* what mp3s_pcm_batch_info.n_rows counts */;
    int32_t out_rate, L, M, reserved;
} mp3s_pcm_batch_info_at; /* 64 bytes */
/* mp3s_pcm_batch_decode_files with every slot at out_rate: the same front end, the same decode batch per channel count, and one
 * k_pcm_batch_resample launch per batch in the place of k_pcm_batch -- files of 32, 44.1 and 48 kHz share it, each with its own ratio; a
 * file at out_rate is copied.  first_rows, n_rows and valid_rows count OUTPUT rows.  Status rules, the sizing call (d_out == NULL: n_rows
 * at the output rate, valid_rows 0) and the zeroing of failed or frameless slots are unchanged.  A file whose rate the plan refuses for
 * out_rate gets MP3S_E_UNSUPPORTED by the per-file rule of any failing file.  out_rate <= 0: MP3S_E_ARG. */
int mp3s_pcm_batch_decode_files_at(mp3s_ctx *ctx, const uint8_t *const *mp3s, const size_t *lens, int n_files, int out_rate,
                                   const int64_t *first_rows /* NULL: 0 */, int64_t T, int out_channels, int out_format, void *d_out,
                                   size_t out_bytes, mp3s_pcm_batch_info_at *info, int32_t *status);
/* mp3s_pcm_batch_encode of a batch at ANY sampling rate in_rate.  `mode` takes the non-zero values of MP3S_OPT_WAV_RESAMPLE (1: the auto
 * rule, or 32000 / 44100 / 48000 forced; anything else MP3S_E_ARG).  Target == in_rate: the call IS mp3s_pcm_batch_encode at that rate,
 * byte for byte.  Otherwise k_pcm_unbatch lays the items at the source rate into a scratch of frames, the unchanged k_wav_resample
 * computes them into the encode batch's PCM and the batch is encoded at the target rate: out[i].sampling_rate is the target, n_frames
 * ceil(ceil(n_rows L / M) / 1152).  A rate the resampler refuses fails the call with MP3S_E_EXIT "Unsupported sampling frequency.";
 * the bitrate is checked against the target rate.  Items and status as for mp3s_pcm_batch_encode. */
int mp3s_pcm_batch_encode_at(mp3s_ctx *ctx, const void *d_in, int n_items, int in_channels, int in_format, int64_t T, const int64_t *n_rows,
                             int in_rate, int mode, int bitrate_kbps, const uint8_t *const *hide_bits, const int32_t *n_hide,
                             mp3s_buf **owner, mp3s_file *out, int32_t *status);

/* ---------------------------------------------------------------- QMDCT on the device, section vi-g: spectra as tensors, Markov features
 * (behind (vi-f); the label stands without parentheses and behind the title: the next heading of the dashed form is (vii))
 * replaces: nothing in the reference -- its decoder keeps the quantised MDCT coefficients (the `is` values of the Huffman decode) to
 *           itself.  They are what a payload lives in, and what MP3 steganalysis of ANY encoder works from; (vi-e) speaks for this
 *           encoder family only.
 * Both calls below stand on the front half of the decode (upload, Huffman decode, the host's repair, no transform), as (vi-e) does.
 * For one stream of n_frames frames and nch channels, d_is is the decoder's own layout, int16 [frame][2 gr][2 ch][576]:
 *   G = 2 * n_frames granule rows;  q[c][g][k] = is[g >> 1][g & 1][c][k];  a = |q| in int32 (-32768 gives 32768).
 * The frame a decoder repeats behind a bad header (dup_last_frame) has no spectrum of its own and is not a row.  A mono stream has rows
 * for c = 0 only; whatever lies at ch 1 of d_is is never read.  Rows are taken as they lie: short and mixed blocks keep their own line
 * order (three interleaved windows), nothing is reordered -- mp3s_table_audit.window_units says how many units of a file are such.
 *
 * Features.  T = MP3S_QMDCT_T, B = 2 T + 1 = 9, K = n_lines (1 .. 576): only the lines k < K count.  Per stream AND channel, all int64
 * and exact:
 *   hist[v], v = 0 .. 15:  the number of (g, k), g < G, k < K, with min(a, 15) == v.
 *   dh[g][k] = clamp(a[g][k] - a[g][k+1], -T, T) for k + 1 < K;
 *   intra[i][j]:  the number of (g, k), g < G, k + 2 < K, with dh[g][k] == i - T and dh[g][k+1] == j - T.
 *   dv[g][k] = clamp(a[g][k] - a[g+1][k], -T, T) for g + 1 < G;
 *   inter[i][j]:  the number of (g, k), g + 2 < G, k < K, with dv[g][k] == i - T and dv[g+1][k] == j - T.
 *   max_abs:  the maximum of a over the counted lines, 0 without rows.   bandwidth:  1 + the largest k < K with a != 0 in any row, 0 if none.
 * So sum(hist) = G K, sum(intra) = G max(K - 2, 0), sum(inter) = max(G - 2, 0) K.  Probabilities are a division the caller does.
 * The work of a stream is cut into slices of MP3S_QMDCT_SLICE granule rows of one channel, one workgroup each: a slice [s0, s1) owns
 * the hist and intra terms of its rows and the inter terms whose FIRST row lies in it (it reads rows up to s1 + 1 where they exist).
 * Every term has one owner and the sums are integers: the result does not depend on the order the slices arrive in. */
#define MP3S_QMDCT_T 4
#define MP3S_QMDCT_SLICE 64
typedef struct { int64_t hist[16], intra[9][9], inter[9][9], max_abs, bandwidth; } mp3s_qmdct_channel; /* 180 * 8 = 1440 bytes */
typedef struct { mp3s_qmdct_channel ch[2]; int32_t n_frames, channels, sampling_rate, kbps, n_lines, reserved; } mp3s_qmdct_features; /* 2904 bytes */
/* k_qmdct_features alone (k_qmdct.hpp), asynchronous on the context's stream.  d_segs [n_segs] are the streams (mp3s_table_audit_seg:
 * first_frame, n_frames) of the batch d_is of n_frames frames; h_segs is the same table on the host, read before the call returns: it
 * sizes the grid -- one workgroup per (segment, channel, slice) --, which travels on the stream from a buffer the context keeps, by the
 * rule of mp3s_pcm_diff_dev.  d_out [n_segs] is written completely (cleared on the stream in front of the kernel; the caller clears
 * nothing): n_frames, channels = nch and n_lines filled in, sampling_rate and kbps 0, ch[1] of a mono batch zero.  A segment of 0
 * frames gets zeros.  Null pointers, n_frames <= 0, n_segs <= 0, nch outside {1, 2}, n_lines outside [1, 576], a d_is that is not
 * 4-byte or a d_out that is not 8-byte aligned, an h_segs entry that reaches outside the batch: MP3S_E_ARG (checked without a device). */
int mp3s_qmdct_features_dev(mp3s_ctx *ctx, const int16_t *d_is, int n_frames, int nch, const mp3s_table_audit_seg *d_segs,
                            const mp3s_table_audit_seg *h_segs, int n_segs, int n_lines, mp3s_qmdct_features *d_out);
/* The features of a list of MP3 files on the frame of the list-of-files calls: scanned on the host threads, grouped by channel count,
 * per group ONE batch through the front half of the decode and one k_qmdct_features launch; 2904 bytes per file come down.
 * sampling_rate and kbps are the last frame's, as in every list call.  A file without a frame gets zeros with its header fields.
 * status[i] / mp3s_last_error() by the rule of every list call (MP3S_E_ARG for a null file).  The records point at nothing: no owner. */
int mp3s_qmdct_features_files(mp3s_ctx *ctx, const uint8_t *const *mp3s, const size_t *lens, int n_files, int n_lines,
                              mp3s_qmdct_features *out, int32_t *status);
/* The spectra themselves in the caller's device memory: int16 [B][C][Gt][576], row-major, C = 1 or 2, Gt granule rows a slot: element
 * (b, c, g, k) at (((b * C) + c) * Gt + g) * 576 + k. */
typedef struct {
    int64_t src_frame;      /* first frame of the stream in d_is */
    int64_t n_frames;       /* frames the stream has there (>= 0) */
    int64_t first_granule;  /* where the window starts inside the stream (>= 0; may lie at or behind 2 n_frames) */
    int32_t slot;           /* b: the item's rows go to d_out[b][.][0..Gt) */
    int32_t reserved;
} mp3s_qmdct_batch_item; /* 32 bytes */
typedef struct { int32_t n_frames, nch, sampling_rate, bit_rate; int64_t n_granules, first_granule, valid_granules; } mp3s_qmdct_batch_info; /* 40 bytes */
/* k_qmdct_batch alone (k_qmdct.hpp), asynchronous on the context's stream.  With valid = clamp(2 n_frames - first_granule, 0, Gt), row
 * (slot, c, g) for g < valid and c < nch is q[c][first_granule + g] of the item's stream; every other row of the slot is written as
 * zero (a mono item in a two-channel batch gets a zero plane 1).  nch == 2 with out_channels == 1: MP3S_E_ARG -- there is no
 * meaningful downmix of quantised values.  Every element of a slot has one writer, nothing has to be cleared first and nothing outside
 * the slot is touched; the slots of different items must differ.  d_is and d_out must be 16-byte aligned, which makes every row
 * aligned: 16-byte loads and stores only.  h_items is the same table on the host, read before the call returns (the launch geometry
 * travels as mp3s_pcm_batch_dev's does).  Null pointers, n_items <= 0, nch or out_channels outside {1, 2}, Gt <= 0 or above 2^24, a
 * misaligned pointer, a negative field of an item: MP3S_E_ARG (checked without a device). */
int mp3s_qmdct_batch_dev(mp3s_ctx *ctx, const int16_t *d_is, int nch, const mp3s_qmdct_batch_item *d_items,
                         const mp3s_qmdct_batch_item *h_items, int n_items, int out_channels, int64_t Gt, int16_t *d_out);
/* A list of MP3 files into the caller's batch d_out [n_files][out_channels][Gt][576] (device memory, out_bytes of it), by the rules of
 * mp3s_pcm_batch_decode_files with rows read as granules: per channel count ONE front half of the decode and one k_qmdct_batch launch
 * write file i's rows [first_granules[i], first_granules[i] + Gt) into slot i (first_granules NULL: 0).  info[i]: the header fields,
 * n_granules = 2 n_frames, first_granule as given, valid_granules = clamp(n_granules - first_granule, 0, Gt).  status[i]: with status a
 * file that fails alone does not spoil the others (a failing batch is run again file by file), without it the first failing file
 * fails the call; a stereo file with out_channels == 1 fails alone with MP3S_E_ARG.  A failed file has a zeroed info[i], a failed or
 * frameless file valid_granules 0 and a zeroed slot.  out_bytes < n_files * out_channels * Gt * 1152, a negative first granule, a
 * d_out that is not 16-byte aligned: MP3S_E_ARG before anything is touched.  d_out == NULL is the sizing call: only the front end
 * runs, info is filled (valid_granules 0); Gt and out_bytes are ignored.  The call returns behind a synchronise of the context's stream. */
int mp3s_qmdct_batch_decode_files(mp3s_ctx *ctx, const uint8_t *const *mp3s, const size_t *lens, int n_files, const int64_t *first_granules /* NULL: 0 */,
                                  int64_t Gt, int out_channels, int16_t *d_out, size_t out_bytes, mp3s_qmdct_batch_info *info, int32_t *status);

/* ---------------------------------------------------------------- (vii) asynchronous host-fed pipeline
 * replaces: a loop of Steganography.hide_message / clear_file over many files or batches of files -- reference
 *           steganography.py:133-182, whose two serial frame loops (decoder/MP3_Parser.py:68-80, encoder/MP3_Encoder.py:
 *           607-609) become four overlapping stages: host scan on worker threads (straight into page-locked staging) ||
 *           hipMemcpyAsync up || kernels || hipMemcpyAsync down, `depth` jobs in flight, nothing waited for until a result
 *           is collected.
 * A job = the files of one mp3s_hide_messages call (same arguments, same results byte for byte: jobs the device cannot
 * take in one batch, or whose Huffman data is damaged, are redone by that very function; a job whose on-device verdict says
 * a guess failed keeps its device buffers and has its chains resolved at collect time).
 * While a pipe exists its context belongs to it: no other call may use the context until mp3s_pipe_destroy().
 * The submitted file and message buffers are borrowed until the job has been collected. */
typedef struct mp3s_pipe mp3s_pipe;
typedef struct {
    int64_t submitted, collected;
    int64_t fast, slow;               /* collected jobs that went through the overlapped stages / through mp3s_hide_messages */
    double scan_ms, issue_ms;         /* summed over jobs: host scan + input layout; queueing the job's device work */
    double last_device_span_ms;       /* first upload byte to last download byte of the job collected last (HIP events) */
    double scan_cpu_ms;               /* CPU time of the scan threads inside scan_ms (less than scan_ms: the threads were not running) */
    int64_t resolved;                 /* collected jobs whose cursor / address guess failed and whose chains the host resolved on the job's
                                       * own device buffers (scan, decode and transforms kept); fast + resolved + slow = collected */
    /* how the pipe's streams were chosen when it was made (the runtime maps streams onto a few hardware queues; a pipeline whose
     * stages share queues loses its overlap): `rehearsals` miniature jobs of about 1 ms each, at most 12 and 15 ms in all -- 13 x the one-stream miniature, within 60 ms, where that is more (0: a
     * pipe made earlier on this context's stream decided), judged against the same miniature on ONE stream */
    double rehearsal_ms;
    int64_t rehearsals;
    int64_t lanes;                    /* rotation of the copy / front-end candidates | (compute candidate + 1) << 8 | (tail candidate + 1) << 16 */
    int64_t queue_shared;             /* 1: no choice got the miniature through in 0.94 x the one-stream time (side by side: 0.86 - 0.89; on one queue: 1.1 - 1.4): stages share hardware queues */
} mp3s_pipe_stats;
/* depth: jobs in flight (= staging slots); max_job_bytes: MP3 bytes per job the staging is sized for (larger jobs still
 * work, through the synchronous path); scan_threads: host workers */
int mp3s_pipe_create(mp3s_ctx *ctx, int depth, size_t max_job_bytes, int scan_threads, mp3s_pipe **out);
void mp3s_pipe_destroy(mp3s_pipe *pipe);
/* arguments as for mp3s_hide_messages (msgs NULL = clear all, msgs[i] NULL = clear file i); MP3S_E_BUSY when `depth`
 * jobs are in flight (collect one first) */
int mp3s_pipe_submit(mp3s_pipe *pipe, const uint8_t *const *mp3s, const size_t *lens, int n_files, const uint8_t *const *msgs,
                     const size_t *msg_lens, int64_t *ticket);
/* a decode job: the files of one mp3s_decode_file loop, MP3 bytes -> WAV bytes (int16) + stego bits per file; results
 * through mp3s_pipe_collect like those of the other jobs (out[i].data = the WAV image, bits / n_bits set) */
int mp3s_pipe_submit_decode(mp3s_pipe *pipe, const uint8_t *const *mp3s, const size_t *lens, int n_files, int64_t *ticket);
/* an encode job: the files of one mp3s_encode_files call (same arguments, same results byte for byte), WAV bytes -> MP3 bytes --
 * replaces a loop of Encoder(...).encode(), reference encoder/encoder.py:21-58, as the hide job replaces a loop of hide_message.
 * Stages: a worker reads the headers and lays out the encoder's inputs || the WAV images go up as they are (4 608 bytes per frame:
 * the largest transfer the library has) || k_wav_gather on the front-end stream, under the rate loop of the job in front || encode
 * side || download.  A job of more than one (sampling rate, bitrate) group, with a file that fails its checks, or larger than the
 * slot (frames: max_job_bytes / 96, the frames an MP3 job of that size can have -- the slot's WAV image is made from that count when
 * its first encode job comes --, and MP3 bytes OUT: max_job_bytes.  That image costs 48 x max_job_bytes of device memory per slot (402 MB for 8 MB jobs), + page-locked staging
 * as large as the short files -- below 256 KB each -- of the slot's jobs have needed so far) goes through mp3s_encode_files and counts as `slow`.  Results through mp3s_pipe_collect; the WAV and
 * hide_bits buffers are borrowed until then (bitrate_kbps and n_hide are copied). */
int mp3s_pipe_submit_encode(mp3s_pipe *pipe, const uint8_t *const *wavs, const size_t *lens, int n_files, const int32_t *bitrate_kbps,
                            const uint8_t *const *hide_bits, const int32_t *n_hide, int64_t *ticket);
/* waits for the OLDEST job in flight and hands out its results: out[i] / status[i] as mp3s_hide_messages fills them
 * (max_files = room in both arrays), *n_files = files of that job.  MP3S_E_BUSY: nothing in flight. */
int mp3s_pipe_collect(mp3s_pipe *pipe, int64_t *ticket, mp3s_buf **owner, mp3s_file *out, int32_t *status, int max_files,
                      int *n_files);
/* a block job: the share of rank `rank` of `world` in hiding a message in (utf8 != NULL) or clearing ONE stream -- the
 * arguments and the result of mp3s_reencode_block (carry_in NULL for rank 0; the carry is copied at submission) -- through
 * the overlapped stages beside the other jobs, so that the blocks a rank holds of streams that straddle its boundaries do
 * not interrupt the flow of the whole streams in front of and behind them (BASELINE configs[3]).  The result comes through
 * mp3s_pipe_collect_block when the job is the oldest in flight (mp3s_pipe_collect refuses a block job with MP3S_E_ARG). */
int mp3s_pipe_submit_block(mp3s_pipe *pipe, const uint8_t *mp3, size_t len, const uint8_t *utf8, size_t n_msg, int rank, int world,
                           const mp3s_carry *carry_in, int64_t *ticket);
int mp3s_pipe_collect_block(mp3s_pipe *pipe, int64_t *ticket, mp3s_buf **owner, mp3s_block *out);
/* 1: the oldest job in flight is a block job (collect it with mp3s_pipe_collect_block), 0: another job, MP3S_E_BUSY: none */
int mp3s_pipe_next_is_block(mp3s_pipe *pipe);
int mp3s_pipe_get_stats(mp3s_pipe *pipe, mp3s_pipe_stats *out);

#ifdef __cplusplus
}
#endif
#endif
