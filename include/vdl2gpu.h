/*
 * vdl2gpu.h -- C ABI of libvdl2gpu.so: the MI355X-native VDL Mode 2 front end.
 *
 * Drop-in boundary.  The reference has no plugin API; its
 * seam is the translation-unit pair d8psk.c + viterbi.c, entered through
 *
 *     void *rcv_thread(void *arg)            d8psk.c:335   (one pthread per channel)
 *     int   initD8psk(channel_t *ch)         d8psk.c:28
 *     unsigned reversebits(unsigned, int)    d8psk.c:39    (also used by out.c:429-432)
 *
 * consuming the shared sample block `Cbuff` (rtl.c:273 / air.c:190, 32768 samples
 * per hand-off, vdlm2.h:35) with per-channel `thread_param_t{chn,Fr,Fo}`
 * (vdlm2.h:49-52) and producing `msgblk_t` records (vdlm2.h:39-47) through
 * `decodeVdlm2(channel_t*)` (vdlm2.c:189).  This library replaces exactly that:
 * raw sample blocks in, burst records out, everything between on the GPU.
 *
 *     reference interface                      replaced by
 *     ---------------------------------------  -----------------------------------
 *     rcv_thread() x nbch + Bar1/Bar2           vdl2gpu_create() + vdl2gpu_push()
 *     in_callback() cu8->float, rtl.c:285-292   fused into the channeliser kernel
 *     rx_callback() real f32,  air.c:206-208    VDL2GPU_FMT_F32R (VDL2GPU_FMT_S16R: the same stream before
 *                                               the vendor library widens it, see the formats below)
 *     thread_param_t            vdlm2.h:49-52   vdl2gpu_chan_t (same three ints)
 *     decodeVdlm2(ch)           vdlm2.c:189     vdl2gpu_poll() -> vdl2gpu_burst_t,
 *                                               vdl2gpu_burst_to_msgblk() fills the
 *                                               reference's msgblk_t byte layout
 *     initD8psk / viterbi_*     d8psk.c:28,     internal to the kernels
 *                               viterbi.c:37-96
 *     reversebits               d8psk.c:39      reversebits() still exported
 *
 * Plain C types only; no torch / HIP types cross this boundary.  `iq` may be a
 * host pointer (copied with hipMemcpyAsync) or a device pointer (used in place).
 * All functions return 0 on success or a negative VDL2GPU_E* code; none aborts.
 */
#ifndef VDL2GPU_H
#define VDL2GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libvdl2gpu.so is built -fvisibility=hidden with an export map (csrc/vdl2gpu.map): what this header declares is what it exports */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define VDL2GPU_ABI_VERSION 6	/* 3: vdl2gpu_debug_heads, VDL2GPU_F_DEBUG_HEADS, VDL2GPU_MSGBLK_*; 4: vdl2gpu_stats_t.repairs; 5: vdl2gpu_inflight, the handle lock ("Threads");
				 * 6: vdl2gpu_get_host_profile, vdl2gpu_debug_clheads */
#define VDL2GPU_MAXCH 8		/* MAXNBCHANNELS vdlm2.h:26 */
#define VDL2GPU_MAXROWS 8	/* bursts with more rows are rejected, d8psk.c:103 */
#define VDL2GPU_ROWLEN 255

enum {
	VDL2GPU_OK = 0,
	VDL2GPU_EINVAL = -1,	/* bad argument / configuration */
	VDL2GPU_EHIP = -2,	/* a HIP runtime call failed (see vdl2gpu_last_error) */
	VDL2GPU_ENOMEM = -3,
	VDL2GPU_EOVERFLOW = -4,	/* reserved; record overflow is reported through vdl2gpu_stats_t.overflowed, never as an error */
	VDL2GPU_ENODEV = -5	/* no usable GPU: the library never falls back to the CPU */
};

/* sample formats of the wideband stream */
enum {
	VDL2GPU_FMT_CU8 = 0,	/* interleaved u8 I,Q; x = (float)b - 127.37f  (rtl.c:287-289) */
	VDL2GPU_FMT_CS16 = 1,	/* interleaved s16 I,Q; x = (float)v              */
	VDL2GPU_FMT_CF32 = 2,	/* interleaved f32 I,Q  (what Cbuff holds with WITH_RTL)     */
	VDL2GPU_FMT_F32R = 3,	/* real f32 (Cbuff with WITH_AIR, air.c:190)                 */
	/* Two formats receivers deliver natively that the reference's front ends never hand to Cbuff (announced by
	 * VDL2GPU_HAVE_FMT_CS8_S16R, the ABI version is unchanged).  An integer converts to float without rounding, so a
	 * handle fed one of them produces bit for bit what a CF32 / F32R handle produces from the same values -- at 2
	 * bytes a sample over the bus instead of 8 / 4.  VDL2GPU_F_RTL_QUIRK is VDL2GPU_EINVAL with either. */
	VDL2GPU_FMT_CS8 = 4,	/* interleaved s8 I,Q (HackRF, "cs8" recordings); x = (float)v, NO offset (the 127.37 is cu8's) */
	VDL2GPU_FMT_S16R = 5	/* real s16 (libairspy's AIRSPY_SAMPLE_INT16_REAL, which air.c:123 has widened to
				 * AIRSPY_SAMPLE_FLOAT32_REAL on the host); x = (float)v, imaginary part 0, mixed like
				 * VDL2GPU_FMT_F32R: D += x * wf (d8psk.c:368 WITH_AIR) */
};
#define VDL2GPU_HAVE_FMT_CS8_S16R 1

enum { VDL2GPU_MEM_HOST = 0, VDL2GPU_MEM_DEVICE = 1 };

/* == thread_param_t, vdlm2.h:49-52 */
typedef struct {
	int32_t chn;		/* channel number reported back in every burst */
	int32_t Fr;		/* channel frequency, Hz (only used for ppm, d8psk.c:302) */
	int32_t Fo;		/* offset from the tuner centre, Hz (d8psk.c:354) */
} vdl2gpu_chan_t;

typedef struct {
	uint32_t struct_size;	/* sizeof(vdl2gpu_config_t), for ABI growth */
	uint32_t sdrinrate;	/* SDRINRATE: any multiple of 25 kHz from 100 kHz on (2 MS/s rtl.c:36, 5/6 MS/s air.c:134, 10 MS/s ...),
				 * with sdrclk such that the general channeliser's LDS, ((L + maxwin) * 8 + 32 * maxwin) * 8 bytes
				 * with L = sdrinrate / 25000 and maxwin = (sdrclk + 20) / 21, stays within 160 KiB (gfx950's limit
				 * per workgroup).  At the default sdrclk that is up to 25.7 MS/s; at 2 MS/s, sdrclk up to 10416.
				 * Off the 25 kHz grid (announced by VDL2GPU_HAVE_OFFGRID_RATES, the ABI version is unchanged:
				 * 2.048 MS/s of rtl_sdr, 1.024 / 1.92 / 2.56 / 2.88 MS/s, the 61.44/n family 1.92 .. 30.72 MS/s):
				 * any multiple of 1 kHz from 100 kHz on whose LO table, L = vdl2gpu_lo_len(sdrinrate) =
				 * sdrinrate / gcd(sdrinrate, 25000) entries, divides a period of the dump schedule
				 * (4 * sdrclk % L == 0; at the default sdrclk every multiple of 4 kHz) and whose window part of
				 * that LDS, (maxwin * 8 + 32 * maxwin) * 8 bytes, stays within 160 KiB (the table itself need
				 * not): at the default sdrclk maxwin <= 512, up to 43.0 MS/s, so 30.72 MS/s is accepted and 61.44 MS/s is not.
				 * The table is a whole period of the local oscillator only for channel offsets Fo on the 25 kHz
				 * grid, where VDL channels lie; an offset off that grid gets the reference's phase jump every L
				 * samples unless the handle has VDL2GPU_F_EXACT_FO.  VDL2GPU_F_RTL_QUIRK is VDL2GPU_EINVAL off the grid.
				 * Anything else is VDL2GPU_EINVAL from vdl2gpu_create, before any device call. */
	uint32_t sdrclk;	/* SDRCLK, in (21, 1000000] and within the LDS bound above; 0 = sdrinrate/4000 (rtl.c:37, air.c:138) */
	int32_t fmt;		/* VDL2GPU_FMT_* */
	int32_t nbch;		/* channels per wideband stream, 1..8 */
	int32_t nstreams;	/* independent wideband streams decoded side by side (>=1) */
	const vdl2gpu_chan_t *chan;	/* nstreams*nbch entries, stream-major */
	uint64_t max_push;	/* largest nsamples a single vdl2gpu_push() will carry.  Throughput grows with the push (≈ 0.4 ms of
				 * fixed work per push).  The parallel sync tables of a push hold 4096 trigger candidates per channel
				 * (a burst leaves about 18: a channel at 4 bursts a second fills them in 50 s, a saturated one in
				 * 16 s); a channel that exceeds them is handled by the serial machine for that stretch (exact, ~100x
				 * slower; stats.serial_samples shows it).  Long pushes are therefore cut into equal parts inside the
				 * library -- the bursts are the same for any cut --: 8.4 s of air time until the first pushes have
				 * been collected, then as long as fills 90 % of the tables at the candidate density of the busiest
				 * channel over the last four parts, at most 36 s (72 MS at 2 MS/s).
				 * Limit: every stream holds 8 planes of cap = ceil16(49152 + 21 * max_push / sdrclk + 66) decimated
				 * samples (8 bytes each) for max_push; vdl2gpu_create returns VDL2GPU_EINVAL when 8 * cap * 8 bytes
				 * reach 4 GiB (max_push >= 1 596 657 881 at 2 MS/s with the default sdrclk, >= 70 252 947 at sdrclk 22). */
	int32_t device;		/* HIP device ordinal */
	uint32_t max_bursts;	/* burst-record ring capacity (0 = default 65536) */
	uint32_t flags;		/* VDL2GPU_F_* */
} vdl2gpu_config_t;

#define VDL2GPU_F_KEEP_DEC 1u	/* accepted for compatibility: the last push's decimated stream is always kept (vdl2gpu_debug_dec) */
#define VDL2GPU_F_FULLSCAN 4u	/* scan all four FIR sub-phases everywhere instead of probe + regions + verify */
#define VDL2GPU_F_TEST_NOREGION 8u	/* test hook: drop the region scan; the verify pass must then redo channels serially.  Only
					 * libvdl2gpu_test.so (the same sources with -DVDL2GPU_TESTHOOKS) honours it, together with the
					 * VDL2GPU_PRIM_DROP / VDL2GPU_SPLIT_SAMPLES environment handicaps; libvdl2gpu.so rejects the
					 * flag with VDL2GPU_EINVAL and never reads those variables.
					 * VDL2GPU_TEST_EPOCH=T0 (test build, read once in vdl2gpu_create): the handle begins as if T0 input
					 * samples per stream had already been pushed and had left the canonical start state behind them --
					 * total_in = T0, every stream's planes begin at frame D0 - carry with D0 = 21 T0 / SDRCLK, every
					 * channel's next evaluation is D0 + 1, everything else is the zero / perr = 100 start -- so every
					 * stamp it hands out (trig_dec, end_dec, sym_first_dec: + D0; trig_sample, end_sample: + T0) and
					 * samples_in / dec_samples are absolute, the counters start at 0, and whatever the host derives
					 * from the samples so far (the push's place in the dump schedule and the LO table, the exact-Fo
					 * base) follows from total_in.  T0 must be one at which the stream is exactly shift-invariant: a
					 * multiple of 16 SDRCLK (a superperiod of the dump schedule: D0 a multiple of 336), of
					 * vdl2gpu_lo_len(sdrinrate), and of 32768 with VDL2GPU_F_RTL_QUIRK, at most 2^56; anything else is
					 * VDL2GPU_EINVAL before any device call.  (With VDL2GPU_F_EXACT_FO the residual oscillator is
					 * shift-invariant only at multiples of 2 sdrinrate; other admissible T0 are accepted, and the
					 * rotation is then that of the absolute sample indices.)
					 * VDL2GPU_TEST_TICKET0=n (test build): k1_fast's work counters, on the device and as the host
					 * keeps them, start at n instead of 0 (they are 32 bits wide and never reset) */
#define VDL2GPU_F_FRAMES 16u	/* run the block path (RS, HDLC, FCS) on every push's bursts as well: vdl2gpu_poll_frames() */
#define VDL2GPU_F_SERIAL 2u	/* diagnostics: skip the parallel sync tables, one serial machine per channel */
#define VDL2GPU_F_RTL_QUIRK 32u	/* cu8 only: reproduce in_callback() as written (rtl.c:285-292): in every hand-off block of
				 * 32768 samples, sample k is stored at index k+1, index 0 stays 0 and the last sample is
				 * lost -- what the reference decodes on a real RTL stick.  Every push must
				 * then be a whole number of 32768-sample blocks (RTLINBUFSZ/2, vdlm2.h:35). */

#define VDL2GPU_F_DEBUG_HEADS 64u	/* diagnostics: keep the header soft bits of every sync trigger of the last push (vdl2gpu_debug_heads) */
#define VDL2GPU_F_LEVELS 128u	/* measure every burst's signal and noise level on the GPU: vdl2gpu_poll_levels() (see vdl2gpu_level_t) */
#define VDL2GPU_F_SOFT_RS 256u	/* keep every payload byte's reliability (vdl2gpu_soft_t, vdl2gpu_poll_soft()); with VDL2GPU_F_FRAMES the
				 * block path then rescues rows the reference cannot decode by erasing their least reliable bytes */

/* ---- channel offsets off the 25 kHz grid (VDL2GPU_F_EXACT_FO; announced by VDL2GPU_HAVE_EXACT_FO, the ABI version is unchanged) ----
 * The reference's LO table (d8psk.c:353-357) is indexed modulo L = SDRINRATE / 25000, so an offset Fo that is no multiple of
 * 25 kHz gets a phase jump every L samples, and a handle without this flag reproduces that.  With the flag Fo
 * may be any integer Hz with |Fo| < sdrinrate / 2, at every accepted rate, and the oscillator is phase-continuous:
 *   Fg = 25000 * floor((Fo + 12500) / 25000),  Fd = Fo - Fg in [-12500, 12500).
 *   1. The mixer runs as without the flag with the table vdl2gpu_lo_table(sdrinrate, Fg) (what vdl2gpu_debug_lo returns).
 *   2. A channel with Fd == 0 is left alone: its plane has the bits a handle without the flag produces.
 *   3. Otherwise every output D_m (the value after D /= nf, d8psk.c:377) is rotated by the residual oscillator at the centre
 *      of its window.  With a_m, e_m the stream indices of the window's first and last input, R = sdrinrate and
 *      fd = Fd mod 2R (non-negative):
 *          k_m = (fd * ((a_m + e_m) mod 2R)) mod 2R          the phase index, angle -pi * k_m / R
 *          r_m = T_hi[k_m >> 12] (x) T_lo[k_m & 4095]
 *          D'_m = D_m (x) r_m
 *      where x (x) y = (xr*yr - xi*yi, xr*yi + xi*yr) in float32, each product and the sum or difference rounded on its own.
 *   4. T_hi[h] = ((float)cos(-pi*(h*4096)/R), (float)sin(..)) for h < ceil(2R/4096), T_lo[l] = ((float)cos(-pi*l/R),
 *      (float)sin(..)) for l < 4096, computed in double precision on the host and narrowed once.
 * The rotation happens inside the channeliser kernels where they dump; |r_m| = 1 to within 1e-7, so the scale of
 * vdl2gpu_level_t is unaffected.  Together with VDL2GPU_F_RTL_QUIRK: VDL2GPU_EINVAL, before any device call (the quirk is for
 * parity with the reference, jumps included).  vdl2gpu_exact_fo_tables / vdl2gpu_exact_fo_index below state 3. and 4. on the host. */
#define VDL2GPU_F_EXACT_FO 512u
#define VDL2GPU_HAVE_EXACT_FO 1

/* One decoded burst = the msgblk_t fields the DSP fills (vdlm2.h:39-47). */
typedef struct {
	int32_t stream;
	int32_t chn;		/* msgblk_t.chn */
	int32_t Fr;		/* msgblk_t.Fr */
	int32_t nbrow;		/* msgblk_t.nbrow  (header value, d8psk.c:94) */
	int32_t nlbyte;		/* msgblk_t.nlbyte (header value, d8psk.c:95) */
	float df;		/* carrier estimate at sync, rad/symbol (channel_t.df) */
	float ppm;		/* msgblk_t.ppm, d8psk.c:302 */
	int64_t trig_dec;	/* 84 kS/s sample index of the sync trigger (stream time) */
	int64_t end_dec;	/* 84 kS/s sample index of the last symbol of the burst */
	int64_t trig_sample;	/* the same instants in input samples */
	int64_t end_sample;
	uint8_t data[VDL2GPU_MAXROWS][VDL2GPU_ROWLEN];	/* msgblk_t.data rows 0..7 */
} vdl2gpu_burst_t;

/* ---- link quality (VDL2GPU_F_LEVELS; announced by VDL2GPU_HAVE_LEVELS, the ABI version is unchanged) ----
 * The reference keeps only the argument of the channel-filtered value S (filteredphase(), d8psk.c:219-229); with
 * VDL2GPU_F_LEVELS the demodulator also measures |S|^2 while it decodes a burst's payload.  For one channel of one stream,
 * x[n] = the 84 kS/s sample at stream time n (what vdl2gpu_debug_dec returns), mflt[0..64] the channel filter's taps:
 *     S(n, c) = sum_j x[n - 16 + j] * mflt[c + 4j]   over j >= 0 with c + 4j <= 64      (newest sample n, sub-phase c = 0..3)
 *   signal: the burst's symbol evaluations n_k = sym_first_dec + 8k, k = 0 .. nsym-1, all at sub-phase `subphase`:
 *           sig_power = mean_k |S(n_k, subphase)|^2.  The last of them is end_dec (end_dec = sym_first_dec + 8 (nsym - 1));
 *           the first lies trig_dec + 1 .. trig_dec + 8 (the first symbol after the reference's P1, d8psk.c:306, which is taken at
 *           trig_dec with the trigger's own sub-phase 4..12 and is not counted).
 *   noise:  256 evaluations at sub-phase 0 before the burst, m_i = sym_first_dec - 512 - 8i (i = 0..255; the guard of 512 clears the
 *           ramp, the sync word and the filter memory), in 8 blocks of 32 (block b: i in [32b, 32b + 32)).  A block is valid if its
 *           oldest sample m_{32b+31} - 16 >= 0 (the stream's start clips it).  noise_power = the MEDIAN of the valid blocks' mean
 *           |S|^2 (the mean of the two middle ones for an even count); noise_blocks = the number of valid blocks (0..8); with 0
 *           blocks noise_power and noise_dbfs are NaN.  The median tolerates the tail of a preceding burst in up to 3 of the 8
 *           blocks; on a saturated channel (bursts back to back) the value is an upper bound of the noise floor.
 *   scale:  K = (FS * sum_{j=0..16} mflt[4j])^2, FS = 128 (cu8, cs8), 32768 (cs16, s16r), 1 (cf32, f32r): the channeliser AVERAGES the
 *           input samples of each 84 kS/s output (D /= nf, d8psk.c:378), so a full-scale complex tone at the channel centre
 *           leaves it at FS; sig_dbfs = 10 log10(sig_power / K), noise_dbfs likewise, and that tone reads about 0 dBFS.  White
 *           noise of sigma per component reads 10 log10(2 sigma^2 / M * sum_j mflt[4j]^2 / K), M = sdrinrate / 84000.  A real
 *           tone (VDL2GPU_FMT_F32R, and VDL2GPU_FMT_S16R against its FS of 32768) reads about 6 dB lower: the real stream's
 *           image half is not in the channel.
 * The sums run in a fixed order over the symbol index (64 strided partial sums in ascending k, then a fixed pairwise tree; each
 * noise block: a fixed pairwise tree of its 32 values): a burst gets bit-identical levels whatever kernel, path or repair round
 * decoded it and however the stream was cut into pushes.  Levels need no extra input: the noise window lies inside the carried
 * planes even for the longest burst decoded in the push after its trigger. */
#define VDL2GPU_HAVE_LEVELS 1
typedef struct {
	float sig_dbfs;		/* @0  10 log10(sig_power / K) */
	float noise_dbfs;	/* @4  10 log10(noise_power / K); NaN with noise_blocks == 0 */
	float sig_power;	/* @8  mean |S|^2 over the burst's symbols */
	float noise_power;	/* @12 median of the valid noise blocks' mean |S|^2; NaN with noise_blocks == 0 */
	int64_t sym_first_dec;	/* @16 stream time (84 kS/s) of the first symbol evaluation */
	int32_t nsym;		/* @24 symbol evaluations averaged */
	int32_t subphase;	/* @28 their FIR sub-phase, 0..3 */
	int32_t noise_blocks;	/* @32 valid noise blocks, 0..8 */
	int32_t reserved;	/* @36 0 */
} vdl2gpu_level_t;		/* sizeof 40, alignment 8 */

/* ---- soft-decision RS erasures (VDL2GPU_F_SOFT_RS; announced by VDL2GPU_HAVE_SOFT_RS, the ABI version is unchanged) ----
 * The reference slices the payload hard (V > 0.5, d8psk.c:119, 168) and erases only the padding of a short last row (vdlm2.c:63-82).
 * With VDL2GPU_F_SOFT_RS the demodulator keeps how sure it was of every payload byte:
 *   bit reliability   for Grey table w = 0..2 (Grey1/2/3, d8psk.h:47ff) and table index idx = 0..256 (the differential slice):
 *                     R(w, idx) = min(255, (int)floor(fabs((double)Grey_w[idx] - 0.5) * 512)); the descrambler does not enter.
 *   byte reliability  payload byte b (bits q = 25 + 8b + i, i = 0..7, counted from the first header bit): the minimum of R over its
 *                     8 bits, stored at the byte's (row, col) -- the same de-interleave the record's data[] uses.  Every position
 *                     of rel[][] that carries no transmitted byte (zero fill, rows >= nbrow, parity that is not sent) is 255.
 * Row rule of the block path in soft mode (vdl2gpu_decode_blocks_soft; the pipeline's block path with VDL2GPU_F_FRAMES).  Row r has
 * by data bytes and e0 fixed erasures (0, 2 or 4) as in the reference; p_r parity bytes were sent (6 for r < nf_rows - 1, nf_last
 * for r == nf_rows - 1, 0 beyond; nf_rows = nbrow - 1 and nf_last = 6 when nlbyte <= 2, else nf_rows = nbrow and nf_last = 2, 4, 6
 * for nlbyte <= 30, <= 67, above):
 *   1. the reference's rs() runs as always; a row it decodes (count >= 0) is kept as it decoded it;
 *   2. otherwise the candidates [0, by) and [249, 249 + p_r) are ordered by (reliability, position), both ascending;
 *   3. for s = 2, then 4, as long as e0 + s <= 4: rs() of the received row with the e0 fixed erasures followed by the first s
 *      candidates; the first trial that returns >= 0 and leaves all six syndromes zero replaces the row (two parity roots always
 *      stay for detection);
 *   4. if none does, the row is what the reference left (its partial corrections included).
 * HDLC, the flag hunt and the FCS follow unchanged, so a rescued row only ever adds frames that pass the FCS.
 * Memory: 2048 bytes per record slot in each of the device output rings and each host slab, and in the host queue beside every
 * burst record it holds. */
#define VDL2GPU_HAVE_SOFT_RS 1
typedef struct {
	uint8_t rel[VDL2GPU_MAXROWS][VDL2GPU_ROWLEN];	/* @0    byte reliability, 0 (on a decision boundary) .. 255 */
	uint8_t reserved[8];				/* @2040 0 */
} vdl2gpu_soft_t;		/* sizeof 2048 */

/* ---- carrier offset and phase-error spread (VDL2GPU_F_CARRIER; announced by VDL2GPU_HAVE_CARRIER, the ABI version is unchanged) ----
 * A burst record's df / ppm are the reference's one-shot estimate from the 16 sync symbols (d8psk.c:281-302), and stay that.  As a
 * frequency they carry a convention and a scatter: the reference's sync-word table has a slope of pi/8 per symbol built in, so that
 * the slicer (d8psk.c:213, 323-327) sees the eight D8PSK increments at the CENTRES of its sectors -- Grey table index 16 + 32 m, not
 * 32 m -- and 10500 df / 2 pi reads 656.25 Hz below the true offset, give or take some 10 Hz rms.  With VDL2GPU_F_CARRIER the
 * demodulator adds up, over the whole burst, how far every slice fell from the centre of its sector; that is the carrier offset the
 * one-shot estimate left behind, and its spread is the burst's modulation quality.
 * For an accepted burst with header values nbrow, nlbyte, trigger trig_dec, one-shot timing clk0 and carrier estimate df:
 *   ND, NF       data and FEC bytes transmitted (d8psk.c:117-206): ND = 249 (nbrow - 1) + (nlbyte ? nlbyte : 249); nlbyte <= 2: FEC rows
 *                nbrow - 1, the last with 6 bytes, else nbrow rows, the last with 2 / 4 / 6 bytes for nlbyte <= 30 / <= 67 / above;
 *                NF = 6 (FEC rows - 1) + the last row's (0 without FEC rows)
 *   j0, rb       j0 = max(1, (32 - clk0 + 3) / 4), rb = clk0 + 4 j0 - 32 (d8psk.c:239, 317-319)
 *   kmax         (25 + 8 (ND + NF) - 1) / 3: the symbol that carries the last transmitted bit
 *   symbols      k = 8 .. kmax -- exactly the slices the payload decode and the reliability map (vdl2gpu_soft_t) take:
 *                P_k   = filteredphase() (d8psk.c:219-230) at stream time trig_dec + j0 + 8 k, sub-phase rb
 *                idx_k = the slicer's Grey table index of (P_k, P_{k-1}, df), 0..256, 32 steps a sector
 *                e_k   = (idx_k & 31) - 16, in [-16, 15]
 *   nsym = kmax - 7,  sum_e = sum e_k,  sum_e2 = sum e_k^2 (at most 256 nsym)
 * The sums are integers, so no order of summation has to be defined: a burst gets the same record whatever kernel, path or repair
 * round decoded it and however the stream was cut into pushes.  The host derives the rest in double precision, as it does ppm
 * (vdl2gpu_carrier_from_sums is that arithmetic, and what the library itself calls):
 *   m       = (double)sum_e / nsym
 *   dphi_d  = (double)df + M_PI / 8 + m * M_PI / 128        true rotation per symbol beyond the data, rad
 *   dphi    = (float)dphi_d
 *   freq_hz = (float)(10500.0 * dphi_d / (2 * M_PI))
 *   ppm     = (float)(10500.0 * dphi_d / (2 * M_PI * (double)Fr) * 1e6)
 *   rms_rad = (float)(sqrt(max(0, (double)sum_e2 / nsym - m * m)) * M_PI / 128)
 * Sign: positive means the carrier lies ABOVE the channel centre as mixed -- above Fo, or above Fg + Fd with VDL2GPU_F_EXACT_FO; a
 * receiver whose tuner sits low sees its channels high.  freq_hz is what to add to every Fo of an exact-Fo handle.
 * The estimate is decision-directed: it is as good as the slicer's decisions.  A burst whose rms_rad approaches the half-sector
 * pi / 8 = 0.39 has symbols in the wrong sectors and is not to be trusted; a clean one reads 0.02 .. 0.1.  It needs no noise window,
 * so it is a quality figure on a saturated channel too, where vdl2gpu_level_t's noise floor is only an upper bound.
 * Memory: 32 bytes per record slot wherever a level record has 40 -- each device output ring, each host slab, and the host queue
 * beside every burst record it holds. */
#define VDL2GPU_F_CARRIER 1024u
#define VDL2GPU_HAVE_CARRIER 1
typedef struct {
	int32_t nsym;		/* @0  symbols summed, kmax - 7 */
	int32_t sum_e;		/* @4  sum of e_k */
	uint32_t sum_e2;	/* @8  sum of e_k^2 */
	int32_t reserved;	/* @12 0 */
	float dphi;		/* @16 rotation per symbol beyond the data, rad */
	float freq_hz;		/* @20 the same as a frequency: 10500 dphi / 2 pi */
	float ppm;		/* @24 ... relative to the channel frequency Fr (the burst record's own ppm stays the reference's) */
	float rms_rad;		/* @28 spread of the slices around their mean, rad */
} vdl2gpu_carrier_t;		/* sizeof 32, alignment 4 */

/* ---- block report (VDL2GPU_F_BLOCK_REPORT; announced by VDL2GPU_HAVE_BLOCK_REPORT, the ABI version is unchanged) ----
 * The block path (vdlm2.c:84-161: RS(255,249) per row, HDLC un-stuffing, flag hunt, check_frame) hands on the frames that pass and
 * nothing else; the reference says at verbose > 2 why a candidate did not ("#%d error too short", "#%d error crc", vdlm2.c:44-58).
 * With VDL2GPU_F_BLOCK_REPORT (which needs VDL2GPU_F_FRAMES: without it vdl2gpu_create returns VDL2GPU_EINVAL) every burst record
 * gets a vdl2gpu_blockrep_t that says what the block path made of it; vdl2gpu_decode_blocks_report gives the same for a batch on
 * any handle.  For a record with header values nbrow, nlbyte (status 0):
 *   rows        r < nbrow.  Row r has `by` data bytes (249, the last row nlbyte), e0 fixed erasures from set_eras() (vdlm2.c:63-82:
 *               the last row's 251..254 for by <= 30, 253..254 for by <= 67) and p_r transmitted parity bytes, all as at
 *               vdl2gpu_soft_t.  The RECEIVED row is data[r] of the record.
 *   row_roots   what rs() (rs.c:81) returns for the received row with those erasures: -1, or the number of roots it corrected
 *               (erasures count); 0 means all six syndromes were zero.  In soft mode too this is the reference's run on the received
 *               row, not a trial's.
 *   row_how     (the VDL2GPU_ROW_* names are #defines, below)
 *               VDL2GPU_ROW_CLEAN  the received row's syndromes are all zero: nothing was touched
 *               VDL2GPU_ROW_REF    rs() returned >= 0: the row is what the reference decodes (a miscorrection included)
 *               VDL2GPU_ROW_SOFT2 / _SOFT4  soft mode (the record has a reliability map): rs() returned -1 and the trial with
 *                                  2 / 4 candidates of the row rule (vdl2gpu_soft_t, step 3) replaced the row
 *               VDL2GPU_ROW_FAIL   rs() returned -1 and no trial replaced the row (hard mode: none is made; soft mode: e0 + 2 > 4,
 *                                  or every trial failed): the row is what the reference left, its partial corrections included
 *               VDL2GPU_ROW_NONE   r >= nbrow
 *   row_changed the positions j in [0, by) or [249, 249 + p_r) -- the bytes that were transmitted -- at which the row the un-stuffer
 *               reads differs from the received row: the "octets corrected by FEC" of row r (0..255)
 *   stuffed     the zeros the un-stuffer dropped (t == 5, vdlm2.c:127-130) over the 249 (nbrow - 1) + nlbyte data bytes of all rows;
 *               the run of ones carries over from row to row, as in the reference
 *   nbytes      whole un-stuffed bytes: (8 * data bytes - stuffed) / 8, rounded down; byte i is bits 8i .. 8i + 7 of that stream
 *   flag_at     the first i at which the OR of bytes 0..i equals 0x7e -- hdata[0] reaching the flag (vdlm2.c:136-139); -1: never
 *               (no bit was set at all, or a bit outside 0x7e came first)
 *   cand        calls of check_frame() (vdlm2.c:143): bytes equal to 0x7e behind hdata[1], the first byte behind flag_at that is no
 *               0x7e.  A candidate's l counts from hdata[0] to that byte, both included.
 *   too_short   of them l < 13 ("error too short");  bad_fcs  of them l >= 13 with an FCS residue other than 0xf0b8 ("error crc");
 *   frames      of them handed to out(): cand == too_short + bad_fcs + frames.  This counts every frame that checks, also one the
 *               library then drops (more than 12 in a burst, arena or caller's buffer full: vdl2gpu_stats_t.frames_dropped, *dropped).
 * status 1: nbrow outside 1..8 or nlbyte outside 0..249; the block path does not run and every other field is 0.
 * Each field is a function of the burst record alone -- or, in soft mode (a handle with VDL2GPU_F_SOFT_RS, or soft[i] given to
 * vdl2gpu_decode_blocks_report), of the record and its reliability map: integers, no order of summation to define.  A burst
 * therefore gets the same report whatever kernel, path or repair round decoded it and however the stream was cut into pushes, and
 * vdl2gpu_decode_blocks_report on polled records and maps reproduces it.  The record's data[] stays the received rows, as without
 * the flag.  Nothing else changes with the flag: records, frames, their order and every other column are what they are without it.
 * Memory: 48 bytes per record slot in each of the device output rings and each host slab, and in the host queue beside every burst
 * record it holds. */
#define VDL2GPU_F_BLOCK_REPORT 2048u
#define VDL2GPU_HAVE_BLOCK_REPORT 1
#define VDL2GPU_ROW_NONE 0
#define VDL2GPU_ROW_CLEAN 1
#define VDL2GPU_ROW_REF 2
#define VDL2GPU_ROW_SOFT2 3
#define VDL2GPU_ROW_SOFT4 4
#define VDL2GPU_ROW_FAIL 5
#define VDL2GPU_ROW_FEEDBACK 6	/* rs() returned -1 and the record's decision-feedback row replaced the row (vdl2gpu_fb_t, below); counted in rows_rescued */
typedef struct {
	int8_t row_roots[8];	/* @0  rs()'s return value for the received row; rows >= nbrow: 0 */
	uint8_t row_how[8];	/* @8  VDL2GPU_ROW_* */
	uint8_t row_changed[8];	/* @16 transmitted positions at which the decoded row differs from the received one */
	uint16_t bytes_changed;	/* @24 sum of row_changed[] */
	uint16_t rows_failed;	/* @26 rows with row_how == VDL2GPU_ROW_FAIL */
	uint16_t rows_rescued;	/* @28 rows with row_how == VDL2GPU_ROW_SOFT2, _SOFT4, _FEEDBACK or _TRACKED (vdl2gpu_trk_t, below) */
	uint16_t stuffed;	/* @30 zeros the un-stuffer dropped */
	uint16_t nbytes;	/* @32 whole un-stuffed bytes */
	int16_t flag_at;	/* @34 index of the un-stuffed byte that completes the first flag, -1: never */
	uint16_t cand;		/* @36 calls of check_frame() */
	uint16_t too_short;	/* @38 ... with l < 13 */
	uint16_t bad_fcs;	/* @40 ... with l >= 13 and the wrong FCS */
	uint16_t frames;	/* @42 ... that passed */
	int32_t status;		/* @44 0: the block path ran; 1: header out of range, all other fields 0 */
} vdl2gpu_blockrep_t;		/* sizeof 48, alignment 4 */

/* ---- decision-feedback rows (VDL2GPU_F_FEEDBACK; announced by VDL2GPU_HAVE_FEEDBACK, the ABI version is unchanged) ----
 * The reference slices every payload symbol from P_k - P_{k-1} - df (d8psk.c:213, 323-327): both phases carry their full noise.  How far
 * a slice fell from the centre of its sector says how far P_{k-1} was off, and the next slice can be told.  With VDL2GPU_F_FEEDBACK the
 * demodulator slices every payload a second time with the last three of these residuals fed back, and keeps the bytes of that second
 * slice beside the record: the record's own data[], df and every other field and column stay the reference's.
 * For an accepted burst take idx_k (0..256) for the symbols k = 8 .. kmax exactly as defined at vdl2gpu_carrier_t, n = kmax - 7:
 *   e_k  = (idx_k & 31) - 16,  S = sum e_k
 *   mbar = floor((2 S + n) / (2 n)), floor towards minus infinity: the burst's mean residual, the carrier offset df left behind
 *   r_k  = 0 for k < 8
 *   for k = 8 .. kmax in ascending order
 *          c   = 3 r_{k-1} + 2 r_{k-2} + r_{k-3}
 *          o_k = (idx_k - mbar + floor((c + 2) / 4)) mod 256, in 0..255 (floor towards minus infinity, mod non-negative)
 *          r_k = ((idx_k - 16 - 32 (o_k >> 5) - mbar + 128) mod 256) - 128, in -128..127
 *   payload bit q = 25 + 8 b + i of byte b (symbol k = q / 3, table w = q % 3) is Grey_w[o_k], descrambled and compared with 0.5 exactly as
 *   the reference path does with Grey_w[idx_k]; the bytes are assembled and scattered to (row, col) exactly as data[].  Positions that
 *   carry no transmitted byte are 0.
 * Everything is an integer: a burst gets the same vdl2gpu_fb_t whatever kernel, path or repair round decoded it and however the stream
 * was cut into pushes.  (Only idx_k mod 256 enters: idx 256, the slice at +pi, is idx 0 one turn on.)
 * Row rule of the block path when a record has feedback rows (vdl2gpu_decode_blocks_feedback; the pipeline's block path with
 * VDL2GPU_F_FRAMES | VDL2GPU_F_FEEDBACK).  Row r, its fixed erasures and p_r as at vdl2gpu_soft_t:
 *   1. the reference's rs() on the received row runs as always; a row it decodes (count >= 0) is kept as it decoded it -- no frame
 *      the reference gives is ever lost;
 *   2. otherwise rs() of fb.data[r] with the same fixed erasures; if it returns >= 0 and leaves all six syndromes zero, that row
 *      replaces the received one (VDL2GPU_ROW_FEEDBACK);
 *   3. otherwise, in soft mode, the trials of vdl2gpu_soft_t on the received row, unchanged;
 *   4. otherwise the row is what the reference left.
 * HDLC, the flag hunt and the FCS follow unchanged: the FCS still decides what is a frame.  In the block report row_roots stays the
 * reference's run on the received row, row_changed counts against the received row, rows_rescued also counts VDL2GPU_ROW_FEEDBACK.
 * The flag does not need VDL2GPU_F_FRAMES: a host-side consumer can poll the rows and use them later.
 * Memory: 2048 bytes per record slot in each of the device output rings and each host slab, and in the host queue beside every
 * burst record it holds. */
#define VDL2GPU_F_FEEDBACK 4096u
#define VDL2GPU_HAVE_FEEDBACK 1
typedef struct {
	uint8_t data[VDL2GPU_MAXROWS][VDL2GPU_ROWLEN];	/* @0    the rows of the second slice, laid out as the record's data[] */
	uint8_t reserved[8];				/* @2040 0 */
} vdl2gpu_fb_t;		/* sizeof 2048 */

/* ---- every frame of a burst (VDL2GPU_F_ALL_FRAMES; announced by VDL2GPU_HAVE_ALL_FRAMES, the ABI version is unchanged) ----
 * A burst may carry several AVLC frames, one flag closing a frame and opening the next.  blk_thread() calls check_frame() at every 0x7e
 * behind hdata[1], and check_frame() always runs the FCS from hdata[1] (vdlm2.c:52): its second candidate is "frame 1 + FCS + flag +
 * frame 2", which cannot check, so only the first frame of a burst can pass.  The block path without this flag reproduces that.
 * With VDL2GPU_F_ALL_FRAMES (which needs VDL2GPU_F_FRAMES: without it vdl2gpu_create returns VDL2GPU_EINVAL), and in
 * vdl2gpu_decode_blocks_ex with VDL2GPU_BLK_ALL_FRAMES on any handle, the block path hands on every frame of the burst.
 * Everything up to and including the flag hunt is unchanged: RS per row with the soft and feedback row rules, un-stuffing over all
 * rows, flag_at, and m1 = hdata[1] = the first byte behind the first flag that is no 0x7e.  Let B[0..nb) be the whole un-stuffed bytes
 * and q_0 < q_1 < ... the positions q >= m1 with B[q] == 0x7e.
 *   segment j   starts at s_0 = m1, s_{j+1} = q_j + 1, and is closed by q_j
 *   l_j         = q_j - s_j + 2: its length in the reference's terms -- opening flag, bytes, closing flag
 *   l_j == 2    is an empty segment (flags side by side).  It is swallowed, as the reference swallows the flags behind the first one
 *               (k == 1, vdlm2.c:134-135)
 *   passes      iff l_j >= 13 and the FCS-16 (crc.c) run from 0xffff over B[s_j .. q_j - 1] leaves 0xf0b8
 *   frame       each passing segment is one vdl2gpu_frame_t: data = 0x7e, B[s_j .. q_j], len = l_j; seq is its rank among the passing
 *               segments of its burst in stream order; all other fields are the burst's
 * Segment 0 is the reference's first candidate, so a burst of one frame gives the same frame with or without the flag.  The
 * reference's FURTHER candidates (all of them starting at m1, passing only by an accident of 2^-16 each) are not formed in this mode.
 * One thing follows from working on B, as the reference does: the un-stuffer hands a stuffed data byte 0x7e on as the byte 0x7e, and
 * the rule takes it for a flag (so does check_frame()'s caller, vdlm2.c:143, where it only adds a candidate that fails).  A frame that
 * holds a data byte 0x7e is therefore cut there in this mode and does not pass, not even as the first frame of its burst, which the
 * block path without the flag delivers.  A consumer that must not lose those sets VDL2GPU_F_RAW_FLAGS as well (below).
 * As without the flag: at most 12 passing frames of a burst are kept, the first 12 in stream order, and further ones are counted in
 * vdl2gpu_stats_t.frames_dropped / *dropped; bytes behind the last flag are ignored; nothing is re-aligned at bit level -- flags
 * survive the un-stuffer and frames are whole bytes, so byte alignment holds across the frames of a burst.
 * The block report (vdl2gpu_blockrep_t, layout unchanged) in this mode: cand keeps its meaning, every 0x7e behind hdata[1]; too_short
 * counts l_j < 13, the empty segments of l_j = 2 included; bad_fcs counts l_j >= 13 with another residue; frames counts those that
 * pass; cand == too_short + bad_fcs + frames still holds.
 * Nothing else changes with the flag: burst records, their order and every column are what they are without it, and
 * vdl2gpu_poll_frames keeps its order (end_dec, stream, chn, seq). */
#define VDL2GPU_F_ALL_FRAMES 8192u
#define VDL2GPU_HAVE_ALL_FRAMES 1

/* ---- a flag is six adjacent ones (VDL2GPU_F_RAW_FLAGS; announced by VDL2GPU_HAVE_RAW_FLAGS, the ABI version is unchanged) ----
 * A mode of VDL2GPU_F_ALL_FRAMES (vdl2gpu_create returns VDL2GPU_EINVAL for this flag without that one), and in
 * vdl2gpu_decode_blocks_ex VDL2GPU_BLK_RAW_FLAGS beside VDL2GPU_BLK_ALL_FRAMES on any handle.  It tells a flag from a stuffed data
 * byte 0x7e, which the rule above cannot, by looking at the stuffed bit stream.
 * The reference's un-stuffing loop (vdlm2.c:119-133) keeps t, the run of ones in front of the bit it reads; a zero read with t == 5 is
 * dropped.  Every whole un-stuffed byte B[q] ends with its bit 7; where B[q] == 0x7e that bit is a zero that is kept.  Let t7[q] be t
 * when that zero is read.
 *   true flag     F[q] = (B[q] == 0x7e && t7[q] == 6): written "t == 6" -- the six ones are adjacent in the stuffed stream
 *   data byte     a data byte 0x7e was sent as 0 11111 0 1 0; the zero behind its fifth one is dropped, so t7[q] == 1.  (The only place
 *                 a zero can be dropped inside a byte that un-stuffs to 0x7e is between its bits 5 and 6: "a zero was dropped at
 *                 un-stuffed bit offset 8q + 6" is the same statement as !F[q] for such a byte.)
 * The rule of VDL2GPU_F_ALL_FRAMES then holds with F[q] in place of B[q] == 0x7e, in two places:
 *   m1            is the first q > flag_at with !F[q] (not "the first byte that is no 0x7e": a frame that begins with a data byte 0x7e
 *                 keeps that byte).  flag_at itself is unchanged, the prefix OR reaching 0x7e
 *   segments      q_0 < q_1 < ... are the positions q >= m1 with F[q]; s_0, s_{j+1}, l_j, "passes", seq, the first 12 kept and
 *                 frames_dropped are as above.  The frame is 0x7e, B[s_j .. q_j]: un-stuffed bytes, data bytes 0x7e among them
 * The block report in this mode: cand counts the true flags at q >= m1; too_short, bad_fcs and frames follow those segments;
 * cand == too_short + bad_fcs + frames still holds; every field in front of cand (the rows, stuffed, nbytes, flag_at, status) is what it
 * is without the mode.
 * A burst without a data byte 0x7e between its flags gives the same frames and the same report with and without this mode.  Nothing is
 * re-aligned at bit level, as before: a flag that does not end on a byte boundary of B is not seen. */
#define VDL2GPU_F_RAW_FLAGS 16384u
#define VDL2GPU_HAVE_RAW_FLAGS 1

/* ---- symbol timing, clock drift and fine arrival time (VDL2GPU_F_SYMCLK; announced by VDL2GPU_HAVE_SYMCLK, the ABI version is unchanged) ----
 * A burst record says when the burst arrived as trig_dec and the one-shot sub-phase of the 16 sync symbols: a quarter of an 84 kS/s
 * sample, 3 us.  It says nothing of how fast the transmitter's symbol clock runs against the receiver's sample clock (VDL2 allows
 * +-50 ppm, an uncorrected receiver adds 30 .. 100).  With VDL2GPU_F_SYMCLK the GPU measures both over the whole burst with the
 * square-law (Oerder-Meyr) timing estimator at the plane's 8 samples per symbol.  It is not decision-directed and always uses
 * sub-phase 0: the result does not depend on clk0, on the slicer or on any other flag, and nothing else changes with the flag.
 * Notation as at vdl2gpu_level_t: S(n, c) the channel-filtered value at stream time n, sub-phase c.  For an accepted burst with header
 * values nbrow, nlbyte and last symbol end_dec:
 *   nsym            as at vdl2gpu_level_t (the byte schedule of d8psk.c:117-206: (25 + 8 (ND + NF) + 2) / 3 with ND, NF as at
 *                   vdl2gpu_carrier_t), sym_first_dec = end_dec - 8 (nsym - 1), n_k = sym_first_dec + 8 k for k = 0 .. nsym - 1
 *   segments        segment s holds the symbols k in [256 s, min(nsym, 256 s + 256)); nseg = ceil(nsym / 256), at most
 *                   VDL2GPU_SYMCLK_SEGS = 22 (the longest burst has 5449 symbols)
 *   sums            e[s][d] = sum over the segment's k of |S(n_k - d, 0)|^2, d = 0 .. 7, in float; e[s][] = 0 for s >= nseg.
 *                   S is formed in float with the taps in ascending order (j = 0 .. 16, real and imaginary part each a chain of
 *                   multiply, then add: no fused operation), |S|^2 = re * re + im * im.
 *                   The oldest sample touched is sym_first_dec - 23, the newest end_dec: inside what the sync detector and the
 *                   payload decode of the burst have read, never past end_dec -- the result cannot depend on where the stream was cut.
 *   order           of the sum over k: value v[l] of symbol k = 256 s + l for l = 0 .. 255, 0.0f where k >= nsym; four groups of 64
 *                   (l / 64); in each group the xor butterfly v[l] += v[l ^ 32], then ^ 16, 8, 4, 2, 1 (every l of the group ends
 *                   with the same sum); e[s][d] = ((g0 + g1) + g2) + g3.  A burst therefore gets bit-identical sums whatever
 *                   kernel, path or repair round decoded it and however the stream was cut into pushes.
 * The host derives the rest in double precision (vdl2gpu_symclk_from_sums is that arithmetic, and what the library itself calls):
 *   z_s       = sum_d e[s][d] * exp(+2 pi i d / 8)
 *   tau_s     = -(4 / pi) * arg z_s (atan2; + 8 where that gives -4 or less), in 84 kS/s samples, in (-4, 4].  Positive: the symbol
 *               centres lie LATER than the grid n_k.  For s >= 1 tau_s is then unwrapped: 8 is added or subtracted until
 *               tau_s - tau_{s-1} lies in (-4, 4]
 *   line      weighted least squares tau(k) = tau0 + slope * k through the points (c_s, tau_s), c_s = 256 s + (m_s - 1) / 2 the centre
 *               symbol index and the weight m_s the symbol count of segment s
 *   tau0      the line at k = 0;  clock_ppm = -slope / 8 * 1e6: POSITIVE when the transmitter's symbols come FASTER than 10 500 a
 *               second as counted by the receiver's sample clock;  tau_rms = sqrt(sum m_s r_s^2 / sum m_s), r_s the segments'
 *               residuals about the line.  With nseg == 1: tau0 = tau_0, clock_ppm and tau_rms are NaN
 *   toa_sample = (sym_first_dec + tau0 - D + 0.5) * sdrinrate / 84000 - 0.5 (tau0 before it is narrowed to float): the time, in INPUT
 *               samples of the stream, of the centre of symbol k = 0 -- the first symbol behind the 17 of the unique word (reference
 *               symbol + 16), symbol 21 counted from a transmitter's first ramp symbol with 4 ramp symbols.
 *               D = sum_j (16 - j) mflt[4 j] / sum_j mflt[4 j] (j = 0 .. 16) is the centroid delay of the sub-phase-0 taps; mflt is not
 *               symmetric, D is 8.2509, not 8.  The linear map is the mean of the dump schedule (d8psk.c:374-381: output m averages
 *               the inputs [m M, (m + 1) M), M = sdrinrate / 84000, so its centre is input (m + 0.5) M - 0.5).  With VDL2GPU_F_RTL_QUIRK
 *               the map to input samples does NOT hold (every block of 32768 is shifted by one and loses a sample): toa_sample is then
 *               a time in the quirk's own sample count.
 * Accuracy, measured with these formulas in float64 on the CPU model's planes against a synthetic transmitter's truth (cs16 at 2 and
 * 10 MS/s, cu8 at 2 MS/s; 24 bursts of 123 .. 4561 symbols at a random fraction of a symbol; noise 1.7; symbol clock 0, +50, -30 ppm;
 * scripts/symclk_accuracy.py, profiles/r24_symclk_accuracy.txt):
 *   toa_sample  within 0.527 us of the true centre of symbol k = 0.  The error is not centred: mean -0.222 us (a sixtieth of an 84 kS/s
 *               sample; -0.29 / -0.12 / -0.25 us for the three inputs) against a standard deviation of 0.07 .. 0.14 us, with D derived as
 *               above, not fitted -- stated, not absorbed.  Stations that compare arrival times of one burst share the offset
 *   clock_ppm   within 0.319 ppm with nseg >= 10, within 1.386 ppm with 3 <= nseg < 10; with nseg == 2 the line goes through its two
 *               points (tau_rms is 0) and the error reaches 19 ppm; with nseg == 1 there is none
 * The GPU's plane is that model's bit for bit and its sums agree with float64 to 1e-5, so it inherits these errors; the tests bound it
 * by twice the worst of that table (other seeds): 1.054 us, 0.638 ppm, 2.772 ppm.
 * Memory: 744 bytes per record slot wherever a level record has 40 -- each device output ring, each host slab, and the host queue
 * beside every burst record it holds. */
#define VDL2GPU_F_SYMCLK 32768u
#define VDL2GPU_HAVE_SYMCLK 1
#define VDL2GPU_SYMCLK_SEG 256		/* symbols per segment */
#define VDL2GPU_SYMCLK_SEGS 22		/* ceil(5449 / 256): covers a burst of VDL2GPU_MAXROWS rows */
typedef struct {
	int64_t sym_first_dec;	/* @0  stream time (84 kS/s) of the first symbol evaluation, n_0 */
	int32_t nsym;		/* @8  symbols of the burst */
	int32_t nseg;		/* @12 segments used, ceil(nsym / 256) */
	double toa_sample;	/* @16 input-sample time of the centre of symbol k = 0 */
	float tau0;		/* @24 the fitted line at k = 0, 84 kS/s samples */
	float clock_ppm;	/* @28 symbol clock against the sample clock; NaN with nseg == 1 */
	float tau_rms;		/* @32 weighted rms residual of the segments about the line; NaN with nseg == 1 */
	int32_t reserved;	/* @36 0 */
	float e[VDL2GPU_SYMCLK_SEGS][8];	/* @40 the sums; 40 + 22 * 32 = 744 is a multiple of 8: no padding */
} vdl2gpu_symclk_t;		/* sizeof 744, alignment 8 */

/* ---- timing-tracked rows (VDL2GPU_F_TRACKED; announced by VDL2GPU_HAVE_TRACKED, the ABI version is unchanged) ----
 * The reference takes a burst's symbol timing once, from the 16 symbols of the unique word, and keeps it to the burst's last symbol
 * (d8psk.c:281-319).  VDL Mode 2 allows a transmitter's symbol clock +-50 ppm and an uncorrected receiver adds its own: over the 5446
 * symbols of the longest burst the sampling instant walks a quarter of a symbol, and since bursts are interleaved by column the damaged
 * tail is the last columns of EVERY RS row.  With VDL2GPU_F_TRACKED the GPU slices every payload a second time, in segments of 256
 * symbols whose sampling instant may move by a quarter of an 84 kS/s sample from one segment to the next, and keeps the bytes of that
 * slice beside the record: the record's own data[], df and every other field and column stay the reference's.  The flag needs no other
 * flag and changes nothing else.
 * Notation as at vdl2gpu_carrier_t.  For an accepted record with nbrow, nlbyte, df, end_dec:
 *   ND, NF       the data and FEC bytes, kmax = (25 + 8 (ND + NF) - 1) / 3; the payload symbols are k = 8 .. kmax, n = kmax - 7 of them;
 *                symbol k lies at stream time t_k = end_dec - 8 (kmax - k) (that is trig_dec + j0 + 8 k)
 *   positions    are counted in quarter samples.  P(u) is filteredphase() (d8psk.c:219-230) at stream time m = ceil(u / 4) and sub-phase
 *                c = 4 m - u (taps mflt[c], mflt[c + 4], ... on the samples m - 16, m - 15, ...: float sums, oldest sample first, multiply
 *                then add, then atan2f -- exactly as the payload decode forms its phases).  The reference's own slices are P(4 t_k - rb).
 *                Samples at stream times GREATER THAN end_dec count as 0, whatever the stream holds there (only the burst's last symbol
 *                can reach them, and only with d > 0): the record does not depend on where the stream was cut
 *   segments     symbol index i = k - 8; segment s holds i in [256 s, min(n, 256 s + 256)); nseg = ceil(n / 256), at most 22
 *   hypothesis   d of segment s: for each of its symbols idx_k(d) = the Grey table index (d8psk.c:213, 323-327, in 0..256) of
 *                P(4 t_k + d) against P(4 t_{k-1} + d) with the record's df -- both phases with the same d, also for the segment's first
 *                symbol; e = (idx & 31) - 16; the cost C_s(d) = sum of e^2 over the segment's symbols, an integer
 *   choice       segment 0 tries d = 0, -1, -2, -3 in that order; segment s >= 1 tries d_{s-1}, d_{s-1} - 1, d_{s-1} + 1 in that order; a
 *                later candidate wins only with a strictly smaller cost.  One step per 256 symbols follows up to 122 ppm
 *   bytes        idx_k = idx_k(d_s) of the symbol's segment; payload bit q = 25 + 8 b + i of byte b is Grey_{q % 3}[idx_{q / 3}], descrambled
 *                and compared with 0.5 exactly as the reference path does; the bytes are assembled and scattered to (row, col) exactly as
 *                vdl2gpu_fb_t.data is.  Positions that carry no transmitted byte are 0
 *   d_first, d_last, d_min, d_max   d_0, d_{nseg-1}, and the least and greatest d_s of the burst
 * A record that is none has all zeros.  Everything chosen is an integer over bit-exact phases: a burst gets the same vdl2gpu_trk_t
 * whatever kernel, path or repair round decoded it and however the stream was cut into pushes.
 * The block path with tracked rows (the pipeline's with VDL2GPU_F_FRAMES | VDL2GPU_F_TRACKED; vdl2gpu_decode_blocks_tracked on any
 * handle) makes a second attempt PER BURST, not per row: RS(255,249) with three correctable errors "decodes" a garbage row to a wrong
 * codeword about one time in six, such a row would stay in place under a per-row rule, and the FCS then fails.
 *   attempt A    the block path exactly as the other flags and the mode define it.  If one or more of its candidates pass, its frames and
 *                its report are the result: no frame delivered without the flag is ever lost
 *   attempt B    only when A passed none.  For each row r: rs() of trk.data[r] with the row's fixed erasures; if it returns >= 0 and
 *                leaves all six syndromes zero, that row is taken (VDL2GPU_ROW_TRACKED), otherwise the row is what A's row rule left.
 *                If no row is taken B ends here.  Then un-stuffing, the flag hunt and the FCS, as the mode says
 *   result       if B passes one or more candidates: B's frames and B's whole report; otherwise A's -- no frames, and A's report.
 * The report's layout is unchanged: row_roots stays the reference's run on the received row, row_changed counts against the received
 * row, rows_rescued also counts VDL2GPU_ROW_TRACKED.  A second attempt gives the FCS's 2^-16 chance of passing a wrong candidate twice.
 * Memory: 2048 bytes per record slot in each of the device output rings and each host slab, and in the host queue beside every
 * burst record it holds. */
#define VDL2GPU_F_TRACKED 65536u
#define VDL2GPU_HAVE_TRACKED 1
#define VDL2GPU_TRK_SEG 256		/* symbols per segment */
#define VDL2GPU_TRK_SEGS 22		/* covers a burst of VDL2GPU_MAXROWS rows */
#define VDL2GPU_ROW_TRACKED 7		/* block report, row_how: attempt B took the record's timing-tracked row; counted in rows_rescued */
typedef struct {
	uint8_t data[VDL2GPU_MAXROWS][VDL2GPU_ROWLEN];	/* @0    the rows of the tracked slice, laid out as the record's data[] */
	int8_t d_first, d_last, d_min, d_max;		/* @2040 quarter samples: d_0, d_{nseg-1}, min and max over the segments */
	uint8_t nseg;					/* @2044 segments used, ceil(n / 256) */
	uint8_t reserved[3];				/* @2045 0 */
} vdl2gpu_trk_t;		/* sizeof 2048 */

typedef struct {
	uint64_t samples_in;	/* per stream */
	uint64_t dec_samples;	/* 84 kS/s samples produced per channel */
	uint64_t sync_evals;	/* WSYNC evaluations, all channels */
	uint64_t triggers;	/* sync triggers */
	uint64_t header_rejects;	/* d8psk.c:97-107 */
	uint64_t bursts;	/* records handed out */
	uint64_t deferrals;	/* bursts that waited for a later push to complete */
	uint64_t candidates;	/* sync-trigger candidates found by the parallel scan (all timing hypotheses) */
	uint64_t serial_redos;	/* channel-pushes redone serially because the verify pass found an unlisted event */
	uint64_t serial_samples;	/* 84 kS/s samples handled by the serial machine (history-dependent stretches) */
	uint64_t overflowed;	/* burst records dropped: device ring full, or host queue never drained */
	uint64_t frames_dropped;	/* VDL2GPU_F_FRAMES: frames that checked and were not handed out: more than 12 in one burst (with VDL2GPU_F_ALL_FRAMES the
				 * 13th passing segment onwards, in stream order), the device's frame arena full, or the host queue never drained */
	uint64_t repairs;	/* channel-pushes a repair round re-resolved because the verify pass found an unlisted event (cheap; serial_redos
				 * counts the ones no scheduled round could settle) */
} vdl2gpu_stats_t;

typedef struct {
	double channelise_ms;	/* sum over pushes of the channeliser kernels (HIP events on every stage_every-th push, scaled to all) */
	double demod_ms;	/* sum of the demodulator kernels (scan + cluster + resolve) */
	double scan_ms;		/* K2a sync scan */
	double cluster_ms;	/* K2b burst clusters */
	double resolve_ms;	/* K2c resolver + K2d gather */
	double other_ms;	/* compaction / bookkeeping kernels */
	double channelise_fast_ms;	/* the k1_fast launches alone (2 MS/s path): sum over fast_pushes launches */
	uint64_t fast_pushes;	/* number of fast-kernel launches behind channelise_fast_ms (the timed ones) */
	uint64_t pushes;
	uint64_t samples;	/* input samples per stream covered by the sums */
} vdl2gpu_timing_t;

typedef struct vdl2gpu vdl2gpu_t;

int vdl2gpu_abi_version(void);
int vdl2gpu_create(const vdl2gpu_config_t *cfg, vdl2gpu_t **out);
void vdl2gpu_destroy(vdl2gpu_t *h);

/* ---- Threads ------------------------------------------------------------------------------------------------
 * A handle may be used from several threads at once.  The reference has a producer thread -- the SDR library's callback,
 * in_callback() under rtlsdr_read_async() (rtl.c:274-295, 302) / rx_callback() (air.c:191-217) -- and consumer threads behind
 * it (main.c:225-231, vdlm2.c:84); a shim built on this library keeps that shape on ONE handle:
 *   - every call that takes a vdl2gpu_t* locks the handle for its duration; calls from different threads are serialised, none is
 *     lost, and each burst / frame record is handed out exactly once, whichever thread asks;
 *   - PRODUCER side: vdl2gpu_push(), or vdl2gpu_ring_acquire() / vdl2gpu_ring_commit().  One producer at a time: acquire and
 *     commit alternate, and pushes are decoded in the order the calls were made.  A producer call holds the lock while it
 *     enqueues (~0.1 ms) and, when three pushes are already in the pipeline, while it waits for the oldest of them;
 *   - CONSUMER side: vdl2gpu_poll_ready() / vdl2gpu_poll_frames_ready() never wait.  vdl2gpu_poll(), vdl2gpu_poll_frames() and
 *     vdl2gpu_pending() wait for everything that was pushed BEFORE the call -- with the lock released while they wait for the
 *     GPU, so a producer thread keeps committing blocks meanwhile (what it commits after the call began is not waited for);
 *   - per (stream, channel) the bursts come out in time order across calls, as decodeVdlm2() receives them (d8psk.c:201);
 *   - vdl2gpu_sync(), vdl2gpu_get_stats(), vdl2gpu_get_timing() and the vdl2gpu_debug_*() calls drain the pipeline under the
 *     lock: fine from any thread, but they hold the others up for that long;
 *   - vdl2gpu_last_error()'s string is valid until the next call on the handle from any thread;
 *   - vdl2gpu_destroy() must not run beside any other call on the handle (join the threads first);
 *   - different handles share nothing.
 * tests/ctests/thread_stress.c is this shape (one pthread committing ring slots, one collecting), held to the oracle ten times
 * over by tests/test_gpu_dropin.py. */

/* Feed `nsamples` samples of every stream.  Stream s starts at
 * (const char*)iq + s*stream_stride_bytes.  Asynchronous: returns once the
 * work is enqueued on the handle's HIP stream.  Replaces one Bar2/Bar1
 * hand-off of Cbuff (d8psk.c:360-383) for all channels at once, with any
 * block length instead of the fixed 32768.
 * Buffer lifetime: a VDL2GPU_MEM_HOST buffer may be reused as soon as the call returns (it has been copied).
 * A VDL2GPU_MEM_DEVICE buffer is read in place by the channeliser, asynchronously: it must stay valid and
 * unchanged until the second push after this one has been issued, or until vdl2gpu_sync() / vdl2gpu_poll()
 * returns -- whichever comes first (three pushes can be in the pipeline; the call that issues the second push after this one
 * waits until this one's channeliser has read the buffer).
 * Errors are sticky: after a call has returned VDL2GPU_EHIP the handle only accepts vdl2gpu_destroy(). */
int vdl2gpu_push(vdl2gpu_t *h, const void *iq, size_t nsamples, size_t stream_stride_bytes, int memkind);

/* Ingest ring: replaces the producer side of the hand-off -- in_callback()
 * converting a USB block into Cbuff between Bar1 and Bar2 (rtl.c:274-295), rx_callback() copying airspy
 * samples (air.c:191-217) -- by `nslots` slots of page-locked host memory that the producer fills in place
 * (e.g. rtlsdr_read_sync() straight into the slot; the cu8/cs16 conversion happens in the channeliser
 * kernel).  acquire() hands out the next slot -- stream s starts at slot + s * *stream_stride_bytes -- and
 * waits only if that slot's previous contents are still on their way to the GPU; commit(nsamples) enqueues
 * the copy and the whole decode behind it and returns at once, so the copy of one block runs beside the
 * kernels of the one before.  commit(0) drops the block (a short USB read, rtl.c:278-281).  One producer:
 * acquire and commit alternate.  Bursts come out through vdl2gpu_poll*() as with vdl2gpu_push(). */
int vdl2gpu_ring_init(vdl2gpu_t *h, size_t slot_samples, int nslots);
void *vdl2gpu_ring_acquire(vdl2gpu_t *h, size_t *stream_stride_bytes);
int vdl2gpu_ring_commit(vdl2gpu_t *h, size_t nsamples);
/* Wait until everything pushed so far has been demodulated. */
int vdl2gpu_sync(vdl2gpu_t *h);
/* Collect finished bursts (waits for everything pushed so far).  Bursts come out ordered by
 * (end_sample, stream, chn).  Returns the count (>=0) or a negative error.
 * The host keeps what has been fetched from the GPU and not yet handed out in two bounded queues (bursts;
 * with VDL2GPU_F_FRAMES also frames): a consumer that drains only one of them loses the OLDEST entries of the
 * other (counted in vdl2gpu_stats_t.overflowed / frames_dropped).  The bound is applied when a push is collected, BEFORE
 * its entries join the queue: what is unread then is cut to the newest 4 x max_bursts, and the push's own entries come on
 * top -- a queue never holds more than 4 x max_bursts + one push's entries, and never loses an entry while it holds
 * 4 x max_bursts or fewer.  Memory: the storage behind a queue is compacted as soon as its handed-out prefix is the larger part,
 * so it holds at most 2 x the unread records plus one push's worth -- <= 9 x max_bursts records of 2104 bytes
 * (1.2 GB with the default max_bursts = 65536 and a consumer that never polls; a few MB with one that does). */
int vdl2gpu_poll(vdl2gpu_t *h, vdl2gpu_burst_t *out, int max);
/* Same, but never waits: hands out only the bursts of pushes the GPU has already finished.  Lets
 * a caller keep the next pushes running while it consumes the earlier ones (three pushes can be in the pipeline;
 * a fourth first collects the oldest). */
int vdl2gpu_poll_ready(vdl2gpu_t *h, vdl2gpu_burst_t *out, int max);
/* vdl2gpu_poll / vdl2gpu_poll_ready with the bursts' levels: lv[i] belongs to out[i].  Same queue, order, waiting and threading:
 * each burst is handed out once, whichever of the four calls takes it.  lv == NULL: exactly the plain call.  lv != NULL on a handle
 * created without VDL2GPU_F_LEVELS: VDL2GPU_EINVAL, and nothing is consumed. */
int vdl2gpu_poll_levels(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, int max);
int vdl2gpu_poll_levels_ready(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, int max);
/* The same with the bursts' reliability maps as well: soft[i] belongs to out[i] (VDL2GPU_F_SOFT_RS).  lv and soft may each be NULL;
 * lv != NULL without VDL2GPU_F_LEVELS or soft != NULL without VDL2GPU_F_SOFT_RS: VDL2GPU_EINVAL, and nothing is consumed.  The
 * host queue holds a map beside every unread burst: with the flag, 2048 more bytes per record of the bound above. */
int vdl2gpu_poll_soft(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, int max);
int vdl2gpu_poll_soft_ready(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, int max);
/* ... and with the bursts' carrier records: car[i] belongs to out[i] (VDL2GPU_F_CARRIER).  Same queue, order, waiting and threading as
 * the other collectors; each of lv, soft and car may be NULL (all three: exactly vdl2gpu_poll).  car != NULL on a handle created
 * without VDL2GPU_F_CARRIER: VDL2GPU_EINVAL, and nothing is consumed; lv and soft as above. */
int vdl2gpu_poll_carrier(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, int max);
int vdl2gpu_poll_carrier_ready(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, int max);
/* ... and with the bursts' block reports: rep[i] belongs to out[i] (VDL2GPU_F_BLOCK_REPORT).  Same queue, order, waiting and threading
 * as the other collectors; each of lv, soft, car and rep may be NULL (rep == NULL: exactly vdl2gpu_poll_carrier).  rep != NULL on a
 * handle created without VDL2GPU_F_BLOCK_REPORT: VDL2GPU_EINVAL, and nothing is consumed; lv, soft and car as above. */
int vdl2gpu_poll_report(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, vdl2gpu_blockrep_t *rep, int max);
int vdl2gpu_poll_report_ready(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, vdl2gpu_blockrep_t *rep, int max);
/* ... and with the bursts' decision-feedback rows: fb[i] belongs to out[i] (VDL2GPU_F_FEEDBACK).  Same queue, order, waiting and threading
 * as the other collectors; each of lv, soft, car, rep and fb may be NULL (fb == NULL: exactly vdl2gpu_poll_report).  fb != NULL on a
 * handle created without VDL2GPU_F_FEEDBACK: VDL2GPU_EINVAL, and nothing is consumed; lv, soft, car and rep as above. */
int vdl2gpu_poll_feedback(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, vdl2gpu_blockrep_t *rep,
			  vdl2gpu_fb_t *fb, int max);
int vdl2gpu_poll_feedback_ready(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, vdl2gpu_blockrep_t *rep,
				vdl2gpu_fb_t *fb, int max);
/* ... and with the bursts' symbol-clock records: clk[i] belongs to out[i] (VDL2GPU_F_SYMCLK).  Same queue, order, waiting and threading
 * as the other collectors; each of lv, soft, car, rep, fb and clk may be NULL (clk == NULL: exactly vdl2gpu_poll_feedback).  clk != NULL
 * on a handle created without VDL2GPU_F_SYMCLK: VDL2GPU_EINVAL, and nothing is consumed; the others as above. */
int vdl2gpu_poll_symclk(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, vdl2gpu_blockrep_t *rep,
			vdl2gpu_fb_t *fb, vdl2gpu_symclk_t *clk, int max);
int vdl2gpu_poll_symclk_ready(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, vdl2gpu_blockrep_t *rep,
			      vdl2gpu_fb_t *fb, vdl2gpu_symclk_t *clk, int max);
/* ... and with the bursts' timing-tracked rows: trk[i] belongs to out[i] (VDL2GPU_F_TRACKED).  Same queue, order, waiting and threading
 * as the other collectors; each of lv, soft, car, rep, fb, clk and trk may be NULL (trk == NULL: exactly vdl2gpu_poll_symclk).  trk != NULL
 * on a handle created without VDL2GPU_F_TRACKED: VDL2GPU_EINVAL, and nothing is consumed; the others as above. */
int vdl2gpu_poll_tracked(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, vdl2gpu_blockrep_t *rep,
			 vdl2gpu_fb_t *fb, vdl2gpu_symclk_t *clk, vdl2gpu_trk_t *trk, int max);
int vdl2gpu_poll_tracked_ready(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, vdl2gpu_blockrep_t *rep,
			       vdl2gpu_fb_t *fb, vdl2gpu_symclk_t *clk, vdl2gpu_trk_t *trk, int max);
/* Number of bursts a poll would currently return (implies vdl2gpu_sync). */
int vdl2gpu_pending(vdl2gpu_t *h);
/* Pushes the GPU has not finished yet (0..3); never waits.  For a producer that is not bound to real time and wants to
 * size its pushes by what the pipeline can take (a push of a million samples costs the calling thread the same 0.1 ms to enqueue
 * as one of 32768). */
int vdl2gpu_inflight(vdl2gpu_t *h);

int vdl2gpu_get_stats(vdl2gpu_t *h, vdl2gpu_stats_t *out);
int vdl2gpu_get_timing(vdl2gpu_t *h, vdl2gpu_timing_t *out, int reset);
/* Where the calling thread's time inside vdl2gpu_push() went (host bookkeeping: no pipeline drain), seconds summed since the last
 * reset: out8[0] waiting for the device buffer of the push before last; [1] enqueueing the channeliser; [2] collecting the output
 * ring this push reuses (mostly WAITING for the push three back to finish: the GPU is the slower side then); [3] enqueueing the rest
 * of the front stage; [4] moving uncollected records out of the slab's way; [5] enqueueing the back stage and the tail; [6] (part of
 * [2] and of the polling calls) waiting for a ring's completion event; [7] the pushes counted.  Replaces nothing of the reference. */
int vdl2gpu_get_host_profile(vdl2gpu_t *h, double *out8, int reset);
/* h == NULL: why the calling thread's last vdl2gpu_create refused its configuration, where it says (a static string; today
 * VDL2GPU_F_BLOCK_REPORT without VDL2GPU_F_FRAMES), else "null handle". */
const char *vdl2gpu_last_error(vdl2gpu_t *h);
const char *vdl2gpu_strerror(int code);

/* Fill a reference msgblk_t (vdlm2.h:39-47, LP64 layout: prev@0 chn@8 Fr@12
 * tv@16 ppm@32 nbrow@36 nlbyte@40 data@44, sizeof 16624 -- the x86-64 / aarch64 Linux layout; the offsets
 * are compile-time constants of this library, so a host with another ABI must copy the fields itself)
 * from a burst record.  `msgblk` must point at sizeof(msgblk_t) zeroed bytes (calloc, as vdlm2.c:201);
 * msgblk_size is checked against 16624. */
#define VDL2GPU_MSGBLK_OFF_CHN 8
#define VDL2GPU_MSGBLK_OFF_FR 12
#define VDL2GPU_MSGBLK_OFF_TV 16
#define VDL2GPU_MSGBLK_OFF_PPM 32
#define VDL2GPU_MSGBLK_OFF_NBROW 36
#define VDL2GPU_MSGBLK_OFF_NLBYTE 40
#define VDL2GPU_MSGBLK_OFF_DATA 44
#define VDL2GPU_MSGBLK_SIZE 16624	/* oracle/ref_layout_check.c holds these against offsetof(msgblk_t, ..) of the reference's own vdlm2.h
					 * with _Static_assert: `make -C oracle ref` fails if they ever disagree */
int vdl2gpu_burst_to_msgblk(const vdl2gpu_burst_t *b, void *msgblk, size_t msgblk_size);

/* ---- block path: what the reference's blk_thread does with a msgblk_t ----
 * vdlm2.c:84-161 -- RS(255,249) of every row (rs.c), HDLC bit un-stuffing, flag hunt, check_frame()
 * (length >= 13, FCS-16 of crc.c) -- for a whole batch of bursts in one kernel.  One record per
 * frame the reference would pass to out(msgblk_t*, unsigned char *hdata, int l) (vdlm2.h:134):
 * data[0..len) is hdata, the other fields are the msgblk_t's.  Frames come out ordered by
 * (block, seq).  At the rates this library demodulates at, the reference's single blk_thread is
 * the bottleneck; a shim can call this instead of decodeVdlm2() and go to out(). */
#define VDL2GPU_MAXFRAME 2000
typedef struct {
	int32_t stream, chn, Fr;	/* of the burst the frame came in */
	int32_t nbrow, nlbyte;
	int32_t len;			/* l of out(): opening flag .. closing flag */
	int32_t block;			/* index of the burst in the batch */
	int32_t seq;			/* 0 for the burst's first frame, ... */
	float df, ppm;
	int64_t trig_dec, end_dec;
	uint8_t data[VDL2GPU_MAXFRAME];	/* hdata[0..len) */
} vdl2gpu_frame_t;
/* Decode `n` bursts (host array, e.g. straight from vdl2gpu_poll) into CRC-clean frames.
 * Returns the number of frames (<= max_frames; more are dropped and counted in *dropped if given)
 * or a negative error. */
int vdl2gpu_decode_blocks(vdl2gpu_t *h, const vdl2gpu_burst_t *blocks, int n,
			  vdl2gpu_frame_t *frames, int max_frames, int *dropped);
/* The same in soft mode: soft[i] is the reliability map of blocks[i] (vdl2gpu_poll_soft), and rows the reference cannot decode go
 * through the row rule of vdl2gpu_soft_t.  Works on any handle; soft == NULL: exactly vdl2gpu_decode_blocks. */
int vdl2gpu_decode_blocks_soft(vdl2gpu_t *h, const vdl2gpu_burst_t *blocks, const vdl2gpu_soft_t *soft, int n,
			       vdl2gpu_frame_t *frames, int max_frames, int *dropped);
/* ... and with the block reports (vdl2gpu_blockrep_t): rep[i] belongs to blocks[i], n of them, whatever becomes of the frames (also
 * with max_frames == 0).  Works on any handle; soft may be NULL (hard mode); rep == NULL: exactly vdl2gpu_decode_blocks_soft. */
int vdl2gpu_decode_blocks_report(vdl2gpu_t *h, const vdl2gpu_burst_t *blocks, const vdl2gpu_soft_t *soft, int n,
				 vdl2gpu_frame_t *frames, int max_frames, int *dropped, vdl2gpu_blockrep_t *rep);
/* ... and with decision-feedback rows: fb[i] belongs to blocks[i] (vdl2gpu_poll_feedback), and rows the reference cannot decode go through
 * the row rule of vdl2gpu_fb_t.  Works on any handle; soft and rep may each be NULL; fb == NULL: exactly vdl2gpu_decode_blocks_report. */
int vdl2gpu_decode_blocks_feedback(vdl2gpu_t *h, const vdl2gpu_burst_t *blocks, const vdl2gpu_soft_t *soft, const vdl2gpu_fb_t *fb, int n,
				   vdl2gpu_frame_t *frames, int max_frames, int *dropped, vdl2gpu_blockrep_t *rep);
/* ... and with a mode word (announced by VDL2GPU_HAVE_ALL_FRAMES), so that a further mode needs no further name.
 * VDL2GPU_BLK_ALL_FRAMES: every frame of a burst, by the rule at VDL2GPU_F_ALL_FRAMES.  Works on any handle; soft, fb and rep may each be
 * NULL; mode == 0: exactly vdl2gpu_decode_blocks_feedback.
 * VDL2GPU_BLK_ALL_FRAMES | VDL2GPU_BLK_RAW_FLAGS (announced by VDL2GPU_HAVE_RAW_FLAGS): that with the rule at VDL2GPU_F_RAW_FLAGS.
 * The mode word is 0, 1 or 5; every other value -- VDL2GPU_BLK_RAW_FLAGS alone, bit 1 (unassigned), any higher bit -- is VDL2GPU_EINVAL
 * before any device call. */
#define VDL2GPU_BLK_ALL_FRAMES 1u
#define VDL2GPU_BLK_RAW_FLAGS 4u
int vdl2gpu_decode_blocks_ex(vdl2gpu_t *h, const vdl2gpu_burst_t *blocks, const vdl2gpu_soft_t *soft, const vdl2gpu_fb_t *fb, int n,
			     vdl2gpu_frame_t *frames, int max_frames, int *dropped, vdl2gpu_blockrep_t *rep, uint32_t mode);
/* ... and with timing-tracked rows (announced by VDL2GPU_HAVE_TRACKED): trk[i] belongs to blocks[i] (vdl2gpu_poll_tracked), and a burst
 * of which attempt A passes no candidate gets the second attempt defined at vdl2gpu_trk_t.  Works on any handle; soft, fb and rep may
 * each be NULL; mode as above; trk == NULL: exactly vdl2gpu_decode_blocks_ex. */
int vdl2gpu_decode_blocks_tracked(vdl2gpu_t *h, const vdl2gpu_burst_t *blocks, const vdl2gpu_soft_t *soft, const vdl2gpu_fb_t *fb,
				  const vdl2gpu_trk_t *trk, int n, vdl2gpu_frame_t *frames, int max_frames, int *dropped, vdl2gpu_blockrep_t *rep,
				  uint32_t mode);
/* With VDL2GPU_F_FRAMES the same kernel runs on every push's burst records where they lie in device
 * memory, right behind the demodulator.  Collect the frames of everything pushed so far (waits like
 * vdl2gpu_poll; the bursts themselves stay available through vdl2gpu_poll).  Frames come out ordered
 * by (end_dec, stream, chn, seq); `block` is -1 here, and of data[] only [0, len) is written.  Returns the
 * count or a negative error. */
int vdl2gpu_poll_frames(vdl2gpu_t *h, vdl2gpu_frame_t *out, int max);
/* Same, but never waits (like vdl2gpu_poll_ready). */
int vdl2gpu_poll_frames_ready(vdl2gpu_t *h, vdl2gpu_frame_t *out, int max);

/* d8psk.c:39-52; the host path keeps calling it (out.c:429-432, outxid.c:122). */
unsigned int reversebits(const unsigned int bits, const int n);

/* ---- pure host helpers (usable without a GPU) ---- */
/* Length of a channel's local-oscillator table: sdrinrate / gcd(sdrinrate, 25000), the period of the oscillator for
 * an offset on the 25 kHz grid.  SDRINRATE/25000 (d8psk.c:348) where 25 kHz divides the rate; 2048 at 2.048 MS/s,
 * 6144 at 30.72 MS/s.  0 for a rate of 0. */
#define VDL2GPU_HAVE_OFFGRID_RATES 1
int vdl2gpu_lo_len(unsigned sdrinrate);
/* Local-oscillator table of one channel, d8psk.c:353-357 (libm sincosf of the
 * float-narrowed phase step) for n = 0 .. vdl2gpu_lo_len(sdrinrate) - 1.  Returns that length, or
 * VDL2GPU_EINVAL if max_complex is smaller. */
int vdl2gpu_lo_table(unsigned sdrinrate, int fo_hz, float *out_re_im, int max_complex);
/* Integrate-and-dump schedule of one push (d8psk.c:374-381 in closed form). */
int vdl2gpu_plan(uint64_t total_in, uint64_t n, unsigned sdrclk, unsigned lo_len,
		 int *c0, int *no0, int *nf0, int64_t *nout);
/* VDL2GPU_F_EXACT_FO: the rotation tables of a rate, interleaved re,im: T_hi into hi_re_im (max_hi complex values of room),
 * the 4096 entries of T_lo into lo_re_im; either may be NULL.  Returns the length of T_hi, ceil(2 * sdrinrate / 4096), or
 * VDL2GPU_EINVAL (a rate of 0 or above 2^30, max_hi too small). */
int vdl2gpu_exact_fo_tables(unsigned sdrinrate, float *hi_re_im, int max_hi, float *lo_re_im);
/* ... and the phase index k of the window whose first and last inputs are samples a and e of the stream, for a residual
 * offset of fd_hz: (fd * ((a + e) mod 2R)) mod 2R, fd = fd_hz mod 2R taken non-negative.  VDL2GPU_EINVAL for such a rate. */
int64_t vdl2gpu_exact_fo_index(uint64_t a, uint64_t e, unsigned sdrinrate, int fd_hz);
/* VDL2GPU_F_CARRIER: the derived values of a carrier record from its sums, the formulas at vdl2gpu_carrier_t in double precision
 * (what the library's collector calls for every record).  df, Fr: the burst record's.  Fills all of *out (reserved = 0).
 * VDL2GPU_EINVAL for nsym <= 0, Fr == 0 or out == NULL. */
int vdl2gpu_carrier_from_sums(float df, int Fr, int nsym, int sum_e, unsigned sum_e2, vdl2gpu_carrier_t *out);
/* VDL2GPU_F_SYMCLK: the derived values of a symbol-clock record from its sums, the formulas at vdl2gpu_symclk_t in double precision
 * (what the library's collector calls for every record).  e: the sums of the first ceil(nsym / 256) segments, 8 floats each (it may be
 * out->e itself).  Fills all of *out: the two integers as given, nseg, the derived fields, reserved = 0, e copied and zero from segment
 * nseg on.  tau_s: if not NULL, room for VDL2GPU_SYMCLK_SEGS doubles; the first nseg receive the segments' unwrapped tau_s.
 * VDL2GPU_EINVAL for nsym <= 0 or above 256 * VDL2GPU_SYMCLK_SEGS, sdrinrate == 0, e == NULL or out == NULL. */
int vdl2gpu_symclk_from_sums(int64_t sym_first_dec, int nsym, const float *e, unsigned sdrinrate, vdl2gpu_symclk_t *out, double *tau_s);
/* Frequency planning: the tuner centre the reference picks for a list of channel
 * frequencies, and the per-channel mixer offsets Fo it derives (thread_param_t.Fo).
 *   rtl: chooseFc() of rtl.c:123-160 -- the highest Fc (1 Hz steps, downwards from max + 50 kHz) that keeps every
 *        channel within SDRINRATE/2 - 50 kHz, none closer than 50 kHz, and no two adjacent (sorted) channels
 *        mirror images of each other; Fo = Fr - Fc (rtl.c:245-247).  Returns 0 and Fc = 0 when the channels span
 *        more than SDRINRATE - 100 kHz, like the reference.
 *   air: chooseFc() of air.c:47-70 -- the midpoint rounded to the 25 kHz grid, at 5 MS/s (Airspy R2) shifted by
 *        the R820T2 filter pair that just covers the span; Fo = Fr - (Fc + SDRINRATE/4) (air.c:182-184).  The two
 *        tuner register values the reference writes (R10 = 0xB0 | (15-j), R11 = 0xE0 | (15-i)) are returned as
 *        well (0 when none is written).
 * fr[] is NOT reordered (the reference sorts a scratch copy, rtl.c:218-241).  Parity: unpinned -- rtl.c / air.c
 * need the SDR vendor headers and cannot be compiled in the build container; tested against hand-derived
 * cases and an independent brute-force statement of the same rules. */
int vdl2gpu_choose_fc_rtl(const unsigned *fr, int nbch, unsigned sdrinrate, unsigned *fc, int *fo);
int vdl2gpu_choose_fc_air(const unsigned *fr, int nbch, unsigned sdrinrate, unsigned *fc, int *fo, int *r10, int *r11);

/* ---- diagnostics (P3 taps, tests only) ---- */
/* Decimated samples of the LAST push of (stream, channel index), interleaved
 * re,im; needs VDL2GPU_F_KEEP_DEC.  Returns the number of complex samples. */
int64_t vdl2gpu_debug_dec(vdl2gpu_t *h, int stream, int ch, float *out, int64_t max_complex);
/* Local-oscillator table of (stream, channel index): len complex values (with VDL2GPU_F_EXACT_FO: the table of Fg). */
int vdl2gpu_debug_lo(vdl2gpu_t *h, int stream, int ch, float *out, int max_complex);
/* Channeliser launches since vdl2gpu_create, by kernel (announced by VDL2GPU_HAVE_OFFGRID_RATES): out[0] k1_channelise with the
 * LO table in LDS, out[1] k1_channelise with the table in global memory (off-grid rates whose table does not fit LDS),
 * out[2] k1_pp, out[3] k1_fast.  Writes min(n, 4) counters and returns that number. */
int vdl2gpu_debug_k1(vdl2gpu_t *h, unsigned long long *out, int n);
/* Trigger candidates of the last push's sync scan, 6 x int32 each {nrel, r, p2err, perr, err, pfr bits}. */
int vdl2gpu_debug_cands(vdl2gpu_t *h, int stream, int ch, int *out, int max_cands);
/* ... and what follows each of them (one int2 per candidate: where the idle search resumes, relative to the push's planes; status |
 * sub-phase << 2 | descriptors << 4 | triggers << 8 | rejects << 16 | bursts << 24) */
int vdl2gpu_debug_clheads(vdl2gpu_t *h, int stream, int ch, int *out, int max_cands);
/* Verify pass of the last push: first unexpected detector hit per (stream, channel slot), and the
 * idle segments the resolver asked to have verified {lo, hi, r, pad}. */
int vdl2gpu_debug_fail(vdl2gpu_t *h, int *out, int n);
int vdl2gpu_debug_segs(vdl2gpu_t *h, int stream, int ch, int *out, int max_segs);
/* Development cycle counters of the demodulator kernels (meaning is internal). */
int vdl2gpu_debug_counters(vdl2gpu_t *h, unsigned long long *out, int n, int reset);
/* With VDL2GPU_F_DEBUG_HEADS: the descrambled header soft bits (what viterbi_add() is given, d8psk.c:81-83) of every
 * sync trigger ANY kernel of the last push handled -- the clusters of all timing classes, on the real chain or not,
 * and the serial stretches --, 34 x uint32 per entry: nstar (lo, hi), stream * 8 + channel slot, clk0, then the float
 * bits of p2err, perr, err, pfr and soft[25], one word of padding.  Unordered.  Returns the count (<= max_entries). */
int vdl2gpu_debug_heads(vdl2gpu_t *h, uint32_t *out, int max_entries);
/* Device build of the fixed-sequence atan2f, elementwise (host arrays). */
int vdl2gpu_debug_atan2f(vdl2gpu_t *h, const float *y, const float *x, float *out, size_t n);
/* rs() (rs.c:81-291) of n rows on the device: rows n x 255 in/out, eras n x 6 in/out, ret[i] = what rs() returns
 * (-1, or the number of roots with eras[6 i .. 6 i + ret[i]) their positions; 0 with eras untouched for zero syndromes).
 * VDL2GPU_EINVAL: no_eras[i] outside 0..6, or one of a row's first no_eras[i] positions outside 0..254. */
int vdl2gpu_debug_rs(vdl2gpu_t *h, uint8_t *rows, int *eras, const int *no_eras, int *ret, size_t n);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
