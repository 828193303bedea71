/* vdl2gpu_types.h -- types, parameters and constant tables of the device side.  Part of the device side of libvdl2gpu.so; included by vdl2gpu_kernels.h only. */
#ifndef VDL2GPU_TYPES_H
#define VDL2GPU_TYPES_H


#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vdl2_math.h"
#include "../../include/vdl2gpu.h"

#define VDL2_CS 8		/* channel planes per stream */
#ifndef VDL2_NSET
#define VDL2_NSET 3		/* plane sets, table sets and output rings, used in turn (push % VDL2_NSET): so many pushes in the pipeline, the oldest in its tail */
#endif
#define VDL2_NRING VDL2_NSET	/* output rings (records, frames, counters) */
#define VDL2_NSLAB (VDL2_NSET + 1)	/* page-locked slabs the records are exported to, used in turn */
static_assert(VDL2_NSET >= 3 && VDL2_NSET <= 4, "three bits of a record handle name its slab");
#define VDL2_HIST 160		/* frames of history kept: 17-tap FIR + 17 symbols x 8 + slack */
#define VDL2_NPH 68		/* NBPH*D8DWN, vdlm2.h:54-55 */
#define VDL2_STEADY 68		/* evaluations after which the detector forgot the last burst */
#define VDL2_MAXSYM 5456	/* >= ceil((25 + 8*8*255)/3) symbols of the longest burst */
#define VDL2_SERIAL_BELOW 4096	/* pushes of at most this many 84 kS/s frames go to the serial machine directly */
#define VDL2_CARRY_FRAMES 49152	/* >= longest burst (43592 frames) + history + slack */
#define VDL2_LONGEST_BURST 43592	/* trigger .. last symbol of the longest burst, frames: j0 + 8 (nsym - 1) <= 7 + 8 * 5448 (+ 1 of slack) */
/* VDL2GPU_F_LEVELS (vdl2gpu.h, vdl2gpu_level_t): the noise window reaches VDL2_LEV_GUARD + 8 * (VDL2_LEV_NEVAL - 1) + 16 frames in
 * front of a burst's first symbol.  A burst decoded in the push after its trigger (deferred) lies in the carried frames, and so must
 * its noise window: otherwise its levels would read stale planes and depend on where the stream was cut. */
#define VDL2_LEV_GUARD 512
#define VDL2_LEV_NEVAL 256
#define VDL2_LEV_BLOCK 32
static_assert(VDL2_LONGEST_BURST + VDL2_LEV_GUARD + 8 * VDL2_LEV_NEVAL + 16 <= VDL2_CARRY_FRAMES,
	      "the levels' noise window of a deferred burst must lie inside the carried planes");
static_assert(VDL2_LONGEST_BURST >= 7 + 8 * ((25 + 8 * VDL2GPU_MAXROWS * VDL2GPU_ROWLEN + 2) / 3 - 1), "VDL2_LONGEST_BURST covers the longest burst (burst_geom, burst_timing)");
#define VDL2_PN_BITS (16384 + 64)
#define VDL2_CAND_CAP 6144	/* trigger candidates per channel per push (round 5: 4096 -> 6144, what the resolver's 23 bytes of LDS per candidate allow) */
#define VDL2_CL_MAXB 4		/* bursts per cluster before the resolver takes over */
#define VDL2_SEL_CAP 16384	/* bursts on the real chain per channel per push */

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

/* ---- the words host and kernels share: counter blocks, modes and tags, development counters (the control words: CTL_* below) ---- */
struct RingCount {		/* records of one output ring's push */
	unsigned records, dropped;	/* written; not written because the ring was full */
};
struct OutCounters {		/* vdl2gpu.d_outc, device memory */
	RingCount ring[4];
	struct Totals {
		unsigned redo, repairs;	/* since the handle was made: serial redos (k2f_commit); channel-pushes that went through a repair round (k2_begin_repair) */
	} total;
	unsigned spare[6];
};
static_assert(sizeof(RingCount) == 2 * sizeof(unsigned) && sizeof(OutCounters) == 16 * sizeof(unsigned), "OutCounters is sixteen words");
static_assert(VDL2_NRING <= sizeof(OutCounters::ring) / sizeof(RingCount), "the rings' counters lie in front of the running totals");
struct FrameCounters {		/* vdl2gpu.d_fcnt[ring], device memory: the block path's output of one push (VDL2GPU_F_FRAMES) */
	unsigned frames, dropped;	/* written (compact: to the arena); not written (buffer or arena full) */
	unsigned arena_asked;	/* arena bytes asked for, failed allocations included */
	unsigned arena_end;	/* where the arena's last written entry ends: its valid bytes */
};
static_assert(sizeof(FrameCounters) == 4 * sizeof(unsigned), "FrameCounters is four words");
#define VDL2_FMASK_WORDS 16	/* the redo mask: a bit per (stream, channel slot) */
#define VDL2_FMASK_SLOTS (32 * VDL2_FMASK_WORDS)
struct PushCounters {		/* vdl2gpu.h_pin_cnt[ring], page-locked: what k3_rebase hands the host of a push */
	RingCount rec;
	OutCounters::Totals total;	/* the running totals as they stood behind this push */
	unsigned frames, frames_dropped, arena_end;	/* FrameCounters without arena_asked; zero without the block path */
	unsigned cand_ovf;	/* channels whose candidate tables overflowed in this push */
	unsigned fmask[VDL2_FMASK_WORDS];	/* K2f's redo mask of this push */
	unsigned cand_max;	/* most candidates of any channel */
	unsigned spare[7];
};
static_assert(sizeof(PushCounters) == 32 * sizeof(unsigned), "PushCounters is the 32 words a ring's block takes");
#define VDL2_WORD(T, m) ((int)(offsetof(T, m) / sizeof(unsigned)))	/* member m of a counter block, where the block is read as words (k3_rebase) */

/* K2Params.surv_mode / drain_mode: what a detector hit among a scan's survivors means (the legend above k2a_append) */
enum { SURV_CANDS = 0, SURV_VERIFY = 1, SURV_PROBE = 2, SURV_SEEDS_NEVER_SET = 3 /* no host code sets it; the kernels' tests for it stay (above k2a_append) */ };
/* K2Params.sel_mode: which selection a payload launch decodes (k2d_run) */
enum { SEL_FIRST = 0, SEL_REPAIRED = 1, SEL_FINAL = 2 };
/* device-side tag of a record, in vdl2gpu_burst_t.trig_sample until the host fills that field in (collect_records) */
enum { REC_FIRST = 0, REC_FINAL = 1, REC_VOID = 2 };

struct StreamState {
	long long dec_base;	/* stream time (84 kS/s index) of frame 0 of the current planes */
	long long dec_fill;	/* frames present before this push's K1 output */
	long long last_fill;	/* diagnostics: where the last push's output starts */
	long long last_J;
	float2 acc[2][VDL2_CS];	/* integrate-and-dump partial sums carried across pushes */
};

struct ChanState {
	long long pos;		/* stream time of the next WSYNC evaluation */
	int r;			/* FIR sub-phase (channel_t.clk after the -=8), 0..3 */
	int fresh;		/* evaluations since the last trigger/reset, saturating */
	float perr, p2err, pfr;	/* channel_t.perr/p2err/pfr */
	float ring[VDL2_NPH];	/* channel_t.Ph in time order, ring[67] newest */
	unsigned long long n_eval, n_trig, n_reject, n_burst, n_defer, n_slow, n_cand, n_redo;
};

struct ChanCfg {
	int chn, Fr, Fo, pad;
};

struct Cand {			/* free-running detector fires at dec_base + nrel with sub-phase r */
	int nrel, r;
	float p2err, perr, err, pfr;
};

enum { CL_STEADY = 0, CL_DEFER_FIRST = 1, CL_NONSTEADY = 2, CL_INVALID = 3 };
struct Cluster {		/* what the resolver reads of a cluster is its 8-byte head (cl_pack); this is the rest */
	ChanState saved;	/* CL_NONSTEADY: explicit state to continue from */
};

/* resolver's view of a cluster: x = n_s - dec_base, y = status | r_s << 2 | nslots << 4 | ntrig << 8 | nrej << 16 | nburst << 24 */
__device__ __forceinline__ int2 cl_pack(int n_s_rel, int status, int r_s, int nslots, int ntrig, int nrej, int nburst)
{
	ntrig = ntrig > 255 ? 255 : ntrig;
	nrej = nrej > 255 ? 255 : nrej;
	nburst = nburst > 255 ? 255 : nburst;
	return make_int2(n_s_rel, status | (r_s << 2) | (nslots << 4) | (ntrig << 8) | (nrej << 16) | (nburst << 24));
}
__device__ __forceinline__ int cl_status(int2 hd) { return hd.y & 3; }	/* ... and the fields of its y again (x is read as it is: hd.x) */
__device__ __forceinline__ int cl_r(int2 hd) { return (hd.y >> 2) & 3; }	/* sub-phase the idle search resumes in */
__device__ __forceinline__ int cl_nslots(int2 hd) { return (hd.y >> 4) & 15; }
__device__ __forceinline__ int cl_ntrig(int2 hd) { return (hd.y >> 8) & 255; }
__device__ __forceinline__ int cl_nrej(int2 hd) { return (hd.y >> 16) & 255; }
__device__ __forceinline__ int cl_nburst(int2 hd) { return (hd.y >> 24) & 255; }
/* status | r_s << 2 in one byte: what the resolver keeps of every head in LDS (K2cShared.sstat) */
__device__ __forceinline__ uint8_t cl_stat4(int2 hd) { return (uint8_t)(hd.y & 15); }
__device__ __forceinline__ int stat4_status(unsigned s4) { return (int)(s4 & 3u); }
__device__ __forceinline__ int stat4_r(unsigned s4) { return (int)((s4 >> 2) & 3u); }

struct BurstDesc {		/* a burst found by a cluster; payload decoded later if it is on the real chain */
	long long nstar;	/* stream time of the sync trigger */
	int sc;			/* stream*8 + channel */
	int clk0;		/* (int)roundf(of), d8psk.c:305 */
	float df;
	int nbrow, nlbyte, pad;
};

struct Seg {			/* the chain idled in class (r, parity of lo) over stream-relative [lo, hi) */
	int lo, hi, r, pad;
};

struct HeadTap {		/* diagnostics (VDL2GPU_F_DEBUG_HEADS): what one sync trigger gave the header decoder */
	long long nstar;	/* stream time of the trigger */
	int sc;			/* stream * 8 + channel slot */
	int clk0;		/* (int)roundf(of), d8psk.c:305 */
	float p2err, perr, err, pfr;	/* the detector's view at the trigger (d8psk.c:292-305) */
	float soft[25];		/* descrambled header soft bits as viterbi_add() gets them (d8psk.c:81-83) */
};
static_assert(sizeof(HeadTap) == 132 || sizeof(HeadTap) == 136, "HeadTap layout");

struct K1Params {
	const void *raw;
	size_t stream_stride;
	int nbch;
	int sdrclk, L, maxwin;
	int c0, no0, nf0, parity;
	int quirk;		/* cu8 only: the store-index off-by-one of rtl.c:291, per 32768-sample block */
	long long N, J;
	long long jbeg, jend;	/* generic kernel: outputs [jbeg, jend] (jend may be J = the carried tail) */
	long long per_lo, per_n;	/* k1_fast: superperiods [per_lo, per_lo+per_n) */
	int edge_state;		/* k1_fast covers the whole push (it starts and ends on a window boundary of the schedule: no carried
				 * partial window): the launch also leaves the stream state the general kernel would (last_fill, last_J, empty carry) */
	unsigned *tickets;	/* k1_fast: [S][21 roles][8 XCDs] work counters; never reset: */
	unsigned tbase[8];	/* ... what the counters of XCD x hold when this launch starts (every launch adds the number of its tickets) */
	const float2 *lo;	/* [S][8][L] */
	const float2 *lo_ext;	/* k1_fast: [S][8][lo_stride], entry 8 + i = lo[i mod L] for -8 <= i < L + 40 */
	int lo_stride;
	float2 *dec;		/* this push's planes, [S][8][cap] */
	long long cap;
	StreamState *ss;
};

struct K1PParams {		/* k1_pp: whole periods (PER = 4*SDRCLK inputs = 84 outputs) [per_lo, per_lo + per_n) of a push */
	const void *raw;
	size_t stream_stride;
	int nbch;
	int per_in;		/* inputs per period */
	int L;			/* LO table length */
	int ph0;		/* LO index of a period's first sample */
	int d;			/* samples between the 16-byte boundary below a period's first sample and that sample */
	int fast_div;		/* both window lengths are in the set the reciprocal division is proven exact for */
	int unused0;		/* (0; held development switches.  It keeps its place: with the members behind it four or eight bytes lower the
				 * compiler groups the k1_pp kernels' kernarg loads differently and allots them other registers) */
	int nf_lo;		/* the shorter of the two window lengths; rcp_lo = RN(1/nf_lo), rcp_hi = RN(1/(nf_lo+1)) */
	float rcp_lo, rcp_hi;
	int per_n;
	int nsub, wpt;		/* a period's 84 windows are split into nsub tasks of wpt */
	long long per_lo;
	long long sbase0;	/* push-relative index of the first sample of period per_lo */
	const float2 *lo_ext;	/* [S][8][lo_stride]: the LO table followed by its first 16 entries again */
	int lo_stride;
	float2 *dec;
	long long cap;
	StreamState *ss;
	int edge_state;		/* the launch covers the whole push (it starts and ends on a window boundary of the schedule): it also leaves the
				 * stream state the general kernel would (last_fill, last_J, an empty carry in acc[parity ^ 1]) */
	int parity;
	long long J;
	int wend[84];		/* last sample of each window, relative to the period's first sample */
};

/* VDL2GPU_F_EXACT_FO (include/vdl2gpu.h): what the rotating instantiations of the K1 kernels take beside their parameters.  The
 * phase index of output m is k_m = fd * (a_m + e_m) mod M, M = 2 * SDRINRATE.  The dump schedule repeats every SDRCLK inputs
 * for 21 outputs, so with m = 21 q + i:  k_m = (fd * (2 SDRCLK q mod M) + tab[i]) mod M, and a step of q adds tab[21]. */
#define K1R_TAB 24
struct K1Rot {
	const unsigned *tab;	/* [S][8][K1R_TAB] per channel: [i < 21] fd * (a_i + e_i) mod M for the schedule's first period,
				 * [21] fd * 2 SDRCLK mod M, [22] fd = Fd mod M, [23] Fd != 0 (a channel on the grid is left alone) */
	const float2 *hi;	/* T_hi[ceil(M / 4096)] */
	const float2 *lo;	/* T_lo[4096] */
	double rM;		/* 1 / M (k1r_mod) */
	unsigned M;
	unsigned sq0;		/* 2 SDRCLK q0 mod M, q0 = the schedule period the push's output 0 lies in */
	int i0;			/* that output's place in its period: (outputs before the push) mod 21 */
};

struct K2Slog {			/* a stretch the first resolver pass handled with the serial machine: where it began (stream-relative) and what it counted */
	int t, ntrig, nrej, nburst;
};
struct K2aItem;
struct K2Params {
	const float2 *dec;
	long long cap;
	int nbch, nstreams;
	long long J;
	long long dec_base;	/* stream time of frame 0 of the planes (host arithmetic: outputs before this push - VDL2_CARRY_FRAMES) */
	long long scan_lo;	/* first instant the scans look at: dec_base + VDL2_HIST (NOT the channel's position: the front stage of a
				 * push runs before the previous push has committed where its channels stand) */
	int probe_r, probe_par;	/* the class the probe scans everywhere (fixed), parity of its instants */
	StreamState *ss;
	ChanState *cs;
	const ChanCfg *cfg;
	const uint8_t *pn;
	const uint8_t *pn8;	/* the scrambler sequence by payload byte: bit i of pn8[b] = pn[25 + 8 b + i] */
	Cand *cands;		/* [S*8][CAND_CAP] */
	Cluster *clusters;	/* [S*8][CAND_CAP] */
	int2 *clhead;		/* [S*8][CAND_CAP] what the resolver needs of every cluster, 8 bytes: see cl_pack() */
	unsigned *ctl;		/* the push's control words: CTL_* below */
	BurstDesc *stage;	/* burst descriptors of all clusters */
	unsigned *sel_list;	/* descriptors on the real chain (K2c -> K2d) */
	unsigned *sel_list2;	/* ... as the repair rounds re-resolved them (channels in fmask) */
	int sel_mode;		/* K2d: SEL_FIRST = the first selection of every channel (beside the verify pass: the mask is not final yet);
				 * SEL_REPAIRED = the repaired selection of the masked channels (second pass);
				 * SEL_FINAL = one pass behind the commit: the repaired selection for masked channels, the first for the others */
	unsigned stage_cap;
	vdl2gpu_burst_t *recs;	/* output ring of this push */
	vdl2gpu_level_t *levels;	/* VDL2GPU_F_LEVELS: one level record per record slot of `recs`, else nullptr (nothing is measured) */
	vdl2gpu_soft_t *soft;	/* VDL2GPU_F_SOFT_RS: one reliability map per record slot of `recs`, else nullptr */
	RingCount *outc;	/* this push's ring */
	OutCounters::Totals *outc_total;	/* running counts of serial redos and repairs (the host adapts the number of repair rounds by them) */
	unsigned *fmask;	/* [VDL2_FMASK_WORDS] bit per (stream, channel slot) that a repair round re-resolved or K2f redid serially in this push */
	int full_round;		/* this repair round scans the failing channels completely (all classes, every instant): no regions, no verify */
	int mini_round;		/* this repair round re-resolves with what the verify pass found and appended to the tables, nothing else: no scan, no
				 * clusters (the resolver replays the few new candidates itself) */
	int sel_reserved;	/* K2c reserves the output records of a channel's selected bursts in one piece (CTL_SELBASE0), K2d fills them without atomics */
	unsigned rec_cap;
	int force_serial;	/* diagnostics: skip the tables, run the serial machine */
	int prim_drop;		/* test handicap: every prim_drop-th candidate gets no precomputed cluster (the resolver builds it) */
	int full_scan;		/* scan all four sub-phases everywhere (no regions / verify) */
	int test_noregion;	/* test hook: skip the region scan so that K2a-verify must catch the misses */
	int2 *regs;		/* [S*8][REG_CAP] (lo, count) stream-relative */
	Seg *segs;		/* [S*8][SEG_CAP] */
	int *fail;		/* [S*8] earliest unexpected hit (stream-relative), >= VDL2_VERIFIED = verified */
	int *redo;		/* [S*8] 1 = this channel is being re-resolved in the repair round */
	int round;		/* 0 = first pass over every channel; 1 = repair pass over the channels whose
				 * verify failed (the hits were appended to their candidate tables) */
	ChanState *cs_out;	/* resolver result, committed by K2f */
	int *skey;		/* [S*8][CAND_CAP] candidates sorted by time: nrel*4 + r */
	unsigned short *sidx;	/* [S*8][CAND_CAP] sorted rank -> candidate index */
	unsigned short *prim;	/* [S*8][CAND_CAP] candidates whose cluster K2b computes */
	uint8_t *onchain;	/* [S*8][CAND_CAP] by candidate: 1 = the first resolver pass's chain met this candidate in the history-free state (k2p_patch: a
				 * repaired stretch of the chain that arrives at such a candidate has rejoined the old chain) */
	K2Slog *slog;		/* [S*8][VDL2_SLOG_CAP] the first pass's serial stretches (their counts are not in any cluster head) */
	int2 *win;		/* [S*8][VDL2_WIN_CAP] windows of stream-relative time [x, y): bursts of the first selection triggered inside are void (CTL_NWIN0) */
	int *seeds;		/* [S*8][CAND_CAP] probe instants around which all classes are scanned */
	struct K2aItem *items;	/* [S*8][ITEM_CAP] what passed a scan's first screen: a private area per scan workgroup (worked off by that workgroup behind
				 * its last tile), a common area behind them (worked off by the next kernel on the stream) */
	unsigned item_cap;	/* items per channel of the list (private areas + common area): sized by the longest part the handle can be given */
	unsigned item_priv;	/* ... of which private areas at most (host side: launch_scan) */
	int surv_pch, surv_nwg;	/* items a private area holds (a multiple of 256), scan workgroups per channel (= private areas) */
	int surv_common_cap;	/* test hook: the common area holds only so many items (0: all that is left of the list) */
	int surv_slot;		/* which of the push's scans this is: its item counters are ctl[CTL_NSURV0 + slot * S*8 ...] (VDL2_SURV_*) */
	int surv_mode;		/* sparse stages: what a detector hit among the survivors means (k2a_emit: SURV_*) */
	int surv_skip;		/* sparse stages: hits in the probe's class are in the table already (region scan) */
	/* the one-workgroup-per-channel kernel behind a scan drains that scan's common area first (k2x_drain): which scan, and how its list was laid out */
	int drain_slot;		/* VDL2_SURV_* of the scan in front of this launch, -1: nothing to drain */
	int drain_mode, drain_skip;	/* that scan's surv_mode, surv_skip */
	int drain_pch, drain_nwg;	/* ... surv_pch, surv_nwg */
	unsigned long long *dbg;	/* diagnostics: cycle counters */
	HeadTap *headtap;	/* diagnostics: every trigger any kernel of the push handled (nullptr: off) */
	unsigned *headtap_n;
	unsigned headtap_cap;
	vdl2gpu_carrier_t *carrier;	/* VDL2GPU_F_CARRIER: one record of phase-error sums per record slot of `recs`, else nullptr (last: the other members keep their place) */
#ifdef VDL2GPU_TESTHOOKS
	/* test hooks (VDL2GPU_TEST_*_CAP): what the back stage's lists hold, at most their compile-time sizes (the host fills in the size where
	 * the hook is unset).  Only the comparisons read these (K2_*_LIM below); strides, LDS arrays and allocations keep the constants.
	 * (lim_reg also decides WHICH regions a lowered limit keeps: the same ones in every run, evenly spread over the push -- k2r_regions) */
	int lim_reg, lim_seg, lim_vis, lim_win, lim_merge, lim_slog;
#endif
};
/* Development counters (K2Params.dbg, vdl2gpu_debug_counters: 96 words in a test build, 64 in the product; VDL2GPU_DEBUG_COUNTERS).  Every
 * slot that anything outside the kernel that writes it reads has its name here; vdlm2dec_amd/lib.py (DBG) carries the same table for the
 * tests and scripts, and tests/test_shared_words.py holds the two together.
 * [0 .. 15] k2b_clusters, of every sixteenth cluster: 100 MHz ticks in the ring fill and in the rest, clusters sampled, their triggers,
 *   evaluations, the longest rest, steady ends, rejects; ticks and clusters by the cluster's ordinal in its wavefront (+ 0 .. 3)
 * [16 .. 20], [25 .. 29] k2c_resolve per call: ticks in its four phases, calls; replays of clusters K2b did not make, non-steady clusters
 *   continued serially, candidates, visited-list entries, samples through the serial machine
 * [24] channel-pushes that went through a repair round (k2_begin_repair)   [30] evaluation instants of every piece the verify passes scanned
 * [32 .. 47], [48 .. 63] the probe's and the region scan's stage counters (K2A_ST_* below), of every eighth workgroup's first lane
 * -- from here on in a test build only --
 * [64 .. 70] escapes: how often a kernel took the branch for a full list --
 *   64 regions (k2r_regions)  65 verify stretches (k2_emit_seg, k2p_patch, k2a_verify's clamp)  66 visited list (k2c_walk, k2c_resolve)
 *   67 windows (k2p_patch)  68 merge (k2p_patch, k2s_merge: also in 75)  69 serial-stretch log (k2c_publish, k2p_patch)
 *   70 descriptor pool or selection list full under a kernel that stages descriptors (k2b_clusters, k2c_resolve, k2p_patch: MachOut.badslot)
 * [71 .. 74] violations of the two invariants at CTL_NWIN0 (every test reads zero) --
 *   71 (b) k2b_clusters: a cluster's first descriptor whose nstar is not dec_base + its candidate's nrel
 *   72 (b) k2d_run: the same, of every first descriptor of a cluster it decodes
 *   73 (b) k2d_run, SEL_REPAIRED: a record whose trig_dec is not the nstar of the descriptor it was made from
 *   74 (a) k2p_patch: a burst of the first selection triggered inside a window whose cluster's candidate is not marked in onchain[]
 * [75] of the merge escapes, those of k2s_merge (a further round: the resolver takes the channel through the serial machine)
 * [76] k2p_patch gave a repair up that it had begun (k2_begin_repair had run: more windows or stretches than the lists hold, or the pool full)
 * [77 .. 80] how often the checks behind 71 .. 74 were made (a zero there says something only if these are not) */
enum K2Dbg {
	K2_DBG_K2B_RING_TICKS = 0, K2_DBG_K2B_REST_TICKS, K2_DBG_K2B_SAMPLED, K2_DBG_K2B_TRIG, K2_DBG_K2B_EVAL, K2_DBG_K2B_MAX_TICKS,
	K2_DBG_K2B_STEADY, K2_DBG_K2B_REJ, K2_DBG_K2B_ORD_TICKS0 = 8, K2_DBG_K2B_ORD_COUNT0 = 12,
	K2_DBG_K2C_LOAD_TICKS = 16, K2_DBG_K2C_TABLES_TICKS, K2_DBG_K2C_WALK_TICKS, K2_DBG_K2C_PUBLISH_TICKS, K2_DBG_K2C_CALLS,
	K2_DBG_REPAIRED = 24, K2_DBG_K2C_REPLAYS, K2_DBG_K2C_NONSTEADY, K2_DBG_K2C_CANDS, K2_DBG_K2C_VISITED, K2_DBG_K2C_SERIAL_SAMPLES,
	K2_DBG_VERIFY_INSTANTS = 30, K2_DBG_PROBE_STAGE0 = 32, K2_DBG_REGION_STAGE0 = 48,
	K2_DBG_ESC_REG = 64, K2_DBG_ESC_SEG, K2_DBG_ESC_VIS, K2_DBG_ESC_WIN, K2_DBG_ESC_MERGE, K2_DBG_ESC_SLOG, K2_DBG_ESC_STAGE,
	K2_DBG_INV_B_CLUSTER, K2_DBG_INV_B_DECODE, K2_DBG_INV_B_RECORD, K2_DBG_INV_A, K2_DBG_ESC_MERGE_SORT,
	K2_DBG_ESC_PATCH_ABANDON, K2_DBG_CHK_B_CLUSTER, K2_DBG_CHK_B_DECODE, K2_DBG_CHK_B_RECORD, K2_DBG_CHK_A
};
/* the sixteen stage slots behind K2_DBG_PROBE_STAGE0 / K2_DBG_REGION_STAGE0 (K2aShared.prof; ticks unless said otherwise).  The probe stamps
 * the tile's stages; the region scan counts its tile loop as a whole (TILES_OR_WAIT) and its instants.  UNUSED*: stages that have gone */
enum K2aStage {
	K2A_ST_STAGE_IN = 0, K2A_ST_FIR_UNIT, K2A_ST_BARRIER_SAMPLES, K2A_ST_STEPS, K2A_ST_SCREEN, K2A_ST_UNUSED5, K2A_ST_UNUSED6, K2A_ST_UNUSED7,
	K2A_ST_SCREEN_END, K2A_ST_BARRIER_TILE, K2A_ST_UNUSED10, K2A_ST_PASSES /* a count */, K2A_ST_TILES_OR_WAIT, K2A_ST_PARK, K2A_ST_UNUSED14,
	K2A_ST_INSTANTS /* a count */, K2A_ST_SLOTS
};
static_assert(K2A_ST_SLOTS == 16 && K2_DBG_REGION_STAGE0 == K2_DBG_PROBE_STAGE0 + K2A_ST_SLOTS && K2_DBG_ESC_REG == K2_DBG_REGION_STAGE0 + K2A_ST_SLOTS,
	      "the two scans' stage slots lie between the resolver's counters and the test build's");
/* What a list of the back stage holds: the compile-time size, in a test build the run-time value beside it (K2Params.lim_*).  Every
 * comparison against a size goes through its macro, so that a lowered limit is one limit everywhere. */
#ifdef VDL2GPU_TESTHOOKS
#define K2_REG_LIM(p) ((p).lim_reg)
#define K2_SEG_LIM(p) ((p).lim_seg)
#define K2_VIS_LIM(p) ((p).lim_vis)
#define K2_WIN_LIM(p) ((p).lim_win)
#define K2_MERGE_LIM(p) ((p).lim_merge)
#define K2_SLOG_LIM(p) ((p).lim_slog)
#define VDL2_DBG_WORDS 96
#define K2_COUNT(p, slot) do { if ((p).dbg) atomicAdd((p).dbg + (slot), 1ull); } while (0)
#else
#define K2_REG_LIM(p) VDL2_REG_CAP
#define K2_SEG_LIM(p) VDL2_SEG_CAP
#define K2_VIS_LIM(p) K2C_VIS
#define K2_WIN_LIM(p) VDL2_WIN_CAP
#define K2_MERGE_LIM(p) K2S_MERGE
#define K2_SLOG_LIM(p) VDL2_SLOG_CAP
#define VDL2_DBG_WORDS 64
#define K2_COUNT(p, slot) do { } while (0)
#endif
#define CTL_OUT 0
#define CTL_OUT_OVF 1
#define CTL_STAGE 2
#define CTL_TICKET 3
#define CTL_STAGE_OVF 4
/* ... and behind them blocks of a word per channel slot, [S*8] each: CTL_x0(p) is the first word of block x, p a parameter block with
 * `nstreams` (K2Params, K3Params: the host uses the same macros) */
#define CTL_CAND0 8		/* candidate counts */
/* the scans of a push, each with item counters of its own (K2Params.surv_slot) */
enum { VDL2_SURV_PROBE = 0, VDL2_SURV_REGION = 1, VDL2_SURV_VERIFY = 2 /* + repair round (1..4) */, VDL2_SURV_FULL = 7, VDL2_SURV_SLOTS = 8 };
enum { CTL_B_CAND = 0, CTL_B_CANDOVF, CTL_B_NREG, CTL_B_NSEG, CTL_B_NSEL, CTL_B_NPRIM, CTL_B_NSEED, CTL_B_NCLUST,
       CTL_B_NSURV, CTL_B_SELBASE = CTL_B_NSURV + VDL2_SURV_SLOTS, CTL_B_NSEL1, CTL_B_SELBASE1,
       CTL_B_NSURVLIM, CTL_B_NWIN = CTL_B_NSURVLIM + VDL2_SURV_SLOTS, CTL_B_NSLOG, CTL_B_END };
#define CTL_BLOCK(p, b) (CTL_CAND0 + (b) * (p).nstreams * VDL2_CS)
#define CTL_CANDOVF0(p) CTL_BLOCK(p, CTL_B_CANDOVF)	/* bit 0: the candidate table overflowed, bit 1: unusable for another reason than its size */
#define CTL_NREG0(p) CTL_BLOCK(p, CTL_B_NREG)
#define CTL_NSEG0(p) CTL_BLOCK(p, CTL_B_NSEG)
#define CTL_NSEL0(p) CTL_BLOCK(p, CTL_B_NSEL)
#define CTL_NPRIM0(p) CTL_BLOCK(p, CTL_B_NPRIM)
#define CTL_NSEED0(p) CTL_BLOCK(p, CTL_B_NSEED)
#define CTL_NCLUST0(p) CTL_BLOCK(p, CTL_B_NCLUST)	/* candidates [0, n) had their clusters decided by the previous K2s/K2b of this push */
#define CTL_NSURV0(p) CTL_BLOCK(p, CTL_B_NSURV)	/* [VDL2_SURV_SLOTS][S*8] item counts, one set per scan of the push */
#define CTL_SELBASE0(p) CTL_BLOCK(p, CTL_B_SELBASE)	/* first output record of the channel's selected bursts (K2c reserves, K2d fills) */
/* The selection exists twice: the first resolver pass writes sel_list / CTL_NSEL0 / CTL_SELBASE0, the repair rounds sel_list2 and
 * the words below -- the payload decode of the first selection runs beside the verify pass AND beside the repair round (on a
 * stream of its own), which therefore must not touch what it reads. */
#define CTL_NSEL1(p) CTL_BLOCK(p, CTL_B_NSEL1)
#define CTL_SELBASE1(p) CTL_BLOCK(p, CTL_B_SELBASE1)
#define CTL_NSURVLIM0(p) CTL_BLOCK(p, CTL_B_NSURVLIM)	/* [VDL2_SURV_SLOTS][S*8] ~(where the first group that the common area
											 * refused would have begun): 0 = none refused; items below it are complete */
#define CTL_NWIN0(p) CTL_BLOCK(p, CTL_B_NWIN)	/* [S*8] what the repair rounds made void of the channel's FIRST selection: 0 nothing,
											 * 1..VDL2_WIN_CAP: the bursts triggered inside so many windows of stream time (K2Params.win:
											 * a local repair, k2p_patch), VDL2_WIN_ALL: all of it (the channel was resolved again from its
											 * input state, or redone serially) */
#define CTL_NSLOG0(p) CTL_BLOCK(p, CTL_B_NSLOG)	/* [S*8] entries of K2Params.slog the first resolver pass made (VDL2_SLOG_CAP + 1: more than it holds) */
/* Two invariants the windows of CTL_NWIN0 stand on (both implicit in the code, held by the parity and soak tests alone):
 * (a) K2Params.onchain[] marks the candidates the first resolver pass met history-free: exactly the clusters whose bursts that pass
 *     selected and whose head it counted, and the candidates a walk stopped at without counting their head (CL_DEFER_FIRST, CL_INVALID:
 *     such a head counts nothing, or K2Params.slog has it).  ESTABLISHED by k2c_resolve's first pass (k2c_publish, and the kernel's loop
 *     for the candidate a walk stops at); RELIED ON by k2p_patch: a repaired stretch that arrives at such a candidate has rejoined the
 *     old chain, and k2p_old_counts takes the old chain's counts inside a window from these heads;
 * (b) a burst's trigger instant is the same number everywhere: BurstDesc.nstar of a cluster's first burst = dec_base + its candidate's
 *     nrel, and a record's trig_dec = its descriptor's nstar.  ESTABLISHED by k2b_clusters (st.pos = dec_base + nrel) and burst_payload;
 *     RELIED ON by k2_in_windows' callers in k2d_run, which test trig_dec (SEL_REPAIRED) and nstar (SEL_FINAL) against windows that
 *     k2p_patch made of candidate times. */
#define VDL2_CTL_WORDS(nsc) (CTL_CAND0 + CTL_B_END * (size_t)(nsc))	/* (nsc: channel slots, S*8) */
#define VDL2_WIN_CAP 32
#define VDL2_WIN_ALL 0xffffffffu
#define VDL2_SLOG_CAP 16

struct K3Params {
	const float2 *src;
	float2 *dst;
	long long cap;
	int nbch;
	long long J;
	StreamState *ss;
	const ChanState *cs;
	const OutCounters *outc;	/* device counters: every ring's and the running totals */
	const unsigned *fmask;	/* K2f's redo mask of this push (VDL2_FMASK_WORDS) */
	const FrameCounters *fcnt;	/* block path in the pipeline (VDL2GPU_F_FRAMES): this ring's; else nullptr */
	PushCounters *host_cnt;	/* what the host reads of them, in pinned host memory, for this push's ring */
	int ring;
	const unsigned *ctl;	/* the push's control words */
	int nstreams;
};

struct KInitParams {		/* per-push reset of the demodulator's control words */
	unsigned *ctl;
	int ctl_words;
	RingCount *outc;	/* this push's ring */
	int *fail, *redo;
	int nsc;
	unsigned *fmask;	/* VDL2_FMASK_WORDS */
	FrameCounters *fcnt;	/* this ring's block-path counters, or nullptr */
};

/* ---- constant data tables (d8psk.h:20-249) as bit patterns ------------- */
/* (defined once in the library: a second translation unit, vdl2gpu_allframes.hip, takes the types alone) */
#ifndef VDL2GPU_TYPES_NO_TABLES
#define VDL2_TABLE_BEGIN(name, n) __constant__ uint32_t c_##name[n] = {
#define VDL2_F32(x) x,
#define VDL2_TABLE_END };
#include "vdl2_tables.inc"
#undef VDL2_TABLE_BEGIN
#undef VDL2_F32
#undef VDL2_TABLE_END

/* parity-check columns of the (25,20) header code (data, viterbi.c:29-35) */
__constant__ int c_hcol[25] = { 6, 7, 9, 10, 11, 12, 14, 15, 17, 19, 21, 22, 24, 25, 26, 27, 28, 29, 30, 31,
	16, 8, 4, 2, 1
};
#endif	/* VDL2GPU_TYPES_NO_TABLES */

#endif
