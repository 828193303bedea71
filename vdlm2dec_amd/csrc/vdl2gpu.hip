/*
 * vdl2gpu.hip -- host side of libvdl2gpu.so: the C ABI of include/vdl2gpu.h.
 *
 * One handle = one MI355X, three pushes in the pipeline.  vdl2gpu_push() enqueues
 *   front stage (fstream):     [H2D copy] -> K1 channelise -> K2a probe + K2x second stage / regions / region scan + K2x -> K2s sort -> carry for the next push
 *   back stage  (stream):      K2b clusters -> K2c resolve -> K2a verify + K2x (K2d payload beside it, on the copy stream)
 *   tail        (pay_stream):  repair round (merge, resolve, verify) -> commit -> re-resolved payloads -> export -> counters
 * and returns; the front stage of one push runs beside the back stage of the one before and the tail of the one before that
 * (see vdl2gpu::Back and enqueue_back); plane sets, table sets and output rings exist three times, the slabs four times.
 * vdl2gpu_poll() synchronises and hands burst records back in stream-time order.  There is no CPU fallback: without a HIP device
 * vdl2gpu_create() fails with VDL2GPU_ENODEV.
 *
 * Build (see __graft_entry__.build()):
 *   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared \
 *         vdl2gpu.hip -o libvdl2gpu.so
 */
#include "vdl2gpu_kernels.h"
#include "vdl2gpu_blocks.h"
#include "vdl2gpu_symclk.h"
#include "vdl2gpu_tracked.h"

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

extern "C" void sincosf(float, float *, float *);

#define HIPCHK(h, expr)                                                                         \
	do {                                                                                    \
		hipError_t e__ = (expr);                                                        \
		if (e__ != hipSuccess) {                                                        \
			(h)->err = std::string(#expr) + ": " + hipGetErrorString(e__);          \
			return VDL2GPU_EHIP;                                                    \
		}                                                                               \
	} while (0)

#define TRY(expr)                        \
	do {                             \
		const int rc__ = (expr); \
		if (rc__)                \
			return rc__;     \
	} while (0)

/* The HIP events of a push that carries stage events (vdl2gpu_timing_t, VDL2GPU_STAGE_DUMP), recorded by mark().  The numbers are
 * the eN= labels of the stage dump (scripts/dev/stage_gantt.py reads them): they stay.  17 and 19 are no longer recorded. */
enum StageEv {
	E_K1_BEGIN = 0, E_K1_END = 1,			/* in front of the channeliser, behind it */
	E_CLUSTERS_BEGIN = 2, E_CLUSTERS_END = 3,
	E_FRONT_END = 4,				/* the front stage's scan + sort end */
	E_ROUNDS_END = 5,				/* repair rounds end */
	E_BLOCKS_END = 6,				/* second payload pass + block path end */
	E_TAIL_END = 7,
	E_K1_KERNEL_BEGIN = 8, E_K1_KERNEL_END = 9,	/* around the k1_fast / k1_pp launch alone */
	E_SCAN_BEGIN = 10,
	E_K1_HEAD_END = 11,				/* the first period's general launch ends */
	E_VERIFY_BEGIN = 12,
	E_RESOLVE_QUEUED = 13, E_RESOLVE_END = 14,	/* around the resolver, its wait for the previous push's commit included */
	/* VDL2GPU_STAGE_DUMP only: */
	E_VERIFY_END = 15,
	E_TAIL_BEGIN = 16,				/* the verify pass has been seen on the tail's stream */
	E_PATCH_END = 18,				/* local repair ends */
	E_COMMIT_END = 20, E_PAYLOAD2_END = 21, E_EXPORT_END = 22,	/* commit, second payload pass, export end */
	E_RESOLVE_BEGIN = 23,				/* the previous push's commit has been seen */
};
#define NEVX 24
struct PushTiming {
	hipEvent_t e[NEVX];	/* by StageEv */
	uint64_t samples;
	uint64_t index;		/* which push of the handle (VDL2GPU_STAGE_DUMP) */
	bool fast;
	bool staged;
	int fast_parts;		/* fast-kernel launches of this push (E_K1_KERNEL_BEGIN..E_K1_KERNEL_END) */
};

/* An event that may not have been recorded yet (the first pushes of a handle; a path not taken yet): waiting for it then waits
 * for nothing.  The rule: an event that something may wait for before any record is a LaterEvent; an event whose record is certain
 * wherever it is waited for -- earlier in the same call (f_done, k2c_done, pay_done, verify_done, raw_copied), or by the condition
 * of the wait itself (f_tail: last_two_streams) -- is a plain hipEvent_t. */
struct LaterEvent {
	hipEvent_t ev = nullptr;
	bool recorded = false;
	int record(vdl2gpu_t *h, hipStream_t s);
	int wait(vdl2gpu_t *h, hipStream_t s) const;	/* the stream waits */
	int sync(vdl2gpu_t *h) const;			/* the calling thread waits */
	void clear() { recorded = false; }
};

/* A burst record has side columns: entries at the record's index in the device rings, the slabs and the host queue, present when
 * the handle's flags ask for them.  A column is a name in the enum and a row of each of the two tables here. */
enum { COL_LEVEL, COL_SOFT, COL_CARRIER, COL_REPORT, COL_FB, COL_SYMCLK, COL_TRK, VDL2_NCOL };	/* (the order of the collectors' arguments: poll_impl) */
static const size_t col_bytes[VDL2_NCOL] = { sizeof(vdl2gpu_level_t), sizeof(vdl2gpu_soft_t), sizeof(vdl2gpu_carrier_t), sizeof(vdl2gpu_blockrep_t), sizeof(vdl2gpu_fb_t),
					      sizeof(vdl2gpu_symclk_t), sizeof(vdl2gpu_trk_t) };
static const struct { unsigned flag; const char *flag_name, *arg; } col_info[VDL2_NCOL] = {	/* arg: what the collectors' error texts call the column */
	{ VDL2GPU_F_LEVELS, "VDL2GPU_F_LEVELS", "lv" },			/* a level record */
	{ VDL2GPU_F_SOFT_RS, "VDL2GPU_F_SOFT_RS", "soft" },		/* a reliability map (2048 bytes) */
	{ VDL2GPU_F_CARRIER, "VDL2GPU_F_CARRIER", "car" },		/* a carrier record */
	{ VDL2GPU_F_BLOCK_REPORT, "VDL2GPU_F_BLOCK_REPORT", "rep" },	/* a block report (vdl2gpu_create: only with VDL2GPU_F_FRAMES) */
	{ VDL2GPU_F_FEEDBACK, "VDL2GPU_F_FEEDBACK", "fb" },		/* decision-feedback rows (2048 bytes; with or without VDL2GPU_F_FRAMES) */
	{ VDL2GPU_F_SYMCLK, "VDL2GPU_F_SYMCLK", "clk" },		/* a symbol-clock record (744 bytes) */
	{ VDL2GPU_F_TRACKED, "VDL2GPU_F_TRACKED", "trk" },		/* timing-tracked rows (2048 bytes; with or without VDL2GPU_F_FRAMES) */
};

/* A table set (push % VDL2_NSET): what a push's demodulator kernels work in, see alloc_sets. */
struct TableSet {
	K2Params k2{};		/* the set's 21 tables (cands ... items, ctl, fmask), its plane set, and every parameter that never changes */
	LaterEvent k2_done;		/* the end of the tail of the push that used the set */
	hipEvent_t f_done = nullptr;	/* FRONT of the push on the set has been enqueued up to its last kernel */
};
static inline int set_before(int par) { return (par + VDL2_NSET - 1) % VDL2_NSET; }	/* the set of the push before the one on set `par` */
static inline int set_after(int par) { return (par + 1) % VDL2_NSET; }			/* ... of the push after it */

/* An output ring (push % VDL2_NRING): the calling thread waits for the ring's previous push only three pushes later -- with two
 * rings it waited for the tail of the push before last in every call, and the GPU's front stream waited for the calling thread. */
struct OutRing {
	vdl2gpu_burst_t *d_recs = nullptr;
	void *d_side[VDL2_NCOL] = {};
	vdl2gpu_frame_t *d_frames = nullptr;	/* VDL2GPU_F_FRAMES: a byte buffer of compact entries */
	bool busy = false;
	hipEvent_t done2[2] = {};	/* the end of the push's tail: its records and counters are on the host.  Two events, used in turn (ev): a
					 * collector that waits for one with the handle lock released (wait_harvest) would otherwise wait on an
					 * event the producer may re-record for the push three later */
	int ev = 0;			/* which of the two the ring's current push recorded */
	LaterEvent in_read;		/* its channeliser has read the caller's device buffer (cleared by a push from host memory) */
	uint64_t push = 0;		/* which push filled the ring */
	size_t samples = 0;		/* samples (per stream) of that push */
	int slab = 0;			/* the slab its records were exported to */
	bool spec = false;		/* its K2d ran ahead of verify: honour the redo mask */
	hipEvent_t done() const { return done2[ev]; }
	template <class T> T *col(int k) const { return static_cast<T *>(d_side[k]); }	/* (nullptr: the handle has no column k) */
};

/* A slab (push % VDL2_NSLAB) of page-locked host memory, which the GPU itself fills at the end of the push (k_export_records), and
 * its device addresses.  One more than rings, so that a ring collected at the last moment -- by the call that is about to reuse it
 * -- still lies untouched in its slab while the caller polls once more, instead of being copied aside at once. */
struct Slab {
	vdl2gpu_burst_t *h_recs = nullptr, *d_recs = nullptr;
	uint8_t *h_side[VDL2_NCOL] = {};
	void *d_side[VDL2_NCOL] = {};
	size_t lo = 0, hi = 0;	/* ready_idx[lo, hi): where the handles into the slab lie (a push's are contiguous) */
	template <class T> T *col(int k) const { return static_cast<T *>(d_side[k]); }
};

/* Records in pageable storage, with their side columns (byte vectors: col_bytes[k] a record). */
struct RecQueue {
	std::vector<vdl2gpu_burst_t> recs;
	std::vector<uint8_t> side[VDL2_NCOL];
	void clear()
	{
		recs.clear();
		for (auto &s : side)
			s.clear();
	}
};

struct vdl2gpu {
	/* Every public call on the handle takes this lock (see "Threads" in include/vdl2gpu.h): the reference's shape -- the SDR
	 * library's callback thread committing blocks (rtl.c:274-295, 302) while another thread collects msgblk_t's -- works on one
	 * handle.  Recursive because public calls use each other (get_stats -> sync ...).  The blocking collectors release it while
	 * they wait for the GPU (wait_harvest). */
	std::recursive_mutex mu;
	vdl2gpu_config_t cfg;
	std::vector<vdl2gpu_chan_t> chans;
	int S, C, L, maxwin, sdrclk;
	unsigned long long k1_launches[4] = {0, 0, 0, 0};	/* vdl2gpu_debug_k1: k1_channelise (table in LDS), k1_channelise (table in global memory), k1_pp, k1_fast */
	bool k1_glo = false;	/* k1_channelise reads the LO table from global memory (off-grid rates whose table does not fit LDS) */
	size_t sample_bytes;
	long long cap;		/* frames per stream per ping-pong buffer */
	/* what the handle owns: see dev_alloc ... release_owned */
	std::vector<void *> own_dev, own_host;
	std::vector<hipEvent_t> own_events;
	std::vector<hipStream_t> own_streams;
	hipStream_t stream = nullptr;
	/* host samples: two staging buffers in HBM, filled on a stream of their own, so that the copy of one
	 * push runs beside the channeliser of the one before */
	hipStream_t in_stream = nullptr;
	hipEvent_t raw_copied[2] = {nullptr, nullptr};
	void *d_raw[2] = {nullptr, nullptr};
	size_t raw_bytes[2] = {0, 0};
	/* ingest ring (rtl.c:274-295, air.c:191-217): pinned host slots the producer fills in place */
	void *ring_host = nullptr;
	size_t ring_slot_samples = 0, ring_slot_bytes = 0;
	int ring_nslots = 0;
	unsigned long long ring_next = 0;
	bool ring_acquired = false;
	std::vector<LaterEvent> ring_copied;	/* per slot: its copy to the GPU has left it (cleared once acquire has waited for it) */
	float2 *d_lo = nullptr;
	bool rot = false;		/* VDL2GPU_F_EXACT_FO with a channel off the 25 kHz grid: the rotating instantiations of the K1 kernels run */
	K1Rot k1rot{};			/* their second argument: the tables (create_impl), and the push's place in the schedule (push) */
	unsigned *d_rot_tab = nullptr;	/* [S][8][K1R_TAB] */
	float2 *d_rot_hi = nullptr, *d_rot_lo = nullptr;	/* T_hi, T_lo: one pair for all channels of the handle */
	unsigned *d_k1_tickets = nullptr;	/* k1_fast's work counters */
	std::vector<unsigned> k1_tbase;	/* [S][8] what they hold, per stream and XCD (the same for every role; the same for every stream between two calls) */
	int last_set = 0;		/* the table / plane set of the last push (the debug calls read it) */
	float2 *d_lo_ext = nullptr;	/* [S][8][8 + L + 40]: every LO table with its last 8 entries in front and its first 40 behind (k1_pp reads 8 at a time) */
	float2 *d_dec[VDL2_NSET] = {};	/* plane sets, used in turn (push % 3): a set is written by the channeliser two pushes after its last
							 * reader, the back stage's tail, was ENQUEUED -- with two sets the channeliser had to wait for that tail */
	StreamState *d_ss = nullptr;
	ChanState *d_cs = nullptr;
	ChanCfg *d_cfg = nullptr;
	uint8_t *d_pn = nullptr;
	uint8_t *d_pn8 = nullptr;	/* ... by payload byte (K2Params.pn8) */
	TableSet set[VDL2_NSET];
	OutRing ring[VDL2_NRING];
	OutCounters *d_outc = nullptr;
	hipStream_t copy_stream = nullptr;
	size_t ctl_words = 0;
	unsigned rec_cap = 0;
	unsigned item_cap = VDL2_ITEM_CAP, item_priv = VDL2_ITEM_PRIV;	/* K2Params.item_cap; of which private areas at most (create_impl) */
	int full_scan = 0;
	unsigned stage_cap = 0;
	int prim_drop = 0;	/* VDL2GPU_PRIM_DROP (tests) */
#ifndef VDL2_K2D_GRID
#define VDL2_K2D_GRID 64
#endif
	int k2d_grid = VDL2_K2D_GRID;	/* payload workgroups per channel (VDL2GPU_K2D_GRID): 64 -- half the chip's wavefront slots at the kernel's 119 registers.
					 * One workgroup per burst is a chain of latencies; 128 per channel held EVERY slot while the verify pass beside it
					 * waited for them (0.472 against 0.462 ms per step at 64, same box; 32 and 16: 0.468, 0.469) */
	int force_serial = 0;
	int quirk = 0;		/* VDL2GPU_F_RTL_QUIRK */
	int n_cu = 256;
	int probe_occ = 4;	/* resident k2a_probe workgroups per CU */
	bool stage_events = true;	/* per-stage HIP events (vdl2gpu_timing_t breakdown): an event record between two kernels of the chain
					 * costs ~3 us, so only every stage_every-th push carries them (the sums are scaled up in harvest) */
	int stage_every = 4;
	bool stage_dump = false;	/* VDL2GPU_STAGE_DUMP=1: events on every push, their times printed when the push is collected (harvest_timing) */
	hipEvent_t ev_origin = nullptr;
	LaterEvent k1_done[2];		/* per staging buffer (host input): the channeliser has read it */
	hipStream_t pay_stream = nullptr;	/* K2d beside the verify pass; then the push's TAIL (repair rounds, commit, export, counters: see enqueue_back) */
	hipEvent_t verify_done = nullptr;	/* main -> tail: the verify pass has run */
	LaterEvent k2f_done;			/* tail -> main: the channel states are committed */
	hipStream_t tail_prev = nullptr;	/* the stream the previous push's tail ran on */
	hipEvent_t k2c_done = nullptr, pay_done = nullptr;
	int repair_rounds = 0;		/* adapted floor..4 from how often the serial fallback was needed */
	int rounds_floor = 1;		/* one (resolver-only) repair round is always scheduled, see enqueue_back */
	size_t split_samples = 0;	/* pushes longer than this are cut into parts (36 s of air time), see push_checked; halved
					 * whenever a channel's candidate tables overflow */
	size_t split_default = 0;
	unsigned long long last_ovf_push = 0;
	double cand_dens[4] = {0, 0, 0, 0};	/* candidates per input sample of the busiest channel, last four parts collected */
	unsigned cand_dens_n = 0;
	size_t split_unit = 32768;	/* parts are multiples of this (k1_fast takes whole superperiods; the RTL quirk needs whole blocks) */
	unsigned redos_seen = 0, repairs_seen = 0;
	uint64_t last_redo_push = 0;
	unsigned long long *d_dbg = nullptr;
	HeadTap *d_headtap = nullptr;	/* VDL2GPU_F_DEBUG_HEADS: every trigger of the last push (any kernel) */
	unsigned *d_headtap_n = nullptr;
	unsigned headtap_cap = 0;
	uint64_t total_in = 0;		/* samples per stream pushed so far */
	uint64_t test_epoch = 0;	/* test build (VDL2GPU_TEST_EPOCH): where total_in starts, see include/vdl2gpu.h */
	unsigned test_ticket0 = 0;	/* test build (VDL2GPU_TEST_TICKET0): where k1_fast's work counters start */
	uint64_t pushes = 0;
	uint64_t overflowed = 0;
	std::vector<PushTiming> pending;
	std::vector<PushTiming> free_ev;
	vdl2gpu_timing_t tm{};
	RecQueue ready;		/* fetched, not yet handed out (storage order) */
	/* hand-out order, consumed from ready_pos: bits 32-33 = where the record lies (0: `ready`, 1 + slab: that slab),
	 * bits 0-31 = index there -- so that collecting a push's bursts is an index sort and ONE copy per record, into the
	 * caller's buffer (slot_of decodes a handle) */
	std::vector<uint64_t> ready_idx;
	Slab slab[VDL2_NSLAB];
	unsigned slab_cap = 0;
	size_t ready_pos = 0;
	/* block path in the pipeline (VDL2GPU_F_FRAMES) */
	bool frames_on = false;
	unsigned *d_k4tab = nullptr;	/* GF(256) and FCS tables of the block path */
	FrameCounters *d_fcnt = nullptr;	/* [VDL2_NRING] */
	unsigned frame_cap = 0;	/* bytes of a frame buffer (slots + arena) */

	std::vector<uint8_t> fready;		/* compact frame entries as k4_frames wrote them, storage order */
	std::vector<size_t> fready_idx;	/* hand-out order: byte offsets into `fready`, consumed from fready_pos */
	size_t fready_pos = 0;
	uint64_t frames_dropped = 0;
	vdl2gpu_burst_t *h_pin = nullptr;	/* pinned bounce buffer for record read-back */
	bool col_on[VDL2_NCOL] = {};	/* which side columns the handle has */
	double lev_k = 1.0;	/* K of vdl2gpu.h: power of a full-scale tone at the channel centre (VDL2GPU_F_LEVELS) */
	PushCounters *h_pin_cnt = nullptr;	/* [VDL2_NRING] pinned, written by k3_rebase */
	PushCounters *d_pin_cnt = nullptr;	/* its device address */
	unsigned pin_recs = 0;
	bool failed = false;	/* a HIP call failed while work was being enqueued: device and host state no longer agree */
	std::string err;
	double hprof[8] = {0, 0, 0, 0, 0, 0, 0, 0};	/* VDL2GPU_HOST_PROF: seconds of the calling thread in the segments of push_impl (printed at destroy) */
	bool hprof_on = false;
	uint64_t hprof_push0 = 0;	/* pushes at the last reset of hprof[] */
	/* Environment knobs, read ONCE in create_impl (INTEGRATION.md lists them): no other function reads the environment.
	 * The test handicaps (VDL2GPU_PRIM_DROP, VDL2GPU_SPLIT_SAMPLES, VDL2GPU_F_TEST_NOREGION) exist only in the
	 * library built with -DVDL2GPU_TESTHOOKS (libvdl2gpu_test.so, which the tests load). */
	struct {
		bool no_k1_fast = false;	/* VDL2GPU_NO_K1_FAST: general channeliser only */
		bool no_tail = false;		/* VDL2GPU_NO_TAIL: everything behind the verify pass stays on the main stream */
		bool no_whole_pp = false;	/* VDL2GPU_NO_WHOLE_PP: 5/6/10 MS/s pushes always run their first and last period through the general channeliser (round 4) */
		double table_fill = 0.90;	/* VDL2GPU_TABLE_FILL (percent): how full the busiest channel's candidate table may get before parts are shortened */
		bool k1_pp = false;		/* VDL2GPU_K1_PP: k1_pp at 2 MS/s as well */
		bool debug_counters = false;	/* VDL2GPU_DEBUG_COUNTERS: cycle counters of the demodulator kernels */
		bool split_fixed = false;	/* (test hook) the part length was given: do not adapt it */
		int k1f_nfam = 0;		/* VDL2GPU_K1F_NFAM */
		int verify2_wg = 8;		/* VDL2GPU_VERIFY2_WG: workgroups per channel of the local repair round's verify pass */
		int k1_nsub = 0;		/* VDL2GPU_K1_NSUB */
#ifdef VDL2GPU_TESTHOOKS
		int test_item_grid = 0;		/* VDL2GPU_TEST_ITEM_GRID: few scan workgroups with the smallest private areas -- most items take the common area's path */
		int test_item_common = 0;	/* VDL2GPU_TEST_ITEM_COMMON: a common area of so many items -- the list overflows */
		int test_item_verify = 0;	/* VDL2GPU_TEST_ITEM_VERIFY: the two above for the verify passes only */
		/* VDL2GPU_TEST_{REG,SEG,VIS,WIN,MERGE,SLOG}_CAP: what a list of the back stage holds (K2Params.lim_*; 0 or more than its size: its size);
		 * VDL2GPU_TEST_STAGE_DYN: dynamic descriptor slots behind the static ones (0 or more than there are: all of them) */
		int test_reg_cap = 0, test_seg_cap = 0, test_vis_cap = 0, test_win_cap = 0, test_merge_cap = 0, test_slog_cap = 0, test_stage_dyn = 0;
#endif
	} knob;
	/* A push's work is three stages on three streams, and three pushes are in the pipeline at once -- the planes, the tables
	 * (candidates, clusters, descriptors, control words ...) and the output rings exist three times:
	 *   FRONT (fstream): channeliser, scan of one class + regions, sort, carry copy -- wide kernels that need
	 *                    nothing of the previous push's RESULT: the scan starts at the first carried frame and in a fixed
	 *                    class (what the resolver consumes is decided by where it stands, not by where the scan began),
	 *                    the stream-time base is the host's arithmetic, the carry is a fixed 49152 frames;
	 *   BACK  (stream):  clusters, resolver, verify pass (+ payload decode beside it): the resolver needs the channel state
	 *                    the previous push's tail committed (k2f_done);
	 *   TAIL  (pay_stream): repair round, commit, block path, export, counters (enqueue_back).
	 * FRONT(N+1) runs beside BACK(N) and TAIL(N-1): the one-workgroup-per-channel kernels (resolver, commit ...) no longer
	 * leave the GPU idle, and the channeliser's planes are still in the Infinity Cache when the scan reads them.  Pushes too short
	 * for the parallel path (the live path: one SDR block) keep everything on the one stream: a hop costs ~30 us. */
	struct Back {
		bool valid = false;
		K2Params k2{};
		int64_t J = 0;
		int par = 0, ring = 0, slab = 0;
		bool serial = false, two_streams = false;
		bool spec = false;	/* the payloads are decoded beside the verify pass, ahead of its verdict (push_impl decides; K2Params.sel_reserved) */
		unsigned tiles = 0;
		size_t pt_index = 0;	/* its PushTiming in `pending` */
	} back;
	hipStream_t fstream = nullptr;
	LaterEvent k1_ev;		/* channeliser + carry copy of the latest push that kept to the main stream */
	hipEvent_t f_tail = nullptr;	/* the end of the latest front stage on fstream (carry copy included) */
	bool last_two_streams = false;
	int64_t last_J = 0;	/* outputs of the previous push: where its last 49152 frames lie */
	/* stage sums of the pushes that carried stage events, unscaled, and how many those were */
	double st_scan = 0, st_cluster = 0, st_resolve = 0, st_demod = 0, st_other = 0, st_k1 = 0;
	uint64_t st_pushes = 0;
};

int LaterEvent::record(vdl2gpu_t *h, hipStream_t s) { HIPCHK(h, hipEventRecord(ev, s)); recorded = true; return VDL2GPU_OK; }
int LaterEvent::wait(vdl2gpu_t *h, hipStream_t s) const { if (recorded) HIPCHK(h, hipStreamWaitEvent(s, ev, 0)); return VDL2GPU_OK; }
int LaterEvent::sync(vdl2gpu_t *h) const { if (recorded) HIPCHK(h, hipEventSynchronize(ev)); return VDL2GPU_OK; }

/* ------------------------------------------------------------ pure host helpers */
extern "C" unsigned int reversebits(const unsigned int bits, const int n)
{
	unsigned int r = 0;
	for (int i = 0; i < n; ++i)
		r |= ((bits >> i) & 1u) << (n - 1 - i);
	return r;
}

/* Length of the LO table: the period of cexpf(-n*Fo*I) in n for a channel offset on the 25 kHz grid,
 * SDRINRATE / gcd(SDRINRATE, 25000).  Where 25 kHz divides the rate that is the reference's SDRINRATE/STEPRATE
 * (d8psk.c:348); off that grid the reference's table is no whole period (a phase jump every 81 samples at
 * 2.048 MS/s), and the formula is carried over its true period instead: 2048 entries there. */
extern "C" int vdl2gpu_lo_len(unsigned sdrinrate)
{
	unsigned a = sdrinrate, b = 25000u;
	while (b) {
		const unsigned t = a % b;
		a = b;
		b = t;
	}
	return a ? (int)(sdrinrate / a) : 0;
}

/* d8psk.c:353-357: wf[n] = cexpf(-n*Fo*I) with Fo narrowed to float.  cexpf of a
 * purely imaginary argument is (cos, sin) from libm's sincosf. */
extern "C" int vdl2gpu_lo_table(unsigned sdrinrate, int fo_hz, float *out_re_im, int max_complex)
{
	const int L = vdl2gpu_lo_len(sdrinrate);
	if (L <= 0 || L > max_complex)
		return VDL2GPU_EINVAL;
	const float w = (float)((double)((float)fo_hz / (float)sdrinrate) * 2.0 * M_PI);
	for (int n = 0; n < L; ++n) {
		const float y = (float)(-n) * w;
		float sn, cs;
		sincosf(y, &sn, &cs);
		out_re_im[2 * n] = cs;
		out_re_im[2 * n + 1] = sn;
	}
	return L;
}

/* Decimation schedule of one push, pure integer arithmetic:
 * given the number of samples already consumed, where does the push start in
 * the 21/SDRCLK clock, the LO period and the current integrate-and-dump window,
 * and how many 84 kS/s outputs complete inside it. */
extern "C" int vdl2gpu_plan(uint64_t total_in, uint64_t n, unsigned sdrclk, unsigned lo_len,
			    int *c0, int *no0, int *nf0, int64_t *nout)
{
	if (!sdrclk || !lo_len || sdrclk <= 21)
		return VDL2GPU_EINVAL;
	const unsigned __int128 t21 = (unsigned __int128)total_in * 21u;
	const uint64_t done = (uint64_t)(t21 / sdrclk);	/* outputs completed before this push */
	*c0 = (int)(uint64_t)(t21 % sdrclk);
	*no0 = (int)(total_in % lo_len);
	/* first input index after output (done-1): ceil(done*sdrclk/21) */
	const unsigned __int128 num = (unsigned __int128)done * sdrclk;
	const uint64_t first = (uint64_t)((num + 20) / 21);
	*nf0 = (int)(total_in - first);
	*nout = (int64_t)(((uint64_t)*c0 + 21ull * n) / sdrclk);
	return VDL2GPU_OK;
}

/* VDL2GPU_F_EXACT_FO (include/vdl2gpu.h): the two tables of the residual oscillator, angle -pi k / R for the phase index k < 2 R
 * split as k = 4096 h + l; double precision narrowed once.  Either table may be NULL (the call then only returns T_hi's length). */
extern "C" int vdl2gpu_exact_fo_tables(unsigned sdrinrate, float *hi_re_im, int max_hi, float *lo_re_im)
{
	if (!sdrinrate || sdrinrate > (1u << 30))
		return VDL2GPU_EINVAL;
	const int nhi = (int)((2ull * sdrinrate + 4095) / 4096);
	if (hi_re_im && max_hi < nhi)
		return VDL2GPU_EINVAL;
	const double R = (double)sdrinrate;
	if (hi_re_im)
		for (int h = 0; h < nhi; ++h) {
			const double th = -M_PI * (double)(4096ull * (unsigned)h) / R;
			hi_re_im[2 * h] = (float)cos(th);
			hi_re_im[2 * h + 1] = (float)sin(th);
		}
	if (lo_re_im)
		for (int l = 0; l < 4096; ++l) {
			const double th = -M_PI * (double)l / R;
			lo_re_im[2 * l] = (float)cos(th);
			lo_re_im[2 * l + 1] = (float)sin(th);
		}
	return nhi;
}

/* ... and the phase index of the window whose first and last inputs are samples a and e of the stream:
 * (fd * ((a + e) mod 2 R)) mod 2 R with fd = fd_hz mod 2 R taken non-negative */
extern "C" int64_t vdl2gpu_exact_fo_index(uint64_t a, uint64_t e, unsigned sdrinrate, int fd_hz)
{
	if (!sdrinrate || sdrinrate > (1u << 30))
		return VDL2GPU_EINVAL;
	const uint64_t M = 2ull * sdrinrate;
	int64_t f = (int64_t)fd_hz % (int64_t)M;
	if (f < 0)
		f += (int64_t)M;
	const uint64_t sum = (a % M + e % M) % M;
	return (int64_t)(((unsigned __int128)(uint64_t)f * sum) % M);
}

/* the 25 kHz grid point a channel offset is mixed with under VDL2GPU_F_EXACT_FO: 25000 * floor((Fo + 12500) / 25000) */
static int exact_fo_grid(int fo)
{
	const long long t = (long long)fo + 12500;
	return (int)(25000 * (t >= 0 ? t / 25000 : -((-t + 24999) / 25000)));
}

/* chooseFc() of rtl.c:123-160 (the tuner centre for a list of channel frequencies) and the mixer offsets of
 * rtl.c:245-247.  The reference walks Fc down in 1 Hz steps from max + 50 kHz to min - 50 kHz and takes the first
 * value at which every channel is within SDRINRATE/2 - 50 kHz of Fc, none is closer than 50 kHz, and no two
 * neighbouring (sorted) channels are mirror images; if none qualifies the loop ends with Fc = min - 50 kHz, which
 * the reference then uses (reproduced, not fixed).  Parity unpinned: rtl.c needs rtl-sdr.h. */
extern "C" int vdl2gpu_choose_fc_rtl(const unsigned *fr, int nbch, unsigned sdrinrate, unsigned *fc, int *fo)
{
	if (!fr || !fc || nbch < 1 || nbch > VDL2GPU_MAXCH || sdrinrate < 200000)
		return VDL2GPU_EINVAL;
	const int step = 25000;		/* STEPRATE, vdlm2.h:33 */
	unsigned fd[VDL2GPU_MAXCH];
	for (int n = 0; n < nbch; ++n)
		fd[n] = fr[n];
	std::sort(fd, fd + nbch);	/* rtl.c:128-140 */
	*fc = 0;
	if (fd[nbch - 1] - fd[0] > sdrinrate - 4u * step) {	/* rtl.c:142-145: "Frequencies too far apart" */
		if (fo)
			for (int n = 0; n < nbch; ++n)
				fo[n] = 0;
		return VDL2GPU_OK;
	}
	int c, n = 0;
	for (c = (int)fd[nbch - 1] + 2 * step; c > (int)fd[0] - 2 * step; --c) {	/* rtl.c:147-158, int arithmetic as there */
		for (n = 0; n < nbch; ++n) {
			if (std::abs(c - (int)fd[n]) > (int)(sdrinrate / 2) - 2 * step)
				break;
			if (std::abs(c - (int)fd[n]) < 2 * step)
				break;
			if (n > 0 && c - (int)fd[n - 1] == (int)fd[n] - c)
				break;
		}
		if (n == nbch)
			break;
	}
	*fc = (unsigned)c;
	if (fo)
		for (int i = 0; i < nbch; ++i)
			fo[i] = (int)fr[i] - c;	/* rtl.c:245-247 */
	return VDL2GPU_OK;
}

/* chooseFc() of air.c:47-70 and the mixer offsets of air.c:182-184.  Parity unpinned: air.c needs airspy.h. */
extern "C" int vdl2gpu_choose_fc_air(const unsigned *fr, int nbch, unsigned sdrinrate, unsigned *fc, int *fo, int *r10, int *r11)
{
	if (!fr || !fc || nbch < 1 || nbch > VDL2GPU_MAXCH)
		return VDL2GPU_EINVAL;
	static const unsigned hf[] = {1953050, 1980748, 2001344, 2032592, 2060291, 2087988};	/* r820t_hf, air.c:44 */
	static const unsigned lf[] = {525548, 656935, 795424, 898403, 1186034, 1502073, 1715133, 1853622};	/* r820t_lf, air.c:45 */
	const unsigned step = 25000;
	unsigned minf = 140000000u, maxf = 0;	/* air.c:77, 96-97 */
	for (int n = 0; n < nbch; ++n) {
		minf = std::min(minf, fr[n]);
		maxf = std::max(maxf, fr[n]);
	}
	const unsigned bw = maxf - minf + 2 * step;
	unsigned off = 0;
	if (r10)
		*r10 = 0;
	if (r11)
		*r11 = 0;
	*fc = 0;
	if (sdrinrate == 5000000) {	/* the R820T2 of the Airspy R2, air.c:53-66 */
		int i, j;
		for (i = 7; i >= 0; --i)
			if (hf[5] - lf[i] >= bw)
				break;
		if (i < 0) {	/* air.c:57: return 0 */
			if (fo)
				for (int n = 0; n < nbch; ++n)
					fo[n] = 0;
			return VDL2GPU_OK;
		}
		for (j = 5; j >= 0; --j)
			if (hf[j] - lf[i] <= bw)
				break;
		++j;
		if (j > 5)	/* cannot happen: hf[5] - lf[i] >= bw and the test is <=; only equality leaves j = 5 -> 6 */
			j = 5;
		off = (hf[j] + lf[i]) / 2 - sdrinrate / 4;
		if (r10)
			*r10 = 0xB0 | (15 - j);
		if (r11)
			*r11 = 0xE0 | (15 - i);
	}
	*fc = ((maxf + minf) / 2 + off + step / 2) / step * step;	/* air.c:69 */
	if (fo) {
		const unsigned f0 = *fc + sdrinrate / 4;	/* air.c:182 */
		for (int n = 0; n < nbch; ++n)
			fo[n] = (int)(fr[n] - f0);
	}
	return VDL2GPU_OK;
}

/* stream time (84 kS/s index) -> index of the input sample that completed it */
static int64_t dec_to_sample(int64_t m, unsigned sdrclk)
{
	if (m < 0)
		return m;
	return (int64_t)((((unsigned __int128)(uint64_t)(m + 1)) * sdrclk + 20) / 21) - 1;
}

extern "C" int vdl2gpu_abi_version(void)
{
	return VDL2GPU_ABI_VERSION;
}

extern "C" const char *vdl2gpu_strerror(int code)
{
	switch (code) {
	case VDL2GPU_OK: return "ok";
	case VDL2GPU_EINVAL: return "invalid argument";
	case VDL2GPU_EHIP: return "HIP runtime error";
	case VDL2GPU_ENOMEM: return "out of memory";
	case VDL2GPU_EOVERFLOW: return "burst record ring overflow";
	case VDL2GPU_ENODEV: return "no HIP device (there is no CPU fallback)";
	default: return "unknown error";
	}
}

#define HLOCK(h) std::unique_lock<std::recursive_mutex> hlock_((h)->mu)

/* why this thread's last vdl2gpu_create refused its configuration, where it says (there is no handle to keep the text in) */
static thread_local const char *create_err = nullptr;

extern "C" const char *vdl2gpu_last_error(vdl2gpu_t *h)
{
	if (!h)
		return create_err ? create_err : "null handle";
	HLOCK(h);
	return h->err.c_str();	/* (valid until the next call on the handle, from any thread) */
}

/* msgblk_t, vdlm2.h:39-47, LP64: prev@0(8) chn@8 Fr@12 tv@16(16) ppm@32 nbrow@36 nlbyte@40 data@44 */
extern "C" int vdl2gpu_burst_to_msgblk(const vdl2gpu_burst_t *b, void *msgblk, size_t msgblk_size)
{
	if (!b || !msgblk || msgblk_size < VDL2GPU_MSGBLK_SIZE)
		return VDL2GPU_EINVAL;
	char *m = (char *)msgblk;	/* the offsets are held against the reference's own header at build time (see VDL2GPU_MSGBLK_SIZE in include/vdl2gpu.h) */
	memcpy(m + VDL2GPU_MSGBLK_OFF_CHN, &b->chn, 4);
	memcpy(m + VDL2GPU_MSGBLK_OFF_FR, &b->Fr, 4);
	memcpy(m + VDL2GPU_MSGBLK_OFF_PPM, &b->ppm, 4);
	memcpy(m + VDL2GPU_MSGBLK_OFF_NBROW, &b->nbrow, 4);
	memcpy(m + VDL2GPU_MSGBLK_OFF_NLBYTE, &b->nlbyte, 4);
	memcpy(m + VDL2GPU_MSGBLK_OFF_DATA, b->data, VDL2GPU_MAXROWS * VDL2GPU_ROWLEN);
	return VDL2GPU_OK;
}

/* ------------------------------------------------------------------- lifecycle */
/* bytes per sample of a format; 0: no such format.  (The kernels' own table is K1Fmt<FMT>::BYTES: held to this one below.) */
constexpr static size_t fmt_bytes(int fmt)
{
	switch (fmt) {
	case VDL2GPU_FMT_CU8: return 2;
	case VDL2GPU_FMT_CS16: return 4;
	case VDL2GPU_FMT_CF32: return 8;
	case VDL2GPU_FMT_F32R: return 4;
	case VDL2GPU_FMT_CS8: return 2;
	case VDL2GPU_FMT_S16R: return 2;
	default: return 0;
	}
}
#define FMT_BYTES_AGREE(F_) static_assert(fmt_bytes(F_) == K1Fmt<F_>::BYTES, "fmt_bytes and K1Fmt disagree on " #F_)
FMT_BYTES_AGREE(VDL2GPU_FMT_CU8);
FMT_BYTES_AGREE(VDL2GPU_FMT_CS16);
FMT_BYTES_AGREE(VDL2GPU_FMT_CF32);
FMT_BYTES_AGREE(VDL2GPU_FMT_F32R);
FMT_BYTES_AGREE(VDL2GPU_FMT_CS8);
FMT_BYTES_AGREE(VDL2GPU_FMT_S16R);
#undef FMT_BYTES_AGREE

/* Everything a handle creates on the device, in page-locked memory, as an event or as a stream is made here and recorded in the
 * handle; release_owned() is the one place that gives it back.  Callers keep their plain pointers, and use the macros, which
 * name the object in the error text (vdl2gpu_last_error says WHICH allocation failed). */
static int hip_failed(vdl2gpu_t *h, const char *what, hipError_t e)
{
	h->err = std::string(what) + ": " + hipGetErrorString(e);
	return VDL2GPU_EHIP;
}

template <class T> static int dev_alloc(vdl2gpu_t *h, T **p, size_t bytes, const char *what)
{
	void *q = nullptr;
	const hipError_t e = hipMalloc(&q, bytes);
	if (e != hipSuccess)
		return hip_failed(h, what, e);
	h->own_dev.push_back(q);
	*p = static_cast<T *>(q);
	return VDL2GPU_OK;
}
#define DEV_ALLOC(h, p, bytes) TRY(dev_alloc(h, &(p), bytes, "hipMalloc(&" #p ", " #bytes ")"))

/* give one of them back early (a staging buffer that has to grow) */
static void dev_release(vdl2gpu_t *h, const void *p)
{
	auto it = std::find(h->own_dev.begin(), h->own_dev.end(), p);
	if (it == h->own_dev.end())
		return;
	(void)hipFree(*it);
	h->own_dev.erase(it);
}

template <class T> static int host_alloc(vdl2gpu_t *h, T **p, size_t bytes, unsigned flags, const char *what)
{
	void *q = nullptr;
	const hipError_t e = hipHostMalloc(&q, bytes, flags);
	if (e != hipSuccess)
		return hip_failed(h, what, e);
	h->own_host.push_back(q);
	*p = static_cast<T *>(q);
	return VDL2GPU_OK;
}
#define HOST_ALLOC(h, p, bytes, flags) TRY(host_alloc(h, &(p), bytes, flags, "hipHostMalloc(&" #p ", " #bytes ", " #flags ")"))

static int new_event(vdl2gpu_t *h, hipEvent_t *ev, const char *what, bool timing = false)
{
	const hipError_t e = hipEventCreateWithFlags(ev, timing ? hipEventDefault : hipEventDisableTiming);
	if (e != hipSuccess)
		return hip_failed(h, what, e);
	h->own_events.push_back(*ev);
	return VDL2GPU_OK;
}
#define NEW_EVENT(h, ev, ...) TRY(new_event(h, &(ev), "hipEventCreate(&" #ev ")", ##__VA_ARGS__))

/* a non-blocking stream: of priority *prio, or of the default one */
static int new_stream(vdl2gpu_t *h, hipStream_t *s, const char *what, const int *prio = nullptr)
{
	const hipError_t e = prio ? hipStreamCreateWithPriority(s, hipStreamNonBlocking, *prio) : hipStreamCreateWithFlags(s, hipStreamNonBlocking);
	if (e != hipSuccess)
		return hip_failed(h, what, e);
	h->own_streams.push_back(*s);
	return VDL2GPU_OK;
}
#define NEW_STREAM(h, s, ...) TRY(new_stream(h, &(s), "hipStreamCreate(&" #s ")", ##__VA_ARGS__))

static void release_owned(vdl2gpu_t *h)
{
	for (hipStream_t s : h->own_streams)
		(void)hipStreamSynchronize(s);
	for (hipEvent_t e : h->own_events)
		(void)hipEventDestroy(e);
	for (void *p : h->own_dev)
		(void)hipFree(p);
	for (void *p : h->own_host)
		(void)hipHostFree(p);
	for (hipStream_t s : h->own_streams)
		(void)hipStreamDestroy(s);
}

extern "C" void vdl2gpu_destroy(vdl2gpu_t *h)
{
	if (h && h->hprof_on && h->pushes)
		fprintf(stderr, "vdl2gpu host profile, ms per push over %llu pushes: wait for the buffer of the push before last %.3f, channeliser enqueue %.3f, "
				"collect the ring %.3f, front stage enqueue %.3f, spill %.3f, back stage enqueue %.3f; waiting for rings' events (push and poll calls) %.3f\n", (unsigned long long)h->pushes,
			h->hprof[0] / h->pushes * 1e3, h->hprof[1] / h->pushes * 1e3, h->hprof[2] / h->pushes * 1e3, h->hprof[3] / h->pushes * 1e3,
			h->hprof[4] / h->pushes * 1e3, h->hprof[5] / h->pushes * 1e3, h->hprof[6] / h->pushes * 1e3);
	if (!h)
		return;
	(void)hipSetDevice(h->cfg.device);
	release_owned(h);
	delete h;
}

/* Frames of one channel plane: the carry, the longest push (max_push at SDRCLK, 21 frames per SDRCLK samples) and slack, on whole
 * 128-byte lines.  vdl2gpu_create refuses a handle whose 8 planes of a stream reach VDL2_PLANES_MAX bytes; 0 = max_push so large
 * that the count itself would overflow. */
static long long plane_frames(uint64_t max_push, unsigned sdrclk)
{
	if (max_push > ~0ull / 21)
		return 0;
	const long long jmax = (long long)((21ull * max_push) / sdrclk) + 2;
	return (VDL2_CARRY_FRAMES + jmax + 64 + 15) / 16 * 16;
}

/* k1_fast addresses the planes of a stream with 32-bit byte offsets from the stream's first plane; every other kernel uses 64-bit
 * ones.  The limit is part of the ABI (include/vdl2gpu.h, max_push). */
#define VDL2_PLANES_MAX (1ull << 32)

/* k1_channelise keeps the LO table ((L + maxwin) x 8 channels) and a pass's input windows (32 outputs x maxwin) in dynamic LDS; both
 * grow with SDRINRATE and SDRCLK.  The library is built for gfx950 only, where a workgroup may have 160 KiB
 * (hipDeviceAttributeMaxSharedMemoryPerBlock on the MI355X); the kernel has no static LDS.  vdl2gpu_create refuses what it could
 * not launch (include/vdl2gpu.h, sdrinrate). */
#define VDL2_K1_LDS_MAX (160u * 1024u)
static size_t k1_smem_bytes(uint64_t L, uint64_t maxwin)
{
	return (size_t)(((L + maxwin) * VDL2_CS + (uint64_t)K1_OPB * maxwin) * sizeof(float2));
}
/* Rates off the 25 kHz grid have LO tables of thousands of entries (vdl2gpu_lo_len), which need not fit beside the windows:
 * what must fit is the window part of the bound above (the table's maxwin rows of wrap-around and the pass's windows); where the
 * whole does not, the handle runs the variant of k1_channelise that leaves the table in global memory (k1_glo_table). */
static size_t k1_win_bytes(uint64_t maxwin)
{
	return k1_smem_bytes(0, maxwin);
}
/* dynamic LDS of that variant: the pass's windows and the staging tile of LO values, 256 * maxwin + 32 KiB.  Within the limit
 * wherever k1_win_bytes (320 * maxwin) is: both reach 160 KiB at maxwin = 512 */
static size_t k1_glo_smem_bytes(uint64_t maxwin)
{
	return (size_t)(((uint64_t)K1_OPB * maxwin + (uint64_t)K1G_T * K1_THREADS) * sizeof(float2));
}
static_assert(((size_t)K1_OPB * 512 + (size_t)K1G_T * K1_THREADS) * sizeof(float2) <= VDL2_K1_LDS_MAX, "k1_channelise<.., true>: windows of 512 and the staging tile");

/* One kind of table for every set in turn (so the sets' tables lie as they always did: kind by kind). */
template <class T> static int alloc_table(vdl2gpu_t *h, T *K2Params::*m, size_t bytes, const char *what, bool zero = false)
{
	for (TableSet &t : h->set)
		TRY(dev_alloc(h, &(t.k2.*m), bytes, what));
	for (TableSet &t : h->set)
		if (zero)
			HIPCHK(h, hipMemsetAsync(t.k2.*m, 0, bytes, h->stream));
	return VDL2GPU_OK;
}

static const unsigned STAGE_DYN_SLOTS = 65536u;	/* the descriptor pool's dynamic tail behind the clusters' static slots (serial stretches, replays) */

/* The 21 tables of the table sets: a new table is its member of K2Params and a line here. */
#define ALLOC_TABLE(h, name, bytes, ...) TRY(alloc_table(h, &K2Params::name, bytes, "hipMalloc(&set[r].k2." #name ", " #bytes ")", ##__VA_ARGS__))
static int alloc_sets(vdl2gpu_t *h)
{
	const size_t SC = (size_t)h->S * VDL2_CS;
	ALLOC_TABLE(h, fmask, VDL2_FMASK_WORDS * sizeof(unsigned), true);
	ALLOC_TABLE(h, ctl, h->ctl_words * sizeof(unsigned), true);
	ALLOC_TABLE(h, cands, SC * VDL2_CAND_CAP * sizeof(Cand));
	ALLOC_TABLE(h, clusters, SC * VDL2_CAND_CAP * sizeof(Cluster));
	ALLOC_TABLE(h, clhead, SC * VDL2_CAND_CAP * sizeof(int2));
	ALLOC_TABLE(h, stage, (size_t)h->stage_cap * sizeof(BurstDesc));
	ALLOC_TABLE(h, sel_list, SC * VDL2_SEL_CAP * sizeof(unsigned));
	ALLOC_TABLE(h, sel_list2, SC * VDL2_SEL_CAP * sizeof(unsigned));
	ALLOC_TABLE(h, regs, SC * VDL2_REG_CAP * sizeof(int2));
	ALLOC_TABLE(h, segs, SC * VDL2_SEG_CAP * sizeof(Seg));
	ALLOC_TABLE(h, fail, SC * sizeof(int));
	ALLOC_TABLE(h, redo, SC * sizeof(int));
	ALLOC_TABLE(h, cs_out, SC * sizeof(ChanState));
	ALLOC_TABLE(h, skey, SC * VDL2_CAND_CAP * sizeof(int));
	ALLOC_TABLE(h, sidx, SC * VDL2_CAND_CAP * sizeof(unsigned short));
	ALLOC_TABLE(h, prim, SC * VDL2_CAND_CAP * sizeof(unsigned short));
	ALLOC_TABLE(h, seeds, SC * VDL2_CAND_CAP * sizeof(int));
	for (TableSet &t : h->set) {
		DEV_ALLOC(h, t.k2.onchain, SC * VDL2_CAND_CAP);
		DEV_ALLOC(h, t.k2.slog, SC * VDL2_SLOG_CAP * sizeof(K2Slog));
		DEV_ALLOC(h, t.k2.win, SC * VDL2_WIN_CAP * sizeof(int2));
	}
	ALLOC_TABLE(h, items, SC * h->item_cap * sizeof(K2aItem));
	return VDL2GPU_OK;
}

/* The K2Params every kernel of a push on a set starts from: beside the set's tables (alloc_sets), whatever never changes between
 * pushes; enqueue_front adds what is the push's.  Called when everything the parameters name exists. */
static void fill_set_params(vdl2gpu_t *h)
{
	for (int r = 0; r < VDL2_NSET; ++r) {
		K2Params &k = h->set[r].k2;
		k.dec = h->d_dec[r];
		k.cap = h->cap;
		k.nbch = h->C;
		k.nstreams = h->S;
		k.ss = h->d_ss;
		k.cs = h->d_cs;
		k.cfg = h->d_cfg;
		k.pn = h->d_pn;
		k.pn8 = h->d_pn8;
		k.sel_mode = SEL_FIRST;
		k.stage_cap = h->stage_cap;
		k.outc_total = &h->d_outc->total;
		k.rec_cap = h->rec_cap;
		k.probe_r = 0;				/* the one class scanned everywhere: fixed, not the class the channel is in */
		k.prim_drop = h->prim_drop;
		k.dbg = h->knob.debug_counters ? h->d_dbg : nullptr;
		k.headtap = h->d_headtap;
		k.headtap_n = h->d_headtap_n;
		k.headtap_cap = h->headtap_cap;
		k.full_scan = h->full_scan;
#ifdef VDL2GPU_TESTHOOKS
		k.test_noregion = (h->cfg.flags & VDL2GPU_F_TEST_NOREGION) ? 1 : 0;
		{
			/* a hook may only lower a limit: the lists keep their sizes */
			auto lim = [](int hook, int size) { return hook > 0 && hook < size ? hook : size; };
			k.lim_reg = lim(h->knob.test_reg_cap, VDL2_REG_CAP);
			k.lim_seg = lim(h->knob.test_seg_cap, VDL2_SEG_CAP);
			k.lim_vis = lim(h->knob.test_vis_cap, K2C_VIS);
			k.lim_win = lim(h->knob.test_win_cap, VDL2_WIN_CAP);
			k.lim_merge = lim(h->knob.test_merge_cap, K2S_MERGE);
			k.lim_slog = lim(h->knob.test_slog_cap, VDL2_SLOG_CAP);
			k.stage_cap = h->stage_cap - STAGE_DYN_SLOTS + (unsigned)lim(h->knob.test_stage_dyn, (int)STAGE_DYN_SLOTS);	/* (the pool keeps its size) */
		}
#endif
		k.round = 0;
		k.item_cap = h->item_cap;
		k.item_priv = h->item_priv;
		k.drain_slot = -1;
	}
}

/* The longest part push_checked makes of a push: 36 s of air time (split_default); a test build may ask for a third more
 * (VDL2GPU_SPLIT_SAMPLES).  The item lists are sized by the same two numbers. */
static const int PART_SECONDS = 36, TEST_PART_NUM = 4, TEST_PART_DEN = 3;

static int create_impl(vdl2gpu_t *h)
{
	const vdl2gpu_config_t &cfg = h->cfg;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg.device >= ndev) {
		h->err = "no HIP device";
		return VDL2GPU_ENODEV;
	}
	HIPCHK(h, hipSetDevice(cfg.device));
	{
		hipDeviceProp_t prop;
		if (hipGetDeviceProperties(&prop, cfg.device) == hipSuccess && prop.multiProcessorCount > 0)
			h->n_cu = prop.multiProcessorCount;
		int occ = 0;
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k2a_probe, K2A_THREADS, 0) == hipSuccess && occ > 0)
			h->probe_occ = occ;
	}
	int prio_lo = 0, prio_hi = 0;
	HIPCHK(h, hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
	NEW_STREAM(h, h->stream, &prio_hi);
	const int S = h->S, L = h->L;
	/* every environment knob is read here, once */
	auto env_int = [](const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; };
	h->full_scan = ((cfg.flags & VDL2GPU_F_FULLSCAN) || getenv("VDL2GPU_FULL_SCAN")) ? 1 : 0;
	h->stage_every = std::max(1, env_int("VDL2GPU_STAGE_EVERY", h->stage_every));
	h->stage_dump = env_int("VDL2GPU_STAGE_DUMP", 0) != 0;
	if (h->stage_dump)
		h->stage_every = 1;
	h->k2d_grid = std::max(1, env_int("VDL2GPU_K2D_GRID", h->k2d_grid));
	h->knob.no_k1_fast = getenv("VDL2GPU_NO_K1_FAST") != nullptr;
	h->hprof_on = getenv("VDL2GPU_HOST_PROF") != nullptr;
	h->knob.no_tail = getenv("VDL2GPU_NO_TAIL") != nullptr;
	h->knob.no_whole_pp = getenv("VDL2GPU_NO_WHOLE_PP") != nullptr;
	h->knob.table_fill = std::min(100, std::max(10, env_int("VDL2GPU_TABLE_FILL", 90))) / 100.0;
	h->knob.k1_pp = getenv("VDL2GPU_K1_PP") != nullptr;
	h->knob.debug_counters = getenv("VDL2GPU_DEBUG_COUNTERS") != nullptr;
	h->knob.k1f_nfam = env_int("VDL2GPU_K1F_NFAM", 0);
	h->knob.verify2_wg = std::max(1, env_int("VDL2GPU_VERIFY2_WG", 8));
	h->knob.k1_nsub = env_int("VDL2GPU_K1_NSUB", 0);
#ifdef VDL2GPU_TESTHOOKS
	h->prim_drop = env_int("VDL2GPU_PRIM_DROP", 0);
	h->knob.test_item_grid = env_int("VDL2GPU_TEST_ITEM_GRID", 0);
	h->knob.test_item_common = env_int("VDL2GPU_TEST_ITEM_COMMON", 0);
	h->knob.test_item_verify = env_int("VDL2GPU_TEST_ITEM_VERIFY", 0);
	h->knob.test_reg_cap = env_int("VDL2GPU_TEST_REG_CAP", 0);
	h->knob.test_seg_cap = env_int("VDL2GPU_TEST_SEG_CAP", 0);
	h->knob.test_vis_cap = env_int("VDL2GPU_TEST_VIS_CAP", 0);
	h->knob.test_win_cap = env_int("VDL2GPU_TEST_WIN_CAP", 0);
	h->knob.test_merge_cap = env_int("VDL2GPU_TEST_MERGE_CAP", 0);
	h->knob.test_slog_cap = env_int("VDL2GPU_TEST_SLOG_CAP", 0);
	h->knob.test_stage_dyn = env_int("VDL2GPU_TEST_STAGE_DYN", 0);
#endif
	/* A push in which a channel's verify pass fails with no round scheduled costs a serial redo of that channel's whole
	 * push (milliseconds), an idle round 30 us: with 16 channels or more an event somewhere is frequent enough that one
	 * round is always scheduled. */
	/* Parts (see push_checked): at most 36 s of air time; until the first pushes have been collected and their candidate
	 * density is known, 8.4 s -- a saturated channel (250 candidates a second) fills half of the tables in that long. */
	h->split_unit = ((cfg.flags & VDL2GPU_F_RTL_QUIRK) || h->sdrclk != 500 || h->L != 80) ? 32768 : K1F_PER_IN;
	/* other rates: whole periods of the dump schedule (4 * SDRCLK samples), so that a part that starts on a schedule boundary is ONE
	 * k1_pp launch like a whole push (choose_k1: whole_pp) -- unless the quirk wants whole 32768-sample blocks */
	if (!(cfg.flags & VDL2GPU_F_RTL_QUIRK) && h->split_unit == 32768 && (4 * h->sdrclk) % h->L == 0 && ((size_t)4 * h->sdrclk * h->sample_bytes) % 16 == 0)
		h->split_unit = (size_t)4 * h->sdrclk * ((32768 + (size_t)4 * h->sdrclk - 1) / ((size_t)4 * h->sdrclk));	/* (about the block's size) */
	h->split_default = (size_t)((double)PART_SECONDS * (double)h->cfg.sdrinrate) / h->split_unit * h->split_unit;
	{
		/* (until round 10 the verify pass mapped one workgroup to K2A_VRUN tiles and the item list has room for VDL2_MAXWG private areas: a
		 * part could not have more tiles than that covers -- 36 s of air time are 3003 tiles, the bound is 4088.  The pass covers a part
		 * with any grid now; the bound stays, it is what the lists were tested to) */
		const double max_frames = ((double)VDL2_MAXWG * K2A_VRUN - 4.0) * 2.0 * K2A_TS - 2.0 * K2A_TS - (double)VDL2_CARRY_FRAMES;
		const size_t max_part = (size_t)(max_frames * (double)h->sdrclk / 21.0) / h->split_unit * h->split_unit;
		h->split_default = std::min(h->split_default, max_part);
	}
	h->split_samples = std::max(h->split_unit, (size_t)(8.4 * (double)h->cfg.sdrinrate) / h->split_unit * h->split_unit);
#ifdef VDL2GPU_TESTHOOKS
	if (getenv("VDL2GPU_SPLIT_SAMPLES")) {
		h->split_samples = std::min((size_t)atoll(getenv("VDL2GPU_SPLIT_SAMPLES")), h->split_default * TEST_PART_NUM / TEST_PART_DEN);	/* (still inside the verify grid's bound) */
		h->knob.split_fixed = true;
	}
#endif
	h->rounds_floor = 1;	/* see enqueue_back */
	h->repair_rounds = env_int("VDL2GPU_REPAIR_ROUNDS", h->rounds_floor);
	h->force_serial = (cfg.flags & VDL2GPU_F_SERIAL) ? 1 : 0;
	h->quirk = (cfg.flags & VDL2GPU_F_RTL_QUIRK) ? 1 : 0;
	{
		/* The item lists (what passes a scan's first screen: 80 bytes an item, three sets) by the longest PART the handle can be given
		 * -- max_push, or what push_checked cuts longer pushes into (36 s of air time, a third more in a test build): 64 items of private
		 * areas per 1024-instant tile (the verify pass's and the probe's workgroups size theirs at 42 a tile: launch_scan), the
		 * common area half of that again.  A 67 MS push at 2 MS/s keeps round 5's 131 072 + 65 536 items per channel (126 MB a set and
		 * stream); a handle for pushes of a few MS 32 768 + 32 768 (42 MB). */
		const long long jmax = (long long)((21ull * cfg.max_push) / (unsigned)h->sdrclk) + 2;
		const long long jcap = (long long)PART_SECONDS * 84000 * TEST_PART_NUM / TEST_PART_DEN;	/* (84000 frames a second) */
		const long long tiles_max = (VDL2_CARRY_FRAMES + std::min(jmax, jcap)) / K2A_TS + 2;
		const unsigned priv = (unsigned)std::min<long long>(VDL2_ITEM_PRIV, std::max<long long>(32768, (64 * tiles_max + 4095) / 4096 * 4096));
		h->item_priv = priv;
		h->item_cap = priv + std::max(priv / 2, 32768u);	/* (the common area: what a stretch of sync words or a carrier sends past the private areas) */
	}
	h->k1_tbase.assign((size_t)S * 8, h->test_ticket0);
	h->cap = plane_frames(cfg.max_push, (unsigned)h->sdrclk);	/* planes start on 128-byte lines */
	const size_t dec_bytes = (size_t)S * (size_t)h->cap * VDL2_CS * sizeof(float2);
	for (int r = 0; r < VDL2_NSET; ++r) {
		DEV_ALLOC(h, h->d_dec[r], dec_bytes);
		HIPCHK(h, hipMemsetAsync(h->d_dec[r], 0, dec_bytes, h->stream));
	}
	DEV_ALLOC(h, h->d_lo, (size_t)S * VDL2_CS * L * sizeof(float2));
	DEV_ALLOC(h, h->d_lo_ext, (size_t)S * VDL2_CS * (L + 48) * sizeof(float2));
	DEV_ALLOC(h, h->d_k1_tickets, (size_t)S * 21 * 8 * sizeof(unsigned));
	HIPCHK(h, hipMemsetAsync(h->d_k1_tickets, 0, (size_t)S * 21 * 8 * sizeof(unsigned), h->stream));
#ifdef VDL2GPU_TESTHOOKS
	if (h->test_ticket0) {	/* VDL2GPU_TEST_TICKET0: the counters begin where the host's idea of them does (k1_tbase above) */
		const std::vector<unsigned> tk0((size_t)S * 21 * 8, h->test_ticket0);
		HIPCHK(h, hipMemcpyAsync(h->d_k1_tickets, tk0.data(), tk0.size() * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
		HIPCHK(h, hipStreamSynchronize(h->stream));	/* (tk0 ends with this block) */
	}
#endif
	DEV_ALLOC(h, h->d_ss, (size_t)S * sizeof(StreamState));
	DEV_ALLOC(h, h->d_cs, (size_t)S * VDL2_CS * sizeof(ChanState));
	DEV_ALLOC(h, h->d_cfg, (size_t)S * VDL2_CS * sizeof(ChanCfg));
	DEV_ALLOC(h, h->d_pn, VDL2_PN_BITS);
	for (OutRing &rg : h->ring)
		DEV_ALLOC(h, rg.d_recs, (size_t)h->rec_cap * sizeof(vdl2gpu_burst_t));
	DEV_ALLOC(h, h->d_outc, sizeof(OutCounters));
	HIPCHK(h, hipMemsetAsync(h->d_outc, 0, sizeof(OutCounters), h->stream));
	/* (HIP multiplexes its streams onto four hardware queues: a fifth stream shares one with another, and kernels that
	 * were meant to run side by side then run one behind the other -- this handle makes exactly main, copy, resolver, payload;
	 * host input adds one for its copies, which may share a queue with the record read-back) */
	const int prio_normal = 0;
	NEW_STREAM(h, h->copy_stream, &prio_normal);
	for (int r = 0; r < 2; ++r)
		NEW_EVENT(h, h->k1_done[r].ev);
	for (TableSet &t : h->set)
		NEW_EVENT(h, t.k2_done.ev);
	for (OutRing &rg : h->ring) {
		for (int k = 0; k < 2; ++k)
			NEW_EVENT(h, rg.done2[k]);
		NEW_EVENT(h, rg.in_read.ev);
	}
	NEW_STREAM(h, h->fstream, &prio_lo);	/* the back stage (main stream, high priority) is the shorter one: it goes first */
	for (TableSet &t : h->set)
		NEW_EVENT(h, t.f_done);
	NEW_EVENT(h, h->k1_ev.ev);
	NEW_EVENT(h, h->f_tail);
	NEW_STREAM(h, h->pay_stream);
	NEW_EVENT(h, h->k2c_done);
	NEW_EVENT(h, h->pay_done);
	NEW_EVENT(h, h->verify_done);
	NEW_EVENT(h, h->k2f_done.ev);
	h->ctl_words = VDL2_CTL_WORDS((size_t)S * VDL2_CS);
	h->stage_cap = (unsigned)S * VDL2_CS * VDL2_CAND_CAP * VDL2_CL_MAXB + STAGE_DYN_SLOTS;	/* static slots + dynamic tail */
	TRY(alloc_sets(h));
	h->pin_recs = std::min<unsigned>(h->rec_cap, 8192u);
	HOST_ALLOC(h, h->h_pin, (size_t)h->pin_recs * sizeof(vdl2gpu_burst_t), hipHostMallocDefault);
	h->slab_cap = std::min<unsigned>(h->rec_cap, 16384u);	/* 34 MB of page-locked memory per slab at most (four slabs); a push with more bursts takes the bounce buffer for the rest */
#ifdef VDL2GPU_TESTHOOKS
	h->slab_cap = std::max(1u, std::min<unsigned>(h->slab_cap, (unsigned)env_int("VDL2GPU_SLAB_CAP", (int)h->slab_cap)));	/* (tests: force the bounce path) */
#endif
	/* the output rings and the slabs: the records, and beside them the side columns the flags ask for */
	for (int k = 0; k < VDL2_NCOL; ++k)
		h->col_on[k] = (cfg.flags & col_info[k].flag) != 0;
	h->frames_on = (cfg.flags & VDL2GPU_F_FRAMES) != 0;
	if (h->frames_on) {
		unsigned arena = 4u << 20;
#ifdef VDL2GPU_TESTHOOKS
		arena = (unsigned)std::min(std::max(env_int("VDL2GPU_FRAME_ARENA", (int)arena), 64), (int)arena) & ~7u;	/* (tests: an arena a few entries fill) */
#endif
		h->frame_cap = h->rec_cap * K4_SLOT + arena;	/* bytes: a slot per record, and the arena (see K4Params) */
	}
	for (Slab &sl : h->slab) {
		HOST_ALLOC(h, sl.h_recs, (size_t)h->slab_cap * sizeof(vdl2gpu_burst_t), hipHostMallocMapped);
		HIPCHK(h, hipHostGetDevicePointer((void **)&sl.d_recs, sl.h_recs, 0));
	}
	for (int k = 0; k < VDL2_NCOL; ++k) {
		if (!h->col_on[k])
			continue;
		for (OutRing &rg : h->ring)
			DEV_ALLOC(h, rg.d_side[k], (size_t)h->rec_cap * col_bytes[k]);
		for (Slab &sl : h->slab) {
			HOST_ALLOC(h, sl.h_side[k], (size_t)h->slab_cap * col_bytes[k], hipHostMallocMapped);
			HIPCHK(h, hipHostGetDevicePointer(&sl.d_side[k], sl.h_side[k], 0));
		}
	}
	if (h->col_on[COL_LEVEL]) {
		/* K = (FS * sum_j mflt[4j])^2: the channeliser's integrate-and-dump AVERAGES the input samples of an output (D /= nf,
		 * d8psk.c:378), so a full-scale tone at the channel centre leaves it at FS, and the filter's gain there is the sum of the
		 * taps of one sub-phase */
		float mf[65];
		HIPCHK(h, hipMemcpyFromSymbol(mf, HIP_SYMBOL(c_mflt), sizeof mf));
		double g = 0.0;
		for (int j = 0; j <= 16; ++j)
			g += (double)mf[4 * j];
		const double fs = (cfg.fmt == VDL2GPU_FMT_CU8 || cfg.fmt == VDL2GPU_FMT_CS8) ? 128.0
			: ((cfg.fmt == VDL2GPU_FMT_CS16 || cfg.fmt == VDL2GPU_FMT_S16R) ? 32768.0 : 1.0);
		const double a = fs * g;
		h->lev_k = a * a;
	}
	HOST_ALLOC(h, h->h_pin_cnt, VDL2_NRING * sizeof(PushCounters), hipHostMallocMapped);
	memset(h->h_pin_cnt, 0, VDL2_NRING * sizeof(PushCounters));
	DEV_ALLOC(h, h->d_k4tab, K4_TABW * sizeof(unsigned));
	hipLaunchKernelGGL(k4_tables, dim3(1), dim3(64), 0, h->stream, h->d_k4tab);
	HIPCHK(h, hipGetLastError());
	if (h->frames_on) {
		for (OutRing &rg : h->ring)
			DEV_ALLOC(h, rg.d_frames, (size_t)h->frame_cap);
		DEV_ALLOC(h, h->d_fcnt, VDL2_NRING * sizeof(FrameCounters));
		HIPCHK(h, hipMemsetAsync(h->d_fcnt, 0, VDL2_NRING * sizeof(FrameCounters), h->stream));
	}
	HIPCHK(h, hipHostGetDevicePointer((void **)&h->d_pin_cnt, h->h_pin_cnt, 0));
	DEV_ALLOC(h, h->d_dbg, VDL2_DBG_WORDS * sizeof(unsigned long long));
	HIPCHK(h, hipMemsetAsync(h->d_dbg, 0, VDL2_DBG_WORDS * sizeof(unsigned long long), h->stream));
	if (cfg.flags & VDL2GPU_F_DEBUG_HEADS) {
		h->headtap_cap = 1u << 18;
		DEV_ALLOC(h, h->d_headtap, (size_t)h->headtap_cap * sizeof(HeadTap));
		DEV_ALLOC(h, h->d_headtap_n, sizeof(unsigned));
		HIPCHK(h, hipMemsetAsync(h->d_headtap_n, 0, sizeof(unsigned), h->stream));
	}

	std::vector<float2> lo((size_t)S * VDL2_CS * L, make_float2(0.f, 0.f));
	std::vector<ChanCfg> cc((size_t)S * VDL2_CS, ChanCfg{ 0, 0, 0, 0 });
	std::vector<float> tmp(2 * (size_t)L);
	for (int s = 0; s < S; ++s)
		for (int c = 0; c < h->C; ++c) {
			const vdl2gpu_chan_t &ch = h->chans[(size_t)s * h->C + c];
			/* VDL2GPU_F_EXACT_FO: the mixer takes the grid point next to Fo, the dump the rest (rot_tab below) */
			vdl2gpu_lo_table(cfg.sdrinrate, (cfg.flags & VDL2GPU_F_EXACT_FO) ? exact_fo_grid(ch.Fo) : ch.Fo, tmp.data(), L);
			for (int n = 0; n < L; ++n)
				lo[((size_t)s * VDL2_CS + c) * L + n] = make_float2(tmp[2 * n], tmp[2 * n + 1]);
			cc[(size_t)s * VDL2_CS + c] = ChanCfg{ ch.chn, ch.Fr, ch.Fo, 0 };
		}
	HIPCHK(h, hipMemcpyAsync(h->d_lo, lo.data(), lo.size() * sizeof(float2), hipMemcpyHostToDevice, h->stream));
	std::vector<float2> loe((size_t)S * VDL2_CS * (L + 48), make_float2(0.f, 0.f));
	for (size_t sc = 0; sc < (size_t)S * VDL2_CS; ++sc)
		for (int n = 0; n < L + 48; ++n)
			loe[sc * (L + 48) + n] = lo[sc * L + ((n + L - 8) % L)];
	HIPCHK(h, hipMemcpyAsync(h->d_lo_ext, loe.data(), loe.size() * sizeof(float2), hipMemcpyHostToDevice, h->stream));
	HIPCHK(h, hipMemcpyAsync(h->d_cfg, cc.data(), cc.size() * sizeof(ChanCfg), hipMemcpyHostToDevice, h->stream));
	std::vector<unsigned> rtab;	/* (these outlive the copies below: the stream is synchronised at the end) */
	std::vector<float> rhi, rlo;
	if (cfg.flags & VDL2GPU_F_EXACT_FO) {
		const unsigned R = cfg.sdrinrate, clk = (unsigned)h->sdrclk;
		const uint64_t M = 2ull * R;
		rtab.assign((size_t)S * VDL2_CS * K1R_TAB, 0u);
		for (int s = 0; s < S; ++s)
			for (int c = 0; c < h->C; ++c) {
				const int fo = h->chans[(size_t)s * h->C + c].Fo, fd = fo - exact_fo_grid(fo);
				unsigned *t = &rtab[((size_t)s * VDL2_CS + c) * K1R_TAB];
				for (unsigned i = 0; i < 21; ++i)	/* window i of the schedule's first period: inputs ceil(i clk / 21) .. ceil((i + 1) clk / 21) - 1 */
					t[i] = (unsigned)vdl2gpu_exact_fo_index(((uint64_t)i * clk + 20) / 21, ((uint64_t)(i + 1) * clk + 20) / 21 - 1, R, fd);
				t[21] = (unsigned)vdl2gpu_exact_fo_index(clk, clk, R, fd);	/* a period on: a + e grows by 2 SDRCLK */
				t[22] = (unsigned)(((int64_t)fd % (int64_t)M + (int64_t)M) % (int64_t)M);
				t[23] = fd != 0;
				h->rot = h->rot || fd != 0;
			}
	}
	if (h->rot) {
		const int nhi = vdl2gpu_exact_fo_tables(cfg.sdrinrate, nullptr, 0, nullptr);
		rhi.resize(2 * (size_t)nhi);
		rlo.resize(2 * 4096);
		vdl2gpu_exact_fo_tables(cfg.sdrinrate, rhi.data(), nhi, rlo.data());
		DEV_ALLOC(h, h->d_rot_tab, rtab.size() * sizeof(unsigned));
		DEV_ALLOC(h, h->d_rot_hi, rhi.size() * sizeof(float));
		DEV_ALLOC(h, h->d_rot_lo, rlo.size() * sizeof(float));
		HIPCHK(h, hipMemcpyAsync(h->d_rot_tab, rtab.data(), rtab.size() * sizeof(unsigned), hipMemcpyHostToDevice, h->stream));
		HIPCHK(h, hipMemcpyAsync(h->d_rot_hi, rhi.data(), rhi.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
		HIPCHK(h, hipMemcpyAsync(h->d_rot_lo, rlo.data(), rlo.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
		h->k1rot.tab = h->d_rot_tab;
		h->k1rot.hi = h->d_rot_hi;
		h->k1rot.lo = h->d_rot_lo;
		h->k1rot.M = 2u * cfg.sdrinrate;
		h->k1rot.rM = 1.0 / (double)h->k1rot.M;
	}

	/* scrambler sequence from seed 0x4D4B (d8psk.c:54-65, 299): identical for every burst */
	std::vector<uint8_t> pn(VDL2_PN_BITS);
	unsigned sc = 0x4D4B;
	for (size_t i = 0; i < pn.size(); ++i) {
		const unsigned b = (sc ^ (sc >> 14)) & 1u;
		sc = (sc << 1) | b;
		pn[i] = (uint8_t)b;
	}
	HIPCHK(h, hipMemcpyAsync(h->d_pn, pn.data(), pn.size(), hipMemcpyHostToDevice, h->stream));
	std::vector<uint8_t> pn8(2048, 0);	/* 2040 payload bytes at most (8 rows of 255) */
	for (size_t b = 0; b < pn8.size(); ++b)
		for (int i = 0; i < 8; ++i)
			if (25 + 8 * b + i < pn.size())
				pn8[b] |= (uint8_t)(pn[25 + 8 * b + i] << i);
	DEV_ALLOC(h, h->d_pn8, pn8.size());
	HIPCHK(h, hipMemcpyAsync(h->d_pn8, pn8.data(), pn8.size(), hipMemcpyHostToDevice, h->stream));

	fill_set_params(h);

	/* canonical start state: everything zero except initD8psk's perr=100 (d8psk.c:28-37);
	 * 16 zero frames stand for the empty Inbuff ring.  A test build's stream epoch (VDL2GPU_TEST_EPOCH) moves the same state
	 * to the stream time of sample test_epoch: d0 frames on (0 otherwise); everything the host derives from the samples so
	 * far follows from total_in (vdl2gpu_plan, the exact-Fo base and dec_base in push_impl, vdl2gpu_get_stats). */
	h->total_in = h->test_epoch;
	const long long d0 = (long long)(((unsigned __int128)h->test_epoch * 21u) / (unsigned)h->sdrclk);
	std::vector<StreamState> ss(S);
	memset(ss.data(), 0, ss.size() * sizeof(StreamState));
	for (auto &x : ss) {
		x.dec_base = d0 - VDL2_CARRY_FRAMES;	/* new output always starts at frame VDL2_CARRY_FRAMES; zeros before it */
		x.dec_fill = VDL2_CARRY_FRAMES;
	}
	std::vector<ChanState> cs((size_t)S * VDL2_CS);
	memset(cs.data(), 0, cs.size() * sizeof(ChanState));
	for (auto &x : cs) {
		x.pos = d0 + 1;	/* clk: 0 -> 4 (sample 0, idle) -> 8 (sample 1, evaluate) */
		x.r = 0;
		x.fresh = 0;	/* the all-zero start ring counts as history */
		x.perr = 100.0f;
	}
	HIPCHK(h, hipMemcpyAsync(h->d_ss, ss.data(), ss.size() * sizeof(StreamState), hipMemcpyHostToDevice, h->stream));
	HIPCHK(h, hipMemcpyAsync(h->d_cs, cs.data(), cs.size() * sizeof(ChanState), hipMemcpyHostToDevice, h->stream));
	HIPCHK(h, hipStreamSynchronize(h->stream));
	return VDL2GPU_OK;
}

extern "C" int vdl2gpu_create(const vdl2gpu_config_t *cfg, vdl2gpu_t **out)
{
	create_err = nullptr;
	if (!cfg || !out || cfg->struct_size != sizeof(vdl2gpu_config_t))
		return VDL2GPU_EINVAL;
	if (cfg->nbch < 1 || cfg->nbch > VDL2GPU_MAXCH || cfg->nstreams < 1 || !cfg->chan || !cfg->max_push)
		return VDL2GPU_EINVAL;
	if (fmt_bytes(cfg->fmt) == 0 || cfg->sdrinrate < 100000)
		return VDL2GPU_EINVAL;
	const bool offgrid = cfg->sdrinrate % 25000 != 0;	/* include/vdl2gpu.h, sdrinrate: "off the 25 kHz grid" */
	if (offgrid && (cfg->sdrinrate % 1000 || (cfg->flags & VDL2GPU_F_RTL_QUIRK)))
		return VDL2GPU_EINVAL;	/* (the quirk is the reference's RTL front end at its own rates) */
	if ((cfg->flags & VDL2GPU_F_RTL_QUIRK) && cfg->fmt != VDL2GPU_FMT_CU8)
		return VDL2GPU_EINVAL;	/* the quirk is in_callback()'s, and that only ever sees cu8 */
	if (cfg->flags & VDL2GPU_F_EXACT_FO) {
		if (cfg->flags & VDL2GPU_F_RTL_QUIRK)
			return VDL2GPU_EINVAL;	/* (the quirk is for parity with the reference, and that includes its LO's jumps) */
		for (size_t i = 0; i < (size_t)cfg->nstreams * cfg->nbch; ++i)
			if (2ll * std::llabs((long long)cfg->chan[i].Fo) >= (long long)cfg->sdrinrate)
				return VDL2GPU_EINVAL;	/* |Fo| < SDRINRATE / 2 */
	}
#ifndef VDL2GPU_TESTHOOKS
	if (cfg->flags & VDL2GPU_F_TEST_NOREGION)
		return VDL2GPU_EINVAL;	/* test handicaps are compiled into libvdl2gpu_test.so only */
#endif
	if ((cfg->flags & VDL2GPU_F_BLOCK_REPORT) && !(cfg->flags & VDL2GPU_F_FRAMES)) {
		create_err = "vdl2gpu_create: VDL2GPU_F_BLOCK_REPORT needs VDL2GPU_F_FRAMES (the pipeline has no block path to report on)";
		return VDL2GPU_EINVAL;
	}
	if ((cfg->flags & VDL2GPU_F_ALL_FRAMES) && !(cfg->flags & VDL2GPU_F_FRAMES)) {
		create_err = "vdl2gpu_create: VDL2GPU_F_ALL_FRAMES needs VDL2GPU_F_FRAMES (the pipeline has no block path to take frames from)";
		return VDL2GPU_EINVAL;
	}
	if ((cfg->flags & VDL2GPU_F_RAW_FLAGS) && !(cfg->flags & VDL2GPU_F_ALL_FRAMES)) {
		create_err = "vdl2gpu_create: VDL2GPU_F_RAW_FLAGS needs VDL2GPU_F_ALL_FRAMES (it says what a flag is between the frames of a burst)";
		return VDL2GPU_EINVAL;
	}
	const unsigned sdrclk = cfg->sdrclk ? cfg->sdrclk : cfg->sdrinrate / 4000;
	if (sdrclk <= 21 || sdrclk > 1000000)
		return VDL2GPU_EINVAL;
	const unsigned lo_len = (unsigned)vdl2gpu_lo_len(cfg->sdrinrate);
	if (offgrid) {
		/* the table is a whole period of the LO only for offsets on the 25 kHz grid, and a period of the dump schedule
		 * (4 * SDRCLK inputs) must be whole tables: SDRINRATE = 4000 * SDRCLK */
		if ((4ull * sdrclk) % lo_len || k1_win_bytes((sdrclk + 20) / 21) > VDL2_K1_LDS_MAX)
			return VDL2GPU_EINVAL;	/* (above 43.0 MS/s at the default SDRCLK) */
	} else if (k1_smem_bytes(lo_len, (sdrclk + 20) / 21) > VDL2_K1_LDS_MAX)
		return VDL2GPU_EINVAL;	/* the general channeliser's LDS (above 25.7 MS/s at the default SDRCLK) */
	const long long cap = plane_frames(cfg->max_push, sdrclk);
	if (cap == 0 || (unsigned long long)cap * VDL2_CS * sizeof(float2) >= VDL2_PLANES_MAX)
		return VDL2GPU_EINVAL;	/* a stream's planes must stay below 4 GiB (k1_fast's 32-bit offsets) */
	uint64_t test_epoch = 0;
	unsigned test_ticket0 = 0;
#ifdef VDL2GPU_TESTHOOKS
	/* The stream epoch (include/vdl2gpu.h, beside VDL2GPU_F_TEST_NOREGION): only a T0 at which the stream is exactly shift-invariant
	 * -- whole superperiods of the dump schedule (16 SDRCLK inputs, 336 outputs), whole LO tables, whole hand-off blocks of the quirk --
	 * and one whose stamps stay far inside 63 bits.  Refused before any device call. */
	auto env_u64 = [](const char *name, unsigned long long max, unsigned long long *out) {	/* decimal digits only, at most max; unset: *out stays */
		const char *v = getenv(name);
		if (!v)
			return true;
		char *end = nullptr;
		errno = 0;
		const unsigned long long x = strtoull(v, &end, 10);
		if (errno || end == v || *end || *v < '0' || *v > '9' || x > max)
			return false;
		*out = x;
		return true;
	};
	unsigned long long t0 = 0, tk0 = 0;
	if (!env_u64("VDL2GPU_TEST_EPOCH", 1ull << 56, &t0) || !env_u64("VDL2GPU_TEST_TICKET0", 0xffffffffull, &tk0))
		return VDL2GPU_EINVAL;
	if (t0 % (16ull * sdrclk) || t0 % lo_len || ((cfg->flags & VDL2GPU_F_RTL_QUIRK) && t0 % 32768))
		return VDL2GPU_EINVAL;
	test_epoch = t0;
	test_ticket0 = (unsigned)tk0;
#endif
	vdl2gpu_t *h = new(std::nothrow) vdl2gpu;
	if (!h)
		return VDL2GPU_ENOMEM;
	h->cfg = *cfg;
	h->S = cfg->nstreams;
	h->C = cfg->nbch;
	h->L = (int)lo_len;	/* SDRINRATE/STEPRATE, d8psk.c:348; off the 25 kHz grid the LO's true period */
	h->sdrclk = (int)sdrclk;
	h->maxwin = (h->sdrclk + 20) / 21;
	h->k1_glo = offgrid && k1_smem_bytes((uint64_t)h->L, (uint64_t)h->maxwin) > VDL2_K1_LDS_MAX;
	h->sample_bytes = fmt_bytes(cfg->fmt);
	h->rec_cap = cfg->max_bursts ? cfg->max_bursts : 65536u;
	h->chans.assign(cfg->chan, cfg->chan + (size_t)cfg->nstreams * cfg->nbch);
	h->cfg.chan = h->chans.data();
	h->test_epoch = test_epoch;
	h->test_ticket0 = test_ticket0;
	const int rc = create_impl(h);
	if (rc != VDL2GPU_OK) {
		std::string e = h->err;
		if (getenv("VDL2GPU_VERBOSE"))	/* (there is no handle to ask vdl2gpu_last_error() of) */
			fprintf(stderr, "vdl2gpu_create: %s\n", e.c_str());
		vdl2gpu_destroy(h);
		*out = nullptr;
		return rc;
	}
	*out = h;
	return VDL2GPU_OK;
}

/* ------------------------------------------------------------------------ push */
static int get_events(vdl2gpu_t *h, PushTiming &pt)
{
	if (!h->free_ev.empty()) {
		pt = h->free_ev.back();
		h->free_ev.pop_back();
		return VDL2GPU_OK;
	}
	for (auto &e : pt.e)
		NEW_EVENT(h, e, true);
	return VDL2GPU_OK;
}

/* a mark of a push that carries stage events, on stream s; dump_only: one that only VDL2GPU_STAGE_DUMP wants (an event record
 * between two kernels of a chain costs the stream ~3 us) */
static int mark(vdl2gpu_t *h, const PushTiming &pt, StageEv ev, hipStream_t s, bool dump_only = false)
{
	if (pt.staged && (!dump_only || h->stage_dump))
		HIPCHK(h, hipEventRecord(pt.e[ev], s));
	return VDL2GPU_OK;
}

static int harvest_timing(vdl2gpu_t *h)
{
	/* the intervals the stage sums are made of (the demodulator chain starts at the scan, not where the channeliser ended; the
	 * resolver alone, since it may have run beside the next push's channeliser) */
	enum { D_K1, D_SCAN, D_CLUSTER, D_RESOLVE, D_VERIFY /* and the repair rounds */, D_COMMIT /* ... second payload pass, block path */, D_OUT, ND };
	static const struct { StageEv from, to; } stage[ND] = {
		{E_K1_BEGIN, E_K1_END}, {E_SCAN_BEGIN, E_FRONT_END}, {E_CLUSTERS_BEGIN, E_CLUSTERS_END}, {E_RESOLVE_QUEUED, E_RESOLVE_END},
		{E_VERIFY_BEGIN, E_ROUNDS_END}, {E_ROUNDS_END, E_BLOCKS_END}, {E_BLOCKS_END, E_TAIL_END},
	};
	/* VDL2GPU_STAGE_DUMP=1: where every stage of every push began and ended on the GPU's clock, in us since the handle's first
	 * push -- a Gantt chart of the pipeline as it runs WITHOUT a profiler (under rocprofv3 the calling thread is what the streams
	 * wait for), in the pipeline's order (see StageEv.  An event a push does not record keeps the time of the pooled event's last
	 * use: E_PATCH_END on a push that takes the serial path) */
	static const StageEv dump_order[] = {
		E_K1_BEGIN, E_K1_END, E_SCAN_BEGIN, E_FRONT_END, E_CLUSTERS_BEGIN, E_RESOLVE_QUEUED, E_RESOLVE_BEGIN, E_RESOLVE_END, E_VERIFY_BEGIN,
		E_VERIFY_END, E_TAIL_BEGIN, E_PATCH_END, E_ROUNDS_END, E_COMMIT_END, E_PAYLOAD2_END, E_EXPORT_END, E_BLOCKS_END, E_TAIL_END,
	};
	for (auto &pt : h->pending) {
		float d[ND] = {0};
		if (h->stage_dump && pt.staged && h->ev_origin) {
			fprintf(stderr, "vdl2gpu stage dump push %llu:", (unsigned long long)pt.index);
			for (StageEv k : dump_order) {
				float t = -1.0f;
				if (hipEventElapsedTime(&t, h->ev_origin, pt.e[k]) != hipSuccess) {
					(void)hipGetLastError();
					t = -1.0f;
				}
				fprintf(stderr, " e%d=%.1f", (int)k, t * 1e3f);
			}
			fprintf(stderr, "\n");
		}
		if (pt.staged) {	/* only some pushes carry events (each costs the stream ~3 us, and the channeliser now sits on the main
					 * stream): their mean stands for all (see vdl2gpu_get_timing) */
			for (int i = 0; i < ND; ++i)
				HIPCHK(h, hipEventElapsedTime(&d[i], pt.e[stage[i].from], pt.e[stage[i].to]));
			if (pt.fast) {	/* kernel intervals only: first period | fast kernel | tail */
				float a = 0, b = 0, c = 0;
				HIPCHK(h, hipEventElapsedTime(&a, pt.e[E_K1_BEGIN], pt.e[E_K1_HEAD_END]));
				HIPCHK(h, hipEventElapsedTime(&b, pt.e[E_K1_KERNEL_BEGIN], pt.e[E_K1_KERNEL_END]));
				HIPCHK(h, hipEventElapsedTime(&c, pt.e[E_K1_KERNEL_END], pt.e[E_K1_END]));
				d[D_K1] = a + b + c;
			}
			h->st_k1 += d[D_K1];
			h->st_scan += d[D_SCAN] + d[D_VERIFY];
			h->st_cluster += d[D_CLUSTER];
			h->st_resolve += d[D_RESOLVE] + d[D_COMMIT];
			h->st_demod += d[D_SCAN] + d[D_CLUSTER] + d[D_RESOLVE] + d[D_VERIFY] + d[D_COMMIT];
			h->st_other += d[D_OUT];
			h->st_pushes++;
		}
		if (pt.fast && pt.staged) {
			float f = 0;
			HIPCHK(h, hipEventElapsedTime(&f, pt.e[E_K1_KERNEL_BEGIN], pt.e[E_K1_KERNEL_END]));
			h->tm.channelise_fast_ms += f;
			h->tm.fast_pushes++;	/* counts the fast-kernel launches that were timed */
		}
		h->tm.pushes++;
		h->tm.samples += pt.samples;
		h->free_ev.push_back(pt);
	}
	h->pending.clear();
	return VDL2GPU_OK;
}

static int harvest_ring(vdl2gpu_t *h, int ring, bool blocking);
static int enqueue_back(vdl2gpu_t *h);
static void spill_slab(vdl2gpu_t *h, int slab);

/* A scan kernel.  Its workgroups work what passes their first screen off themselves, behind their last tile (k2a_tail); what
 * their private areas of the item list did not hold is left in the list's common area for the one-workgroup-per-channel kernel
 * that follows on the stream -- the scan's ScanDrain says where that is, and goes to that kernel's launch (launch_per_channel). */
enum { SCAN_PROBE, SCAN_REGION, SCAN_VERIFY };
struct ScanDrain { int slot = -1, mode = SURV_CANDS, skip = 0, pch = 0, nwg = 0; };	/* (slot -1: nothing to drain) */
static int launch_scan(vdl2gpu_t *h, int which, const K2Params &k2, dim3 grid, hipStream_t st, int slot, int mode, int skip, unsigned tiles_per_wg, ScanDrain &drain)
{
	K2Params q = k2;
	/* a scan workgroup's private part of the item list: one and a half times what its tiles yield at the first screen's 2.7 %
	 * (28 per tile and class; the region scan's tiles are sync words: far more pass) plus a sync word's worth; what it does
	 * not hold goes to the common area */
	const unsigned item_priv = k2.item_priv;
	grid.x = std::min<unsigned>(grid.x, VDL2_MAXWG);
	/* every scan walks its work with any grid (the verify pass too, since round 10: its workgroups share the part's pieces out among
	 * however many they are), so one bound holds for all three: a private area of 256 items at least for every workgroup */
	grid.x = std::max(1u, std::min<unsigned>(grid.x, item_priv / 256u));
	unsigned want = (tiles_per_wg * (which == SCAN_REGION ? 400u : 42u * (K2A_TS / 1024u)) + 128u + 255u) / 256u * 256u;	/* (42 of a 1024-instant tile pass: 2.7 % x 1.5) */
	q.surv_common_cap = 0;	/* (0: whatever the list has left behind the private areas) */
#ifdef VDL2GPU_TESTHOOKS
	const bool test_items = !h->knob.test_item_verify || which == SCAN_VERIFY;
	if (test_items && h->knob.test_item_grid > 0) {
		grid.x = std::min<unsigned>(grid.x, (unsigned)h->knob.test_item_grid);
		want = 256u;
	}
	if (test_items && h->knob.test_item_common > 0)
		q.surv_common_cap = h->knob.test_item_common;
#endif
	q.surv_nwg = (int)grid.x;
	q.surv_pch = (int)std::max(256u, std::min(want, item_priv / grid.x / 256u * 256u));
	/* The grid is final.  The private areas lie in front of the list's common area: the kernels take `item_cap - surv_nwg * surv_pch`
	 * for the common area's size, unsigned.  The clamps above guarantee it (grid.x <= item_priv / 256, so item_priv / grid.x / 256 * 256
	 * is at least 256 and at most item_priv / grid.x), and create_impl makes the common area non-empty; said here so that a change
	 * to either fails the push instead of wrapping in a kernel. */
	if ((unsigned)q.surv_nwg * (unsigned)q.surv_pch > item_priv || item_priv >= k2.item_cap) {
		h->err = "launch_scan: the scan's private areas (" + std::to_string(q.surv_nwg) + " x " + std::to_string(q.surv_pch) +
			 " items) do not fit the item list (" + std::to_string(item_priv) + " private of " + std::to_string(k2.item_cap) + ")";
		return VDL2GPU_EINVAL;
	}
	q.surv_slot = slot;
	q.surv_mode = mode;
	q.surv_skip = skip;
	q.drain_slot = -1;
	switch (which) {
	case SCAN_PROBE: hipLaunchKernelGGL(k2a_probe, grid, dim3(K2A_THREADS), 0, st, q); break;
	case SCAN_REGION: hipLaunchKernelGGL(k2a_region, grid, dim3(K2A_THREADS), 0, st, q); break;
	default: hipLaunchKernelGGL(k2a_verify, grid, dim3(K2A_THREADS), 0, st, q); break;
	}
	drain = ScanDrain{ slot, mode, skip, q.surv_pch, q.surv_nwg };
	return VDL2GPU_OK;
}

/* A one-workgroup-per-channel kernel (k2r_regions, k2s_sort, k2s_merge, k2p_patch, k2c_resolve, k2f_commit) of `nt` threads on
 * stream s, which first works off the common area of the scan in front of it, if there is one.  Nothing else writes
 * K2Params.drain_*: a launch without a drain gets none. */
template <class... A>
static void launch_per_channel(const vdl2gpu_t *h, void (*kernel)(K2Params, A...), unsigned nt, hipStream_t s, const K2Params &k2, const ScanDrain &drain = ScanDrain(),
			       A... more)	/* (k2f_commit_fb: the feedback rows) */
{
	K2Params q = k2;
	q.drain_slot = drain.slot;
	q.drain_mode = drain.mode;
	q.drain_skip = drain.skip;
	q.drain_pch = drain.pch;
	q.drain_nwg = drain.nwg;
	hipLaunchKernelGGL(kernel, dim3((unsigned)h->C, (unsigned)h->S), dim3(nt), 0, s, q, more...);
}

/* the cluster kernel: a persistent grid */
static void launch_clusters(const vdl2gpu_t *h, hipStream_t s, const K2Params &k2)
{
	hipLaunchKernelGGL(k2b_clusters, dim3((unsigned)(h->n_cu * 4 * K2B_GRIDW), (unsigned)((h->S * VDL2_CS + 63) / 64)), dim3(K2B_NT), 0, s, k2);
}

/* The payload kernel of the handle's flags (each optional pass is a kernel variant of its own: register pressure) on the
 * selection `sel_mode` names (K2Params.sel_mode).  ring: the output ring k2.recs lies in; with VDL2GPU_F_FEEDBACK its feedback rows are
 * the kernel's second argument (they are no member of K2Params: vdl2gpu_resolve.h, k2d_run).  The two tables -- the eight kernels
 * without the feedback pass, the eight with it -- are filled from K2D_PAYLOAD_KERNELS, each kernel where K2D_INDEX of its own line's
 * flags says, and asked with K2D_INDEX of the handle's: no order to keep in step by hand. */
struct PayloadKernels {
	void (*fb0[8])(K2Params);
	void (*fb1[8])(K2Params, vdl2gpu_fb_t *);
	PayloadKernels()
	{
#define K2D_ENTER(name, waves, LEV, SOFT, CAR, FB) fb##FB[K2D_INDEX(LEV, SOFT, CAR, 0)] = name;
		K2D_PAYLOAD_KERNELS(K2D_ENTER)
#undef K2D_ENTER
	}
};
static void launch_payload(const vdl2gpu_t *h, hipStream_t s, const K2Params &k2, int sel_mode, int ring)
{
	static const PayloadKernels kernels;
	const int which = K2D_INDEX(h->col_on[COL_LEVEL] ? 1 : 0, h->col_on[COL_SOFT] ? 1 : 0, h->col_on[COL_CARRIER] ? 1 : 0, 0);
	K2Params q = k2;
	q.sel_mode = sel_mode;
	const dim3 grid((unsigned)h->k2d_grid, (unsigned)(VDL2_CS * h->S));
	if (h->col_on[COL_FB])
		hipLaunchKernelGGL(kernels.fb1[which], grid, dim3(K2D_NT), 0, s, q, h->ring[ring].col<vdl2gpu_fb_t>(COL_FB));
	else
		hipLaunchKernelGGL(kernels.fb0[which], grid, dim3(K2D_NT), 0, s, q);
}

/* tiles' worth of items a verify workgroup's private area is sized for: its share q of the pieces (k2a_verify) when a launch of
 * nwg workgroups per channel scans all of a part -- the pieces' instants are the part's at most, and a stretch's partial last piece
 * rounds a share up by one */
static unsigned verify_share(unsigned pieces, unsigned nwg)
{
	nwg = std::max(1u, std::min<unsigned>(nwg, VDL2_MAXWG));
	return (pieces + nwg - 1) / nwg + 1;
}

/* A sample format as a kernel instantiation: f is called with std::integral_constant<int, FMT> of the handle's format, and launches
 * kernel<decltype(F)::value>.  (What else knows the formats: fmt_bytes, and the full scale of a level record in create_impl.) */
template <class F> static void with_fmt(int fmt, F &&f)
{
	switch (fmt) {
	case VDL2GPU_FMT_CU8: f(std::integral_constant<int, VDL2GPU_FMT_CU8>{}); break;
	case VDL2GPU_FMT_CS16: f(std::integral_constant<int, VDL2GPU_FMT_CS16>{}); break;
	case VDL2GPU_FMT_CF32: f(std::integral_constant<int, VDL2GPU_FMT_CF32>{}); break;
	case VDL2GPU_FMT_CS8: f(std::integral_constant<int, VDL2GPU_FMT_CS8>{}); break;
	case VDL2GPU_FMT_S16R: f(std::integral_constant<int, VDL2GPU_FMT_S16R>{}); break;
	default: f(std::integral_constant<int, VDL2GPU_FMT_F32R>{}); break;
	}
}

/* A channeliser kernel of the handle: `plain`, or with VDL2GPU_F_EXACT_FO `rot`, which takes the rotation behind the parameters. */
template <class P> static void launch_k1(const vdl2gpu_t *h, void (*plain)(P), void (*rot)(P, K1Rot), dim3 grid, unsigned threads, size_t smem,
					 hipStream_t ks, const P &p)
{
	if (h->rot)
		hipLaunchKernelGGL(rot, grid, dim3(threads), smem, ks, p, h->k1rot);
	else
		hipLaunchKernelGGL(plain, grid, dim3(threads), smem, ks, p);
}

static int push_impl(vdl2gpu_t *h, const void *iq, size_t nsamples, size_t stream_stride_bytes, int memkind, bool wait_copy);

static int push_checked(vdl2gpu_t *h, const void *iq, size_t nsamples, size_t stream_stride_bytes, int memkind, bool wait_copy)
{
	if (h && h->failed) {
		h->err = "an earlier HIP error left the handle unusable: " + h->err;
		return VDL2GPU_EHIP;
	}
	/* A push carries at most ~36 s of air time through the tables, and less on busy channels: the tables hold 6144 trigger
	 * candidates per channel, and a channel that overflows them is handled by the serial machine for the whole part
	 * (exact, ~15 ms for 34 s of 8 channels).  Longer pushes are cut into equal parts whose length follows the candidate
	 * density of the pushes collected lately (harvest_ring) -- multiples of a k1_fast superperiod (8000 samples at
	 * 2 MS/s: the parts then need no general channeliser launch at their edges) or of the reference's 32768-sample block
	 * (other rates; VDL2GPU_F_RTL_QUIRK needs whole blocks anyway); any cut gives the same bursts. */
	int rc = VDL2GPU_OK;
	const size_t lim = h ? h->split_samples : 0;
	auto passes = [&](const void *q, size_t n) -> int { return push_impl(h, q, n, stream_stride_bytes, memkind, wait_copy); };
	if (!h || !iq || lim == 0 || nsamples <= lim)
		rc = passes(iq, nsamples);
	else {
		if (nsamples > h->cfg.max_push)
			return VDL2GPU_EINVAL;
		const size_t parts = (nsamples + lim - 1) / lim;
		const size_t unit = h->split_unit;
		const size_t part = ((nsamples + parts - 1) / parts + unit - 1) / unit * unit;
		for (size_t off = 0; off < nsamples && rc == VDL2GPU_OK; off += part)
			rc = passes((const char *)iq + off * h->sample_bytes, std::min(part, nsamples - off));
	}
	if (rc == VDL2GPU_EHIP)
		h->failed = true;	/* part of the push may be enqueued: nothing after it can be trusted */
	return rc;
}

extern "C" int vdl2gpu_push(vdl2gpu_t *h, const void *iq, size_t nsamples, size_t stream_stride_bytes, int memkind)
{
	if (!h)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	/* the caller may reuse a host buffer as soon as we return (the reference's producer refills Cbuff
	 * right after the consumers pass Bar1, d8psk.c:383): wait for the copy, not for the kernels */
	return push_checked(h, iq, nsamples, stream_stride_bytes, memkind, true);
}

/* ---------------------------------------------------------------- ingest ring */
extern "C" int vdl2gpu_ring_init(vdl2gpu_t *h, size_t slot_samples, int nslots)
{
	if (!h || slot_samples == 0 || slot_samples > h->cfg.max_push || nslots < 2 || nslots > 64)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	if (h->ring_host) {
		h->err = "vdl2gpu_ring_init: the ring exists already";
		return VDL2GPU_EINVAL;
	}
	HIPCHK(h, hipSetDevice(h->cfg.device));
	h->ring_slot_samples = slot_samples;
	h->ring_slot_bytes = slot_samples * h->sample_bytes * (size_t)h->S;
	HOST_ALLOC(h, h->ring_host, h->ring_slot_bytes * (size_t)nslots, hipHostMallocDefault);
	h->ring_nslots = nslots;
	h->ring_copied.resize((size_t)nslots);
	for (LaterEvent &e : h->ring_copied)
		NEW_EVENT(h, e.ev);
	return VDL2GPU_OK;
}

extern "C" void *vdl2gpu_ring_acquire(vdl2gpu_t *h, size_t *stream_stride_bytes)
{
	if (!h)
		return nullptr;
	HLOCK(h);
	if (!h->ring_host || h->ring_acquired)
		return nullptr;
	const size_t slot = (size_t)(h->ring_next % (unsigned long long)h->ring_nslots);
	if (h->ring_copied[slot].recorded) {	/* its copy to the GPU must have left the slot */
		if (hipSetDevice(h->cfg.device) != hipSuccess || h->ring_copied[slot].sync(h)) {
			h->err = "vdl2gpu_ring_acquire: waiting for the slot failed";
			return nullptr;
		}
		h->ring_copied[slot].clear();
	}
	if (stream_stride_bytes)
		*stream_stride_bytes = h->ring_slot_samples * h->sample_bytes;
	h->ring_acquired = true;
	return (char *)h->ring_host + slot * h->ring_slot_bytes;
}

extern "C" int vdl2gpu_ring_commit(vdl2gpu_t *h, size_t nsamples)
{
	if (!h)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	if (!h->ring_host || !h->ring_acquired || nsamples > h->ring_slot_samples)
		return VDL2GPU_EINVAL;
	const size_t slot = (size_t)(h->ring_next % (unsigned long long)h->ring_nslots);
	h->ring_acquired = false;
	h->ring_next++;
	if (nsamples == 0)
		return VDL2GPU_OK;	/* e.g. a short USB read: the block is dropped (rtl.c:278-281) */
	const int rc = push_checked(h, (char *)h->ring_host + slot * h->ring_slot_bytes, nsamples,
				    h->ring_slot_samples * h->sample_bytes, VDL2GPU_MEM_HOST, false);
	if (h->in_stream) {	/* whatever was enqueued from the slot, its end is marked: acquire() waits for it */
		const std::string push_err = h->err;
		if (h->ring_copied[slot].record(h, h->in_stream)) {
			if (rc == VDL2GPU_OK) {
				h->failed = true;
				return VDL2GPU_EHIP;
			}
			h->err = push_err;	/* (the push's own error is the one to report) */
		}
	}
	return rc;
}

/* k4_frames on the records of output ring `ring` where they lie: compact entries, the record count from the device.  fmask: not
 * nullptr when K2d's second pass tags void records (see K4Params) */
/* The block kernel on `grid` workgroups of stream s: with a report or without (rep), with the records' decision-feedback rows in the
 * row rule (k4.fb is given) or without; mode (VDL2GPU_BLK_*): 0, every segment between flags is a candidate frame (ALL_FRAMES), or that
 * with a flag being six adjacent ones of the stuffed stream (ALL_FRAMES | RAW_FLAGS); with the records' timing-tracked rows
 * (k4.trk is given), each of these with the second attempt of vdl2gpu_trk_t */
static void launch_blocks(hipStream_t s, unsigned grid, const K4Params &k4, bool rep, uint32_t mode)
{
	void (*const kernel)(K4Params) =
		k4.trk ? k4_frames_trk_kernel(rep, k4.fb != nullptr, mode)	/* the records' timing-tracked rows are given: the kernels with the second attempt */
		: mode & VDL2GPU_BLK_RAW_FLAGS ? (k4.fb ? (rep ? k4_frames_raw_rep_fb : k4_frames_raw_fb) : (rep ? k4_frames_raw_rep : k4_frames_raw))
		: mode & VDL2GPU_BLK_ALL_FRAMES ? (k4.fb ? (rep ? k4_frames_all_rep_fb : k4_frames_all_fb) : (rep ? k4_frames_all_rep : k4_frames_all))
						: (k4.fb ? (rep ? k4_frames_rep_fb : k4_frames_fb) : (rep ? k4_frames_rep : k4_frames));
	hipLaunchKernelGGL(kernel, dim3(grid), dim3(K4_NT), 0, s, k4);
}

static K4Params k4_ring_params(vdl2gpu_t *h, int ring, const unsigned *fmask)
{
	K4Params k4{};
	k4.recs = h->ring[ring].d_recs;
	k4.nrecs_dev = &h->d_outc->ring[ring].records;
	k4.rec_cap = h->rec_cap;
	k4.frames = h->ring[ring].d_frames;
	k4.nframes = h->d_fcnt + ring;
	k4.frame_cap = h->frame_cap;
	k4.compact = 1;
	k4.tabs = h->d_k4tab;
	k4.fmask = fmask;
	k4.soft = h->ring[ring].col<vdl2gpu_soft_t>(COL_SOFT);	/* (nullptr without VDL2GPU_F_SOFT_RS: the reference's block path) */
	k4.rep = h->ring[ring].col<vdl2gpu_blockrep_t>(COL_REPORT);	/* (nullptr without VDL2GPU_F_BLOCK_REPORT, and k4_frames is launched, which does not look at it) */
	k4.fb = h->ring[ring].col<vdl2gpu_fb_t>(COL_FB);	/* (nullptr without VDL2GPU_F_FEEDBACK: launch_blocks) */
	k4.trk = h->ring[ring].col<vdl2gpu_trk_t>(COL_TRK);	/* (nullptr without VDL2GPU_F_TRACKED: launch_blocks) */
	return k4;
}

/* The BACK stage of a push (see vdl2gpu::Back): resolver, payload decode beside the verify pass, repair rounds, commit,
 * block path, counters -- on the main stream, behind the previous push's back stage and behind this push's front. */
static int enqueue_back(vdl2gpu_t *h)
{
	if (!h->back.valid)
		return VDL2GPU_OK;
	h->back.valid = false;
	const K2Params &k2 = h->back.k2;
	const int64_t J = h->back.J;
	const int par = h->back.par, ring = h->back.ring;
	const bool serial = h->back.serial, spec = h->back.spec;
	const unsigned tiles = h->back.tiles;
	const int GS = h->S;
	const PushTiming &pt = h->pending[h->back.pt_index];
	hipStream_t rs = h->stream;
	if (h->back.two_streams)
		HIPCHK(h, hipStreamWaitEvent(rs, h->set[par].f_done, 0));
	/* the cluster kernel needs nothing of the previous push's result either, but it is wide, and the stages are better
	 * balanced with it here: FRONT = channeliser + scan, BACK = clusters + resolver + verify */
	TRY(mark(h, pt, E_CLUSTERS_BEGIN, rs));
	if (!serial)
		launch_clusters(h, rs, k2);
	HIPCHK(h, hipGetLastError());
	TRY(mark(h, pt, E_CLUSTERS_END, rs));
	TRY(mark(h, pt, E_RESOLVE_QUEUED, rs));
	/* The verify pass's pieces (k2a_verify): a part's stretches are disjoint, so at most a piece per tile of 2 * K2A_TS samples and one
	 * more per stretch.  The first pass's grid is ONE RESIDENT ROUND -- six workgroups a CU, shared out over the (channel, stream)
	 * slots, about seven pieces each at 8 channels and 67 MS -- and no longer the map of the part (a workgroup per K2A_VRUN tiles: 2 800
	 * workgroups for 1 536 places; -DK2A_VGRID_RESIDENT=0 is that grid, DESIGN.md section 5 has both). */
	const unsigned vpieces = tiles / 2 + 1;
#if K2A_VGRID_RESIDENT
	const unsigned vwg0 = std::min(vpieces, std::max(1u, (unsigned)h->n_cu * 6u / (unsigned)(h->C * GS)));
#else
	const unsigned vwg0 = (vpieces + K2A_VRUN - 1) / K2A_VRUN;
#endif
	const dim3 vgrid0(vwg0, (unsigned)h->C, (unsigned)GS);
	ScanDrain vdrain;	/* the verify pass whose common area the next one-workgroup-per-channel kernel of the tail has to drain */
	TRY(h->k2f_done.wait(h, rs));	/* the channel states the resolver starts from are committed on the previous push's tail */
	TRY(mark(h, pt, E_RESOLVE_BEGIN, rs, true));
	launch_per_channel(h, k2c_resolve, K2_NT, rs, k2);
	HIPCHK(h, hipGetLastError());
	TRY(mark(h, pt, E_RESOLVE_END, rs));
	/* The resolver's selection is final unless the verify pass fails -- then a repair round re-resolves the
	 * channel, or K2f redoes it serially, and the host drops what K2d made of it (see harvest_ring; K2d decodes
	 * a repaired selection in a second pass behind the rounds): decode the payloads beside the verify pass
	 * instead of behind it (`spec`, decided in push_impl). */
	h->ring[ring].spec = spec;
	if (spec)
		HIPCHK(h, hipEventRecord(h->k2c_done, rs));
	/* The payload decode beside the verify pass: on the copy stream (a hardware queue of its own), so that the push's TAIL on the
	 * payload stream -- the repair round and the commit, which the NEXT push's resolver waits for: the pipeline's loop-carried
	 * dependency -- starts when the verify pass ends, not when this latency-bound kernel has found CUs between the verify pass's
	 * workgroups and finished.  The repair rounds write a selection of their own (K2Params.sel_list2), so nothing the decode
	 * reads changes under it; the tail waits for it only where it needs its records: in front of the second payload pass and the
	 * export. */
	hipStream_t ps = h->copy_stream;	/* (four hardware queues: the copy stream has one job) */
	if (spec) {
		HIPCHK(h, hipStreamWaitEvent(ps, h->k2c_done, 0));
		launch_payload(h, ps, k2, SEL_FIRST, ring);
		HIPCHK(h, hipEventRecord(h->pay_done, ps));
	}
	TRY(mark(h, pt, E_VERIFY_BEGIN, rs));
	if (!serial)
		TRY(launch_scan(h, SCAN_VERIFY, k2, vgrid0, rs, VDL2_SURV_VERIFY, SURV_VERIFY, 0, verify_share(vpieces, vgrid0.x), vdrain));
	HIPCHK(h, hipGetLastError());
	TRY(mark(h, pt, E_VERIFY_END, rs, true));
	/* ---- the TAIL: everything behind the verify pass -- repair rounds, commit, the payloads a round re-resolved, block path,
	 * export, counters: a chain of one-workgroup-per-channel kernels and a PCIe copy, 0.1 ms while nothing fails and 0.3 ms when
	 * a channel is repaired (most pushes of ordinary traffic).  On the main stream it stood between this push's verify pass and
	 * the NEXT push's cluster kernel, which needs none of it; it runs on the payload stream instead (behind the payload decode
	 * it would have had to wait for anyway), the main stream goes on with the next push, and only that push's resolver waits --
	 * for the commit (k2f_done), which the cluster kernel in front of it covers.  k2_done, which frees the plane and table sets
	 * and tells the host the ring is complete, is recorded at the tail's end. */
	hipStream_t ts = (spec && h->back.two_streams && !h->knob.no_tail) ? h->pay_stream : rs;
	if (ts != rs) {
		HIPCHK(h, hipEventRecord(h->verify_done, rs));
		HIPCHK(h, hipStreamWaitEvent(ts, h->verify_done, 0));
	}
	if (h->tail_prev && h->tail_prev != ts)	/* tails follow each other (running totals, StreamState) */
		TRY(h->set[set_before(par)].k2_done.wait(h, ts));
	h->tail_prev = ts;
	TRY(mark(h, pt, E_TAIL_BEGIN, ts, true));
	if (!h->full_scan && !serial) {
		/* Repair rounds.  The verify pass has appended what it found to the failing channel's table (candidates without
		 * clusters): a round re-sorts the table, re-resolves the channel -- the resolver replays the new candidates with the
		 * serial machine and returns to the tables behind each -- and verifies the stretches the new chain idles through
		 * (other classes than before from the first new event on).  Every other channel's workgroups exit at once: three
		 * launches, ~12 us, when nothing failed -- which is why one round is ALWAYS scheduled: an unlisted event (a noise
		 * trigger that exists in one class only) turns up about once per 100 channel-seconds of ordinary traffic, and without
		 * a round it costs a serial redo of the channel's whole push (K2f: 8 ms at 33 s of air time).  If more than one round
		 * is scheduled (after a serial redo: adapted below), the LAST one does not repair, it starts over: the channels that
		 * still fail are scanned completely -- every class at every instant, like VDL2GPU_F_FULLSCAN but for them alone
		 * (~0.1 ms for a channel of a 67 MS push) -- their tables rebuilt from nothing, which leaves nothing to verify and
		 * nothing to cascade.  What still fails after the last round is redone serially by K2f. */
		K2Params k2r = k2;	/* (what a round's launches share: round, full_round, mini_round) */
		/* (a repair round writes its own selection, sel_list2: the payload decode of the first one goes on beside it -- unless the
		 * last round is a complete one: that re-makes the failing channels' clusters, whose descriptors the decode may be reading) */
		if (spec && h->repair_rounds >= 2 && ts != ps)
			HIPCHK(h, hipStreamWaitEvent(ts, h->pay_done, 0));
		for (int rr = 1; rr <= h->repair_rounds; ++rr) {
			k2r.round = rr;
			k2r.full_round = (rr == h->repair_rounds && h->repair_rounds >= 2) ? 1 : 0;
			k2r.mini_round = k2r.full_round ? 0 : 1;
			if (k2r.full_round) {
				launch_per_channel(h, k2r_regions, K2R_NT, ts, k2r, vdrain);	/* (resets the channel's tables) */
				const unsigned want = tiles;
				unsigned per = (unsigned)h->n_cu;	/* few channels fail: each may use the whole GPU (the others' workgroups leave at once) */
				per = per > want ? want : per;
				ScanDrain pdrain;
				TRY(launch_scan(h, SCAN_PROBE, k2r, dim3(per, (unsigned)h->C, (unsigned)GS), ts, VDL2_SURV_FULL, SURV_CANDS, 0, 4 * ((want + per - 1) / per), pdrain));
				launch_per_channel(h, k2s_sort, K2S_NT, ts, k2r, pdrain);
				launch_clusters(h, ts, k2r);
				launch_per_channel(h, k2c_resolve, K2_NT, ts, k2r);
				vdrain = ScanDrain();	/* (nothing is verified behind a complete round) */
			} else if (rr == 1) {
				/* the first round repairs locally: from each event the verify pass listed to where the new chain rejoins the old one
				 * (k2p_patch: one narrow kernel, tables read where they lie), and the verify pass looks at what changed */
				launch_per_channel(h, k2p_patch, K2P_NT, ts, k2r, vdrain);
				TRY(mark(h, pt, E_PATCH_END, ts, true));
				/* a handful of workgroups per channel, which share the pieces of the stretches a local repair changed out among
				 * themselves (k2a_verify: a few tiles as a rule, a piece or two each; at most the part): every workgroup of a launch
				 * has to wait for a slot beside the other pushes' wide kernels before it can leave */
				const unsigned nv = std::min<unsigned>(vpieces, (unsigned)h->knob.verify2_wg);
				TRY(launch_scan(h, SCAN_VERIFY, k2r, dim3(nv, vgrid0.y, vgrid0.z), ts, VDL2_SURV_VERIFY + rr, SURV_VERIFY, 0, verify_share(vpieces, nv), vdrain));
			} else {
				/* a further round resolves the channels that still fail again from their input state, with everything listed so far */
				launch_per_channel(h, k2s_merge, K2M_NT, ts, k2r, vdrain);
				launch_per_channel(h, k2c_resolve, K2_NT, ts, k2r);
				TRY(launch_scan(h, SCAN_VERIFY, k2r, vgrid0, ts, VDL2_SURV_VERIFY + rr, SURV_VERIFY, 0, verify_share(vpieces, vgrid0.x), vdrain));
			}
		}
		HIPCHK(h, hipGetLastError());
	}
	TRY(mark(h, pt, E_ROUNDS_END, ts));
	if (h->col_on[COL_FB])
		launch_per_channel(h, k2f_commit_fb, K2_NT, ts, k2, vdrain, h->ring[ring].col<vdl2gpu_fb_t>(COL_FB));
	else
		launch_per_channel(h, k2f_commit, K2_NT, ts, k2, vdrain);

	TRY(h->k2f_done.record(h, ts));
	TRY(mark(h, pt, E_COMMIT_END, ts, true));
	if (spec) {
		if (ts != ps)
			HIPCHK(h, hipStreamWaitEvent(ts, h->pay_done, 0));	/* the export needs the first pass's records, K3 publishes the record count */
		if (!h->full_scan && !serial)	/* what the repair rounds (or K2f's serial redo) made void of the first selection is tagged now, what they selected is decoded */
			launch_payload(h, ts, k2, SEL_REPAIRED, ring);
	} else
		launch_payload(h, ts, k2, SEL_FINAL, ring);	/* one pass behind the commit: the repaired selection where there is one */
	HIPCHK(h, hipGetLastError());
	TRY(mark(h, pt, E_PAYLOAD2_END, ts, true));
	if (h->col_on[COL_TRK]) {
		/* VDL2GPU_F_TRACKED: the timing-tracked rows of every record of the push's ring, behind the last payload pass -- the records are
		 * final -- and in front of the block path, which reads them; on the tail's stream, where the set is the push's own until k2_done
		 * below.  Record-driven, like k_symclk_sums: whichever kernel, pass or round made a record, this is the one place that slices it. */
		KTrackedParams kt{};
		kt.dec = k2.dec;
		kt.cap = (int)k2.cap;
		kt.dec_base = k2.dec_base;
		kt.frames = (int)std::min<long long>(VDL2_CARRY_FRAMES + J, k2.cap);
		kt.cfg = h->d_cfg;
		kt.nbch = h->C;
		kt.nstreams = h->S;
		kt.recs = h->ring[ring].d_recs;
		kt.count = &h->d_outc->ring[ring].records;
		kt.rec_cap = h->rec_cap;
		kt.out = h->ring[ring].col<vdl2gpu_trk_t>(COL_TRK);
		kt.pn8 = k2.pn8;
		hipLaunchKernelGGL(k_tracked_rows, dim3(std::min(h->rec_cap, 4u * (unsigned)h->n_cu)), dim3(KTR_NT), 0, ts, kt);
		HIPCHK(h, hipGetLastError());
	}
	if (h->frames_on) {
		/* block path on the records where they lie (vdlm2.c:84-161).  In the chain, not beside it:
		 * a latency-bound kernel like this one and the next push's scan slow each other down by
		 * more than the overlap saves. */
		launch_blocks(ts, (unsigned)h->n_cu * 16, k4_ring_params(h, ring, spec ? h->set[par].k2.fmask : nullptr), h->col_on[COL_REPORT],
			      (h->cfg.flags & VDL2GPU_F_ALL_FRAMES ? VDL2GPU_BLK_ALL_FRAMES : 0u) | (h->cfg.flags & VDL2GPU_F_RAW_FLAGS ? VDL2GPU_BLK_RAW_FLAGS : 0u));
		HIPCHK(h, hipGetLastError());
	}
	TRY(mark(h, pt, E_BLOCKS_END, ts));
	if (h->col_on[COL_SYMCLK]) {
		/* VDL2GPU_F_SYMCLK: the timing sums of every record of the push's ring, behind the last payload pass -- the records are final --
		 * and on the tail's stream, where the second payload pass has just read the same planes: the set is the push's own until
		 * k2_done below.  Record-driven: whichever kernel, pass or round made a record, this is the one place that measures it. */
		KSymclkParams kc{};
		kc.dec = k2.dec;
		kc.cap = k2.cap;
		kc.dec_base = k2.dec_base;
		kc.frames = std::min<long long>(VDL2_CARRY_FRAMES + J, k2.cap);
		kc.cfg = h->d_cfg;
		kc.nbch = h->C;
		kc.nstreams = h->S;
		kc.recs = h->ring[ring].d_recs;
		kc.count = &h->d_outc->ring[ring].records;
		kc.rec_cap = h->rec_cap;
		kc.out = h->ring[ring].col<vdl2gpu_symclk_t>(COL_SYMCLK);
		symclk_taps(kc.taps);
		hipLaunchKernelGGL(k_symclk_sums, dim3(VDL2GPU_SYMCLK_SEGS, std::min(h->rec_cap, 2u * (unsigned)h->n_cu)), dim3(KSC_NT), 0, ts, kc);
		HIPCHK(h, hipGetLastError());
	}
	{
		/* the push's records go to the host by the GPU's own hand: page-locked memory, coalesced 8-byte stores */
		KExportParams ke{};
		ke.recs = h->ring[ring].d_recs;
		ke.count = &h->d_outc->ring[ring].records;
		ke.dst = h->slab[h->back.slab].d_recs;
		ke.cap = std::min(h->slab_cap, h->rec_cap);
		const OutRing &rg = h->ring[ring];
		const Slab &sl = h->slab[h->back.slab];
		ke.lev = rg.col<vdl2gpu_level_t>(COL_LEVEL);	/* (nullptr without VDL2GPU_F_LEVELS) */
		ke.ldst = sl.col<vdl2gpu_level_t>(COL_LEVEL);
		ke.soft = rg.col<vdl2gpu_soft_t>(COL_SOFT);	/* (nullptr without VDL2GPU_F_SOFT_RS) */
		ke.sdst = sl.col<vdl2gpu_soft_t>(COL_SOFT);
		ke.car = rg.col<vdl2gpu_carrier_t>(COL_CARRIER);	/* (nullptr without VDL2GPU_F_CARRIER) */
		ke.cdst = sl.col<vdl2gpu_carrier_t>(COL_CARRIER);
		ke.rep = rg.col<vdl2gpu_blockrep_t>(COL_REPORT);	/* (nullptr without VDL2GPU_F_BLOCK_REPORT) */
		ke.rdst = sl.col<vdl2gpu_blockrep_t>(COL_REPORT);
		hipLaunchKernelGGL(k_export_records, dim3((unsigned)h->n_cu), dim3(256), 0, ts, ke);
		HIPCHK(h, hipGetLastError());
		if (h->col_on[COL_FB]) {	/* the feedback rows beside them: a kernel of its own, k_export_records keeps its registers */
			hipLaunchKernelGGL(k_export_feedback, dim3((unsigned)h->n_cu), dim3(256), 0, ts, ke.count, ke.cap,
					   rg.col<const vdl2gpu_fb_t>(COL_FB), sl.col<vdl2gpu_fb_t>(COL_FB));
			HIPCHK(h, hipGetLastError());
		}
		if (h->col_on[COL_TRK]) {	/* ... and the timing-tracked rows */
			hipLaunchKernelGGL(k_export_tracked, dim3((unsigned)h->n_cu), dim3(256), 0, ts, ke.count, ke.cap,
					   rg.col<const vdl2gpu_trk_t>(COL_TRK), sl.col<vdl2gpu_trk_t>(COL_TRK));
			HIPCHK(h, hipGetLastError());
		}
		if (h->col_on[COL_SYMCLK]) {	/* ... and the symbol-clock records, likewise */
			hipLaunchKernelGGL(k_export_symclk, dim3((unsigned)h->n_cu), dim3(256), 0, ts, ke.count, ke.cap,
					   rg.col<const vdl2gpu_symclk_t>(COL_SYMCLK), sl.col<vdl2gpu_symclk_t>(COL_SYMCLK));
			HIPCHK(h, hipGetLastError());
		}
		TRY(mark(h, pt, E_EXPORT_END, ts, true));
		K3Params k3{};
		k3.src = nullptr;	/* (the counters kernel copies nothing) */
		k3.dst = nullptr;
		k3.cap = h->cap;
		k3.nbch = h->C;
		k3.J = J;
		k3.ss = h->d_ss;
		k3.cs = h->d_cs;
		k3.outc = h->d_outc;
		k3.fmask = h->set[par].k2.fmask;
		k3.fcnt = h->frames_on ? h->d_fcnt + ring : nullptr;
		k3.host_cnt = h->d_pin_cnt + ring;
		k3.ring = ring;
		k3.ctl = h->set[par].k2.ctl;
		k3.nstreams = h->S;
		hipLaunchKernelGGL(k3_rebase, dim3((unsigned)GS), dim3(64), 0, ts, k3);
		HIPCHK(h, hipGetLastError());
	}
	TRY(mark(h, pt, E_TAIL_END, ts));
	TRY(h->set[par].k2_done.record(h, ts));
	h->ring[ring].ev ^= 1;
	HIPCHK(h, hipEventRecord(h->ring[ring].done(), ts));
	return VDL2GPU_OK;
}

/* ---- the stages of a push, in the order push_impl runs them ---- */

/* Where the channeliser reads a push's samples: the caller's device buffer as it is, or -- host samples -- one of the two
 * staging buffers in HBM, filled on a stream of their own. */
struct Input {
	const void *src;
	size_t stride;
	bool staged;
};

static int stage_input(vdl2gpu_t *h, const void *iq, size_t nsamples, size_t stream_stride_bytes, int memkind, bool wait_copy, int stg, Input &in)
{
	in = Input{ iq, stream_stride_bytes, false };
	if (memkind == VDL2GPU_MEM_DEVICE)
		return VDL2GPU_OK;
	if (memkind != VDL2GPU_MEM_HOST)
		return VDL2GPU_EINVAL;
	const size_t per = nsamples * h->sample_bytes;
	const size_t need = per * (size_t)h->S;
	if (!h->in_stream) {
		NEW_STREAM(h, h->in_stream);
		for (int i = 0; i < 2; ++i)
			NEW_EVENT(h, h->raw_copied[i]);
	}
	if (need > h->raw_bytes[stg]) {
		HIPCHK(h, hipStreamSynchronize(h->fstream));
		HIPCHK(h, hipStreamSynchronize(h->stream));
		HIPCHK(h, hipStreamSynchronize(h->pay_stream));
		HIPCHK(h, hipStreamSynchronize(h->in_stream));
		dev_release(h, h->d_raw[stg]);
		h->d_raw[stg] = nullptr;
		h->raw_bytes[stg] = 0;
		DEV_ALLOC(h, h->d_raw[stg], need);
		h->raw_bytes[stg] = need;
	}
	TRY(h->k1_done[stg].wait(h, h->in_stream));	/* the channeliser of the push before last has read this buffer */
	for (int s = 0; s < h->S; ++s)
		HIPCHK(h, hipMemcpyAsync((char *)h->d_raw[stg] + (size_t)s * per,
					 (const char *)iq + (size_t)s * stream_stride_bytes, per,
					 hipMemcpyHostToDevice, h->in_stream));
	HIPCHK(h, hipEventRecord(h->raw_copied[stg], h->in_stream));
	if (wait_copy)
		HIPCHK(h, hipEventSynchronize(h->raw_copied[stg]));
	in = Input{ h->d_raw[stg], per, true };
	return VDL2GPU_OK;
}

/* Which channeliser kernels a push takes -- arithmetic on the handle's constants, the push's place in the schedule and where its
 * samples lie; nothing is launched here.  K1_FAST at SDRCLK 500 with L = 80 only; K1_PP where whole periods of the dump schedule
 * are whole LO tables and whole 16-byte pieces; the general kernel for everything else, and for the first and the last
 * (super)period of a push the other two do not take as a whole. */
enum { K1_GENERAL, K1_PP, K1_FAST };
struct K1Choice {
	int kind;
	bool whole;		/* the kernel takes all of the push: no general launch at either end */
	long long per_lo;	/* its first (super)period: 0 if whole, else 1 */
	long long sbase0;	/* K1_PP: push-relative index of the first sample of period per_lo */
	int d;			/* K1_PP: samples between the 16-byte boundary below that sample and the sample */
};
static K1Choice choose_k1(const vdl2gpu_t *h, int c0, int64_t J, size_t nsamples, const void *src, size_t stride)
{
	const K1Choice general{ K1_GENERAL, false, 0, 0, 0 };
	K1Choice c = general;
	/* whole periods of the schedule (4*SDRCLK inputs = 84 outputs, the LO table a whole number of times:
	 * SDRINRATE = 4000*SDRCLK, air.c:138) on the period-parallel kernel; the first period (carried partial
	 * window) and the tail on the general one */
	const long long periods = J / K1P_PER_OUT;
	const int per_in = 4 * h->sdrclk;
	if (!(per_in % h->L == 0 && periods >= 4 && !h->quirk && !h->knob.no_k1_fast &&
	      std::min(K1P_CH, h->maxwin) <= h->L))	/* k1_pp steps its LO index by a piece (<= a chunk, <= a window) and wraps it once */
		return general;
	/* a push that starts on a window boundary of the schedule (nothing carried in) and is a whole number of periods (nothing
	 * carried out) needs no general launch at either end: the period-parallel kernel takes all of it (as k1_fast does below) */
	const bool whole_pp = c0 == 0 && nsamples % (size_t)per_in == 0 && J == periods * K1P_PER_OUT && !h->knob.no_whole_pp;
	c.per_lo = whole_pp ? 0 : 1;
	c.sbase0 = k1_win_end(K1P_PER_OUT * c.per_lo - 1, h->sdrclk, c0) + 1;
	/* 16-byte pieces: a period's first sample sits d samples above a 16-byte boundary, the same d for
	 * every period (a period is a whole number of 16-byte pieces) and every stream */
	const uintptr_t a0 = (uintptr_t)src + (uintptr_t)c.sbase0 * h->sample_bytes;
	if ((a0 % 16) % h->sample_bytes || (h->S > 1 && stride % 16) || ((size_t)per_in * h->sample_bytes) % 16)
		return general;
	c.d = (int)((a0 % 16) / h->sample_bytes);
	if (whole_pp && c.d != 0) {	/* (the kernel reads a period from the 16-byte boundary below its first sample: that would lie in front of the buffer) */
		c.per_lo = 1;
		c.sbase0 = k1_win_end(K1P_PER_OUT * c.per_lo - 1, h->sdrclk, c0) + 1;
		const uintptr_t a1 = (uintptr_t)src + (uintptr_t)c.sbase0 * h->sample_bytes;
		if ((a1 % 16) % h->sample_bytes)
			return general;
		c.d = (int)((a1 % 16) / h->sample_bytes);
	}
	const long long nsp = periods / 4;	/* superperiods of 4 periods = 336 outputs = 21 lines of the planes */
	if (h->sdrclk == 500 && h->L == 80 && nsp >= 3 && !h->knob.k1_pp &&
	    (size_t)h->cap * VDL2_CS * sizeof(float2) < VDL2_PLANES_MAX) {	/* k1_fast addresses a stream's planes with 32-bit offsets (vdl2gpu_create holds every handle to it) */
		/* 2 MS/s: the LO values of a window fit a lane's registers (lane = window x channel).  Whole superperiods in
		 * the middle; the first one (carried partial window) and the tail on the general kernel -- unless the push
		 * starts on a window boundary of the schedule (c0 == 0: nothing carried in) and is a whole number of
		 * superperiods (nothing carried out): then the fast kernel takes all of it and the two general launches
		 * (36 us each for 0.02 % of the samples: launch and latency, not work) are not made at all. */
		c.kind = K1_FAST;
		c.whole = c0 == 0 && nsamples % K1F_PER_IN == 0 && J == nsp * K1F_PER_OUT;
		c.per_lo = c.whole ? 0 : 1;
	} else {
		c.kind = K1_PP;
		c.whole = c.per_lo == 0;
	}
	return c;
}

/* The general channeliser for outputs jbeg..jend of the push. */
static void launch_k1_general(vdl2gpu_t *h, const K1Params &k1, hipStream_t ks, long long jbeg, long long jend)
{
	if (jend < jbeg)
		return;
	const long long per_block = K1_OPB * K1_PASSES;
	/* <= VDL2_K1_LDS_MAX either way (vdl2gpu_create) */
	const size_t smem = h->k1_glo ? k1_glo_smem_bytes((uint64_t)h->maxwin) : k1_smem_bytes((uint64_t)h->L, (uint64_t)h->maxwin);
	K1Params q = k1;
	q.jbeg = jbeg;
	q.jend = jend;
	const unsigned gx = (unsigned)((jend - jbeg + 1 + per_block - 1) / per_block);
	const dim3 grid(gx, (unsigned)h->S);
	++h->k1_launches[h->k1_glo ? 1 : 0];
	with_fmt(h->cfg.fmt, [&](auto F) {
		constexpr int FMT = decltype(F)::value;
		if (h->k1_glo)
			launch_k1<K1Params>(h, k1_channelise<FMT, true>, k1_channelise<FMT, true, true>, grid, K1_THREADS, smem, ks, q);
		else
			launch_k1<K1Params>(h, k1_channelise<FMT>, k1_channelise<FMT, false, true>, grid, K1_THREADS, smem, ks, q);
	});
}

/* k1_fast on the push's whole superperiods (all of them, or all but the first and the last: `whole`). */
static void launch_k1_fast(vdl2gpu_t *h, K1Params &k1, bool whole, hipStream_t ks)
{
	const int GS = h->S;
	const long long nsp = k1.J / K1F_PER_OUT;
	k1.per_lo = whole ? 0 : 1;
	k1.per_n = whole ? nsp : nsp - 2;
	k1.edge_state = whole ? 1 : 0;
	k1.lo_ext = h->d_lo_ext;
	k1.lo_stride = h->L + 48;
	/* The grid is resident as a whole: n_cu * 2 * K1F_WAVES_OF(fmt) workgroups of two wavefronts fit.  Per stream
	 * 21 roles x 8 XCDs families of `nfam` workgroups each, which take the family's tickets in turn (see k1_fast);
	 * a family needs no more workgroups than it has tickets.  With several streams the families are many and
	 * small: rather two workgroups each and a twentieth of them waiting for a slot than one each and half the
	 * SIMDs' wavefront slots empty. */
	long long ngrp;
	{
		const long long slots = (long long)h->n_cu * 2 * (h->rot ? K1F_ROT_WAVES : K1F_WAVES_OF(h->cfg.fmt));
		const long long per_fam = (long long)K1F_ROLES * 8 * GS;
		long long nfam = slots / per_fam;
		if (nfam < 4 && (nfam + 1) * per_fam * 100 <= slots * 108)
			++nfam;
		if (h->knob.k1f_nfam > 0)
			nfam = h->knob.k1f_nfam;
		const long long tickets = ((k1.per_n + 7) / 8 + K1F_CHUNK - 1) / K1F_CHUNK;	/* of the family with the most */
		nfam = std::max<long long>(1, std::min(nfam, tickets));
		ngrp = nfam * 8;
	}
	/* the counters are never reset: a launch makes exactly one request per ticket of a family (k1_fast), so the
	 * host knows where each one stands */
	k1.tickets = h->d_k1_tickets;
	for (int x = 0; x < 8; ++x) {
		k1.tbase[x] = h->k1_tbase[x];	/* (every stream stands where the first does: all have seen the same pushes) */
		const long long n_x = (k1.per_n - x + 7) >> 3;
		if (n_x > 0)
			for (int sg = 0; sg < GS; ++sg)
				h->k1_tbase[(size_t)sg * 8 + x] += (unsigned)((n_x + K1F_CHUNK - 1) / K1F_CHUNK);
	}
	const dim3 grid((unsigned)ngrp * K1F_ROLES, (unsigned)GS);
	++h->k1_launches[3];
	with_fmt(h->cfg.fmt, [&](auto F) { launch_k1<K1Params>(h, k1_fast<decltype(F)::value>, k1_fast<decltype(F)::value, true>, grid, K1F_THREADS, 0, ks, k1); });
}

/* k1_pp on the push's whole periods (all of them, or all but the first and the last: ch.whole). */
static void launch_k1_pp(vdl2gpu_t *h, const K1Params &k1, const K1Choice &ch, hipStream_t ks)
{
	const int GS = h->S;
	const long long periods = k1.J / K1P_PER_OUT;
	K1PParams kp{};
	kp.per_lo = ch.per_lo;
	kp.sbase0 = ch.sbase0;
	kp.d = ch.d;
	kp.edge_state = ch.whole ? 1 : 0;
	kp.parity = k1.parity;
	kp.J = k1.J;
	kp.raw = k1.raw;
	kp.stream_stride = k1.stream_stride;
	kp.nbch = h->C;
	kp.per_in = 4 * h->sdrclk;
	kp.L = h->L;
	kp.ph0 = (int)(((long long)k1.no0 + kp.sbase0) % h->L);
	kp.per_n = (int)(ch.whole ? periods : periods - 2);
	kp.lo_ext = h->d_lo_ext;
	kp.lo_stride = h->L + 48;
	kp.dec = k1.dec;
	kp.cap = h->cap;
	kp.ss = h->d_ss;
	int nfmin = 1 << 30, nfmax = 0;
	for (int k = 0; k < K1P_PER_OUT; ++k) {
		kp.wend[k] = (int)(k1_win_end(K1P_PER_OUT * kp.per_lo + k, h->sdrclk, k1.c0) - kp.sbase0);
		const int nf = kp.wend[k] - (k ? kp.wend[k - 1] : -1);
		nfmin = std::min(nfmin, nf);
		nfmax = std::max(nfmax, nf);
	}
	auto proven = [](int nf) { return nf == 23 || nf == 24 || nf == 59 || nf == 60 || nf == 71 || nf == 72 || nf == 119 || nf == 120; };
	kp.fast_div = proven(nfmin) && proven(nfmax) && nfmax - nfmin <= 1;
	kp.nf_lo = nfmin;
	kp.rcp_lo = 1.0f / (float)nfmin;
	kp.rcp_hi = 1.0f / (float)(nfmin + 1);
	/* tasks = (blocks of 64 periods) x (runs of wpt windows): enough of them that the last round of
	 * workgroups is a small share of the launch, as long as possible otherwise */
	const long long blocks = (kp.per_n + 63) / 64;
	const int divs[] = {1, 2, 3, 4, 6, 7, 12, 14, 21, 28};
	const long long resident = (long long)h->n_cu * 3;
	int best = 1;
	double best_eff = -1;
	for (int nsub : divs) {
		const long long tasks = blocks * nsub * GS;
		const long long rounds = (tasks + resident - 1) / resident;
		const double eff = (double)tasks / (double)(rounds * resident) - 0.004 * nsub;	/* shorter tasks pay their start-up more often */
		if (eff > best_eff) {
			best_eff = eff;
			best = nsub;
		}
	}
	if (h->knob.k1_nsub > 0)
		best = h->knob.k1_nsub;
	kp.nsub = best;
	kp.wpt = K1P_PER_OUT / best;
	const dim3 grid((unsigned)(blocks * kp.nsub), (unsigned)GS);
	++h->k1_launches[2];
	with_fmt(h->cfg.fmt, [&](auto F) { launch_k1<K1PParams>(h, k1_pp<decltype(F)::value>, k1_pp<decltype(F)::value, true>, grid, K1P_THREADS, 0, ks, kp); });
}

/* what every channeliser kernel is told of the handle and the push, beside the push's place in the schedule (vdl2gpu_plan) */
static void fill_k1(const vdl2gpu_t *h, K1Params &k1, const Input &in, size_t nsamples, int par)
{
	k1.raw = in.src;
	k1.stream_stride = in.stride;
	k1.nbch = h->C;
	k1.sdrclk = h->sdrclk;
	k1.L = h->L;
	k1.maxwin = h->maxwin;
	k1.parity = (int)(h->pushes & 1);	/* the carried partial window is double-buffered in StreamState.acc: read [parity], written [parity ^ 1] */
	k1.quirk = h->quirk;
	k1.N = (long long)nsamples;
	k1.lo = h->d_lo;
	k1.dec = h->d_dec[par];
	k1.cap = h->cap;
	k1.ss = h->d_ss;
}

/* The channeliser of a push on stream `ks`: k1 comes with the push's place in the schedule; what choose_k1 decided is launched, the
 * general kernel around it where the other one does not take the whole push. */
static int enqueue_k1(vdl2gpu_t *h, K1Params &k1, const Input &in, size_t nsamples, int par, hipStream_t ks, PushTiming &pt)
{
	fill_k1(h, k1, in, nsamples, par);
	const K1Choice ch = choose_k1(h, k1.c0, k1.J, nsamples, in.src, in.stride);
	if (ch.kind == K1_GENERAL)
		launch_k1_general(h, k1, ks, 0, k1.J);
	else {
		/* the kernel takes whole (super)periods of `unit` outputs; unless it takes the whole push, the general kernel takes the
		 * first one (the carried partial window) and everything from the last one on */
		const long long unit = ch.kind == K1_FAST ? K1F_PER_OUT : K1P_PER_OUT;
		if (!ch.whole)
			launch_k1_general(h, k1, ks, 0, unit - 1);
		TRY(mark(h, pt, E_K1_HEAD_END, ks));	/* the wait for the resolver that follows is not channeliser time */
		pt.fast = true;
		TRY(mark(h, pt, E_K1_KERNEL_BEGIN, ks));
		if (ch.kind == K1_FAST)
			launch_k1_fast(h, k1, ch.whole, ks);
		else
			launch_k1_pp(h, k1, ch, ks);
		TRY(mark(h, pt, E_K1_KERNEL_END, ks));
		pt.fast_parts = 1;
		if (!ch.whole)
			launch_k1_general(h, k1, ks, (k1.J / unit - 1) * unit, k1.J);
	}
	HIPCHK(h, hipGetLastError());
	return VDL2GPU_OK;
}

/* The rest of the FRONT stage behind the channeliser: reset of the control words, probe, regions, region scan, sort, the carry
 * for the next push -- and what enqueue_back needs of this push (h->back). */
static int enqueue_front(vdl2gpu_t *h, hipStream_t fs, long long dec_base, PushTiming &pt)
{
	vdl2gpu::Back &p = h->back;	/* (push_impl has put the push's J, sets and path there) */
	const int GS = h->S, par = p.par, ring = p.ring;
	const int64_t J = p.J;
	const bool serial = p.serial, two_streams = p.two_streams;
	TableSet &set = h->set[par];
	{
		KInitParams ki{};
		ki.ctl = set.k2.ctl + CTL_STAGE;
		ki.ctl_words = (int)(h->ctl_words - CTL_STAGE);
		ki.outc = &h->d_outc->ring[ring];
		ki.fail = set.k2.fail;
		ki.redo = set.k2.redo;
		ki.nsc = h->S * VDL2_CS;
		ki.fmask = set.k2.fmask;
		ki.fcnt = h->frames_on ? h->d_fcnt + ring : nullptr;
		hipLaunchKernelGGL(k_push_init, dim3(1), dim3(1024), 0, fs, ki);
	}
	TRY(mark(h, pt, E_SCAN_BEGIN, fs));
	K2Params k2 = set.k2;	/* the set's tables and everything that never changes (fill_set_params); what follows is this push's */
	k2.J = J;
	k2.recs = h->ring[ring].d_recs;
	k2.levels = h->ring[ring].col<vdl2gpu_level_t>(COL_LEVEL);	/* (nullptr without VDL2GPU_F_LEVELS: nothing is measured) */
	k2.soft = h->ring[ring].col<vdl2gpu_soft_t>(COL_SOFT);	/* (nullptr without VDL2GPU_F_SOFT_RS) */
	k2.carrier = h->ring[ring].col<vdl2gpu_carrier_t>(COL_CARRIER);	/* (nullptr without VDL2GPU_F_CARRIER) */
	k2.outc = &h->d_outc->ring[ring];
	k2.dec_base = dec_base;
	k2.scan_lo = dec_base + VDL2_HIST;	/* the scan starts at the first carried frame that has its history */
	k2.probe_par = (int)((dec_base + VDL2_HIST) & 1);
	k2.force_serial = serial ? 1 : 0;
	k2.sel_reserved = p.spec ? 1 : 0;
	if (h->d_headtap) {
		/* VDL2GPU_F_DEBUG_HEADS: one tap buffer for the handle, so the pipeline is drained first -- the back stage and the
		 * tail of the two pushes before would otherwise still be appending to it ("every trigger of the LAST push") */
		HIPCHK(h, hipStreamSynchronize(h->stream));
		HIPCHK(h, hipStreamSynchronize(h->pay_stream));
		HIPCHK(h, hipStreamSynchronize(h->copy_stream));
		HIPCHK(h, hipMemsetAsync(h->d_headtap_n, 0, sizeof(unsigned), fs));
	}
	const unsigned tiles = (unsigned)((VDL2_CARRY_FRAMES + J) / K2A_TS + 2);
	if (!serial) {
		ScanDrain pdrain, rdrain;
		{
			/* as many workgroups as are resident at once, each walking its share of the channel's tiles */
			const unsigned want = h->full_scan ? tiles : tiles / 2 + 1;
			unsigned per = (unsigned)((h->n_cu * h->probe_occ + h->C * GS - 1) / (h->C * GS));
			per = per < 1 ? 1 : (per > want ? want : per);
			per = std::min<unsigned>(per, VDL2_MAXWG);
			/* the probe needs the carry the push before made (the first 49152 frames of this plane set); with the front
			 * stage on two streams (below) that copy is not on this stream */
			TRY(launch_scan(h, SCAN_PROBE, k2, dim3(per, (unsigned)h->C, (unsigned)GS), fs, VDL2_SURV_PROBE,
					h->full_scan ? SURV_CANDS : SURV_PROBE, 0, (h->full_scan ? 4 : 1) * ((want + per - 1) / per), pdrain));
		}
		/* (k2r_regions works the probe's common area off first, k2s_sort the region scan's) */
		launch_per_channel(h, k2r_regions, K2R_NT, fs, k2, pdrain);
		TRY(launch_scan(h, SCAN_REGION, k2, dim3(128, (unsigned)h->C, (unsigned)GS), fs, VDL2_SURV_REGION, SURV_CANDS, 1, 2, rdrain));
		HIPCHK(h, hipGetLastError());
		launch_per_channel(h, k2s_sort, K2S_NT, fs, k2, rdrain);
	}
	TRY(mark(h, pt, E_FRONT_END, fs));	/* end of the front stage's scan + sort */
	HIPCHK(h, hipGetLastError());
	/* ---- end of the FRONT stage */
	if (two_streams)
		HIPCHK(h, hipEventRecord(set.f_done, fs));
	{
		/* the carry for the NEXT push: the last 49152 frames of this push's planes (its own carry included if it is
		 * shorter) go in front of where the next push's output will start, in the other plane set -- a fixed amount,
		 * so that it does not wait for the resolver to say how much is still unconsumed (3 MB per stream).  Behind
		 * this push's scan rather than in front of the next push's channeliser: there the copy sat for 100 us
		 * behind the cluster kernel, which has the higher priority. */
		/* the next plane set's head was last read by the tail of the push two back (a repaired channel's payloads are
		 * decoded late: a burst at the very start of that push lies in its head); the next push's channeliser, right
		 * behind this copy, waits for that same tail anyway */
		if (two_streams)
			TRY(h->set[set_after(par)].k2_done.wait(h, fs));
		K3Params k3{};
		k3.src = h->d_dec[par];
		k3.dst = h->d_dec[set_after(par)];
		k3.cap = h->cap;
		k3.nbch = h->C;
		k3.J = J;
		hipLaunchKernelGGL(k3_carry, dim3(24, (unsigned)h->C, (unsigned)GS), dim3(K3_THREADS), 0, fs, k3);
		HIPCHK(h, hipGetLastError());
		if (two_streams)	/* a following push that keeps to the main stream must see the carry (and with two front streams: the next probe) */
			HIPCHK(h, hipEventRecord(h->f_tail, fs));
		else	/* ... and a following push's front stage this push's channeliser state and carry, made on the main stream */
			TRY(h->k1_ev.record(h, fs));
	}
	p.valid = true;
	p.k2 = k2;
	p.tiles = tiles;
	p.pt_index = h->pending.size();
	return VDL2GPU_OK;
}

/* One push (a part of at most split_samples, see push_checked): checks -> staging copy -> channeliser -> collect the output ring
 * this push reuses -> rest of the front stage -> spill the slab -> back stage and tail -> bookkeeping.  hp(k) closes segment k of
 * the calling thread's time (vdl2gpu_get_host_profile). */
static int push_impl(vdl2gpu_t *h, const void *iq, size_t nsamples, size_t stream_stride_bytes, int memkind, bool wait_copy)
{
	if (!h || (!iq && nsamples))
		return VDL2GPU_EINVAL;
	if (nsamples == 0)
		return VDL2GPU_OK;
	if (nsamples > h->cfg.max_push)
		return VDL2GPU_EINVAL;
	if (h->S > 1 && stream_stride_bytes < nsamples * h->sample_bytes)
		return VDL2GPU_EINVAL;
	if (h->quirk && nsamples % 32768) {
		h->err = "VDL2GPU_F_RTL_QUIRK: every push must be whole 32768-sample blocks";
		return VDL2GPU_EINVAL;
	}
	HIPCHK(h, hipSetDevice(h->cfg.device));
	if (h->pending.size() >= 256) {	/* bound the event backlog */
		HIPCHK(h, hipStreamSynchronize(h->fstream));
		HIPCHK(h, hipStreamSynchronize(h->stream));
		HIPCHK(h, hipStreamSynchronize(h->pay_stream));
		int rc = harvest_timing(h);
		if (rc)
			return rc;
	}
	/* include/vdl2gpu.h: a device buffer must stay unchanged "until the second push after this one has been issued": that push
	 * is this call, for the buffer of the push before last (with two output rings the wait for that push's ring implied it) */
	auto hnow = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	double hp_t = hnow();	/* (always on: six clock reads a push; vdl2gpu_get_host_profile() hands the sums out, VDL2GPU_HOST_PROF prints them at destroy) */
	auto hp = [&](int k) { const double t = hnow(); h->hprof[k] += t - hp_t; hp_t = t; };
	TRY(h->ring[(h->pushes + 1) % VDL2_NRING].in_read.sync(h));
	hp(0);
	vdl2gpu::Back &p = h->back;	/* what the stages share of this push; enqueue_front completes it for enqueue_back */
	p.slab = (int)(h->pushes % VDL2_NSLAB);	/* page-locked slab this push's records are exported to */
	p.ring = (int)(h->pushes % VDL2_NRING);	/* output ring of this push (collected below, once the GPU has been given work to do meanwhile) */
	p.par = (int)(h->pushes % VDL2_NSET);	/* table set and plane set of this push */
	const int stg = (int)(h->pushes & 1);	/* staging buffer of this push; its channeliser's events are k1_done[stg] */
	const int par = p.par;
	OutRing &rg = h->ring[p.ring];
	Input in;
	TRY(stage_input(h, iq, nsamples, stream_stride_bytes, memkind, wait_copy, stg, in));

	K1Params k1{};
	vdl2gpu_plan(h->total_in, nsamples, (unsigned)h->sdrclk, (unsigned)h->L, &k1.c0, &k1.no0, &k1.nf0, &p.J);
	k1.J = p.J;
	if (h->rot) {
		/* where the push's output 0 stands in the 21-output schedule, and the phase index (per Hz of Fd) of the schedule period
		 * it lies in: that period begins at input q * SDRCLK of the stream, and a + e of its windows grows by twice that */
		const uint64_t done = (uint64_t)(((unsigned __int128)h->total_in * 21u) / (unsigned)h->sdrclk);
		const uint64_t qin = done / 21 * (uint64_t)h->sdrclk;
		h->k1rot.i0 = (int)(done % 21);
		h->k1rot.sq0 = (unsigned)vdl2gpu_exact_fo_index(qin, qin, h->cfg.sdrinrate, 1);
	}
	/* A short push (a live SDR block is 1376 frames per channel) is cheaper on the serial machine alone
	 * than through the scan's ten launches: the parallel path only pays from a few thousand frames on. */
	p.serial = h->force_serial || (p.J <= VDL2_SERIAL_BELOW && !h->full_scan && !h->set[p.par].k2.test_noregion);
	p.two_streams = !p.serial;	/* see vdl2gpu::Back */
	p.spec = !h->full_scan && !p.serial && h->S * VDL2_CS <= VDL2_FMASK_SLOTS;	/* see enqueue_back */
	const bool two_streams = p.two_streams;
	hipStream_t fs = two_streams ? h->fstream : h->stream;	/* the front stage's stream */
	/* stream time of frame 0 of this push's planes: the outputs completed before it, minus the carried frames in front */
	const long long dec_base = (long long)(((unsigned __int128)h->total_in * 21u) / (unsigned)h->sdrclk) - VDL2_CARRY_FRAMES;

	PushTiming pt{};
	int rc = get_events(h, pt);
	if (rc)
		return rc;
	pt.samples = nsamples;	/* (per stream) */
	pt.fast = false;
	pt.staged = h->stage_events && (h->pushes % (uint64_t)h->stage_every) == 0;
	pt.index = h->pushes;
	/* The channeliser opens the front stage (fstream; the main stream for a push that takes the serial path).  What its stream waits for: */
	hipStream_t ks = fs;
	if (two_streams) {
		/* the plane set this push's channeliser writes, the table set and the output ring were last used by the push three
		 * back: by its tail (the payload decode of a repaired channel reads the planes to the very end of it) */
		TRY(h->set[par].k2_done.wait(h, fs));
		if (!h->last_two_streams)	/* the previous push's channeliser ran on the main stream: its state and carry */
			TRY(h->k1_ev.wait(h, fs));
	} else {
		if (h->last_two_streams)	/* the previous push's channeliser state and carry were written on the front stream */
			HIPCHK(h, hipStreamWaitEvent(fs, h->f_tail, 0));
		TRY(h->set[set_before(par)].k2_done.wait(h, fs));	/* ... and its tail may have run on the payload stream */
	}
	if (in.staged)	/* host samples: the staging copy */
		HIPCHK(h, hipStreamWaitEvent(ks, h->raw_copied[stg], 0));
	if (pt.staged && h->stage_dump && !h->ev_origin) {	/* the origin of the dump's times: in front of the first push's first event, on its stream */
		NEW_EVENT(h, h->ev_origin, true);
		HIPCHK(h, hipEventRecord(h->ev_origin, ks));
	}
	TRY(mark(h, pt, E_K1_BEGIN, ks));
	TRY(enqueue_k1(h, k1, in, nsamples, par, ks, pt));
	TRY(mark(h, pt, E_K1_END, ks));
	if (memkind != VDL2GPU_MEM_HOST)	/* the caller's device buffer has been read: see the wait at the top */
		TRY(rg.in_read.record(h, ks));
	else
		rg.in_read.clear();
	if (in.staged)	/* (only the staging copy of the push after next waits for it) */
		TRY(h->k1_done[stg].record(h, ks));
	/* The output ring of this push: if the push that last used it (three back) has not been collected yet, collect it now --
	 * the GPU has the two pushes in between and this push's channeliser to work on while this thread waits for that push's
	 * tail. */
	hp(1);	/* channeliser enqueued */
	if (rg.busy) {
		const int rch = harvest_ring(h, p.ring, true);
		if (rch < 0)
			return rch;
	}
	hp(2);	/* ring collected */
	TRY(enqueue_front(h, fs, dec_base, pt));
	h->pending.push_back(pt);
	hp(3);	/* rest of the front stage enqueued */
	spill_slab(h, p.slab);	/* (this push's export will write the slab of the push four back: whatever of it the caller has not taken yet moves aside) */
	hp(4);
	TRY(enqueue_back(h));
	hp(5);	/* back stage enqueued */
	h->last_J = p.J;
	h->last_two_streams = two_streams;
	rg.busy = true;
	rg.slab = p.slab;
	rg.push = h->pushes;
	rg.samples = nsamples;
	h->last_set = par;
	h->total_in += nsamples;
	h->pushes++;
	return VDL2GPU_OK;
}

extern "C" int vdl2gpu_sync(vdl2gpu_t *h)
{
	if (!h)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	HIPCHK(h, hipSetDevice(h->cfg.device));
	HIPCHK(h, hipStreamSynchronize(h->fstream));
	HIPCHK(h, hipStreamSynchronize(h->stream));
	HIPCHK(h, hipStreamSynchronize(h->pay_stream));
	HIPCHK(h, hipStreamSynchronize(h->copy_stream));
	return harvest_timing(h);
}

/* A record in a slab holds what k_export_records sent: the header and the rows the burst uses; everything behind is zero by
 * definition (burst_payload clears a record before it fills it) and is not read from the slab. */
static inline void rec_copy(vdl2gpu_burst_t *dst, const vdl2gpu_burst_t *src, bool from_slab)
{
	if (!from_slab) {
		*dst = *src;
		return;
	}
	const int nb = std::min(std::max(src->nbrow, 0), (int)VDL2GPU_MAXROWS);
	const size_t used = offsetof(vdl2gpu_burst_t, data) + (size_t)nb * VDL2GPU_ROWLEN;
	memcpy(dst, src, used);
	memset(reinterpret_cast<char *>(dst) + used, 0, sizeof *dst - used);
}

/* The slot a handle of the hand-out order (ready_idx) names: the record and, for every side column the handle was made with, the
 * entry beside it -- in a slab or in the pageable queue.  The one place that decodes a handle. */
struct Slot {
	vdl2gpu_burst_t *rec;
	uint8_t *side[VDL2_NCOL];	/* nullptr: the column is off */
	bool from_slab;
};
static inline vdl2gpu_burst_t *rec_at(vdl2gpu_t *h, uint64_t hd)	/* (the record alone: the index sort's comparator) */
{
	const unsigned src = (unsigned)(hd >> 32) & 7u;
	return (src ? h->slab[src - 1].h_recs : h->ready.recs.data()) + (uint32_t)hd;
}
static inline Slot slot_of(vdl2gpu_t *h, uint64_t hd)
{
	const unsigned src = (unsigned)(hd >> 32) & 7u;
	const size_t i = (uint32_t)hd;
	Slot s{};
	s.from_slab = src != 0;
	s.rec = rec_at(h, hd);
	for (int k = 0; k < VDL2_NCOL; ++k)
		if (h->col_on[k])
			s.side[k] = (src ? h->slab[src - 1].h_side[k] : h->ready.side[k].data()) + i * col_bytes[k];
	return s;
}

/* Copy the slot `hd` names to the end of the pageable queue `q` and return its index there.  (`q` is not the storage `hd` points
 * into: a slab's slot goes to h->ready, h->ready's slots go to a queue of their own.) */
static uint64_t move_aside(vdl2gpu_t *h, RecQueue &q, uint64_t hd)
{
	const Slot s = slot_of(h, hd);
	q.recs.emplace_back();
	rec_copy(&q.recs.back(), s.rec, s.from_slab);
	for (int k = 0; k < VDL2_NCOL; ++k)
		if (s.side[k])
			q.side[k].insert(q.side[k].end(), s.side[k], s.side[k] + col_bytes[k]);
	return (uint64_t)(q.recs.size() - 1);
}

static void forget_slabs(vdl2gpu_t *h)	/* (no handle points into a slab any more) */
{
	for (Slab &s : h->slab)
		s.lo = s.hi = 0;
}

/* A ring's slab is about to be written again (its push's back stage is being enqueued): whatever of it has not been
 * handed out yet moves to the pageable queue.  A consumer that polls after every push never gets here with anything. */
static void spill_slab(vdl2gpu_t *h, int slab)
{
	/* only the stretch of the hand-out order that the slab's push put there (a consumer that polls rarely may have 4 x max_bursts
	 * unread entries: walking all of them in every push cost the calling thread more than enqueueing the push) */
	Slab &sl = h->slab[slab];
	const size_t lo = std::max(sl.lo, h->ready_pos), hi = std::min(sl.hi, h->ready_idx.size());
	sl.lo = sl.hi = 0;
	for (size_t i = lo; i < hi; ++i)
		if (((h->ready_idx[i] >> 32) & 7u) == (unsigned)(1 + slab))
			h->ready_idx[i] = move_aside(h, h->ready, h->ready_idx[i]);
}

/* harvest_ring, first part: adapt the part length and the number of repair rounds from the counters the push left. */
static void adapt_from_counters(vdl2gpu_t *h, int ring)
{
	const OutRing &rg = h->ring[ring];
	const PushCounters &cnt = h->h_pin_cnt[ring];
	if (!h->knob.split_fixed && rg.samples) {
		/* How long a part may be follows from how many trigger candidates the busiest channel produced per input sample
		 * in the parts collected lately (the highest of the last four): parts are sized to fill 90 % of the tables, so
		 * that traffic may grow by a tenth from one push to the next before a channel overflows them.  A channel that does
		 * overflow is handled by the serial machine for that part (exact, milliseconds); its density then counts as
		 * twice what the tables hold.  Round 2 halved the parts on an overflow and doubled them again after 1024 quiet
		 * pushes: busy channels ended up in parts a quarter full. */
		const unsigned novf = cnt.cand_ovf;
		const unsigned maxc = cnt.cand_max;
		/* (a part's scan starts at the first carried frame: its count covers the part plus 49152 frames of the one before) */
		const double span = (double)rg.samples + (double)VDL2_CARRY_FRAMES * (double)h->sdrclk / 21.0;
		double d = (double)std::min<unsigned>(maxc, VDL2_CAND_CAP) / span;
		if (novf)
			d = 2.0 * (double)VDL2_CAND_CAP / span;
		h->cand_dens[h->cand_dens_n++ & 3u] = d;
		double dmax = 0.0;
		for (double x : h->cand_dens)
			dmax = std::max(dmax, x);
		size_t lim = h->split_default;
		if (dmax > 0.0)
			lim = (size_t)std::min((double)h->split_default, std::max(0.0, h->knob.table_fill * (double)VDL2_CAND_CAP / dmax - (double)VDL2_CARRY_FRAMES * (double)h->sdrclk / 21.0));
		h->split_samples = std::max(h->split_unit, lim / h->split_unit * h->split_unit);
		if (novf)
			h->last_ovf_push = rg.push;
	}
	/* one round always (enqueue_back); one more after every serial redo -- a repaired chain failed its own verify pass
	 * as often as rounds were scheduled --, and back down one at a time after 256 pushes without a serial redo (what
	 * the first round repairs does not count: it is always there) */
	const unsigned redos = cnt.total.redo, repairs = cnt.total.repairs;
	if (redos != h->redos_seen) {
		h->redos_seen = redos;
		h->last_redo_push = rg.push;
		h->repair_rounds = std::min(4, h->repair_rounds + 1);
	} else if (h->repair_rounds > h->rounds_floor && rg.push > h->last_redo_push + 256) {
		h->repair_rounds--;
		h->last_redo_push = rg.push;
	}
	h->repairs_seen = repairs;
}

/* harvest_ring, second part: the push's n burst records join the host queue, in stream-time order. */
static int collect_records(vdl2gpu_t *h, int ring, unsigned n)
{
	const OutRing &rg = h->ring[ring];
	/* bounded: a consumer that never collects bursts (only frames) loses the oldest ones, counted */
	const size_t qmax = 4 * (size_t)h->rec_cap;
	if (h->ready_idx.size() - h->ready_pos > qmax) {
		const size_t drop = h->ready_idx.size() - h->ready_pos - qmax;
		h->ready_pos += drop;
		h->overflowed += drop;
	}
	if (h->ready_pos == h->ready_idx.size()) {	/* everything handed out: recycle storage */
		h->ready.clear();
		h->ready_idx.clear();
		h->ready_pos = 0;
		forget_slabs(h);
	} else if (h->ready_pos > 1024 && h->ready_pos > h->ready_idx.size() / 2) {	/* the handed-out prefix is the larger part of the storage: drop it
											 * (so the storage never exceeds 2 x the unread records + one push: <= (8 + 1) x max_bursts records) */
		RecQueue keep;
		keep.recs.reserve(h->ready_idx.size() - h->ready_pos);
		for (size_t i = h->ready_pos; i < h->ready_idx.size(); ++i)
			move_aside(h, keep, h->ready_idx[i]);
		h->ready = std::move(keep);
		h->ready_idx.resize(h->ready.recs.size());
		for (size_t i = 0; i < h->ready_idx.size(); ++i)
			h->ready_idx[i] = (uint64_t)i;
		h->ready_pos = 0;
		forget_slabs(h);
	}
	/* the first slab_cap records are already in this ring's slab (k_export_records ran before the event this call
	 * waited for); a push with more than that brings the rest through the bounce buffer */
	const unsigned ns = std::min(n, h->slab_cap);
	const size_t old = h->ready.recs.size();
	for (unsigned done = ns; done < n; done += h->pin_recs) {
		const unsigned m = std::min(h->pin_recs, n - done);
		HIPCHK(h, hipMemcpyAsync(h->h_pin, rg.d_recs + done, (size_t)m * sizeof(vdl2gpu_burst_t),
					 hipMemcpyDeviceToHost, h->copy_stream));
		HIPCHK(h, hipStreamSynchronize(h->copy_stream));
		const vdl2gpu_burst_t *pin = reinterpret_cast<const vdl2gpu_burst_t *>(h->h_pin);
		h->ready.recs.insert(h->ready.recs.end(), pin, pin + m);
		for (int k = 0; k < VDL2_NCOL; ++k) {	/* the side columns present (32, 40 or 48 bytes a record, or 2048 for a map or feedback rows: a pageable copy) */
			if (!h->col_on[k])
				continue;
			std::vector<uint8_t> &q = h->ready.side[k];
			const size_t at = q.size();
			q.resize(at + (size_t)m * col_bytes[k]);
			HIPCHK(h, hipMemcpy(q.data() + at, (const uint8_t *)rg.d_side[k] + (size_t)done * col_bytes[k], (size_t)m * col_bytes[k], hipMemcpyDeviceToHost));
		}
	}
	/* K2d ran ahead of the verify pass: what a repair round (or K2f's serial redo) made void of the first selection
	 * K2d's second pass has tagged (trig_sample == REC_VOID on the device); everything else is a burst of the chain */
	const bool any = rg.spec;
	const size_t iold = h->ready_idx.size();
	auto take = [&](vdl2gpu_burst_t &b, uint64_t handle) {
		if (any && b.trig_sample == REC_VOID)
			return;
		b.trig_sample = dec_to_sample(b.trig_dec, (unsigned)h->sdrclk);
		b.end_sample = dec_to_sample(b.end_dec, (unsigned)h->sdrclk);
		/* d8psk.c:302, same mixed float/double expression */
		b.ppm = (float)((double)(10500.0f * b.df) / (2.0 * M_PI * (double)b.Fr) * 1e6);
		if (h->col_on[COL_LEVEL]) {
			uint8_t *at = slot_of(h, handle).side[COL_LEVEL];
			vdl2gpu_level_t l;
			memcpy(&l, at, sizeof l);
			l.sig_dbfs = (float)(10.0 * log10((double)l.sig_power / h->lev_k));
			l.noise_dbfs = (float)(10.0 * log10((double)l.noise_power / h->lev_k));	/* (NaN stays NaN) */
			memcpy(at, &l, sizeof l);
		}
		if (h->col_on[COL_CARRIER]) {
			uint8_t *at = slot_of(h, handle).side[COL_CARRIER];
			vdl2gpu_carrier_t c;
			memcpy(&c, at, sizeof c);
			if (vdl2gpu_carrier_from_sums(b.df, b.Fr, c.nsym, c.sum_e, c.sum_e2, &c) == VDL2GPU_OK)	/* (a channel with Fr == 0: the sums alone) */
				memcpy(at, &c, sizeof c);
		}
		if (h->col_on[COL_SYMCLK]) {
			uint8_t *at = slot_of(h, handle).side[COL_SYMCLK];
			vdl2gpu_symclk_t c;
			memcpy(&c, at, sizeof c);
			if (vdl2gpu_symclk_from_sums(c.sym_first_dec, c.nsym, &c.e[0][0], h->cfg.sdrinrate, &c, nullptr) == VDL2GPU_OK)	/* (a record that is none: zeros) */
				memcpy(at, &c, sizeof c);
		}
		h->ready_idx.push_back(handle);
	};
	Slab &sl = h->slab[rg.slab];
	for (unsigned i = 0; i < ns; ++i)
		take(sl.h_recs[i], ((uint64_t)(1 + rg.slab) << 32) | i);
	for (size_t i = old; i < h->ready.recs.size(); ++i)
		take(h->ready.recs[i], (uint64_t)i);
	sl.lo = iold;
	sl.hi = h->ready_idx.size();
	std::sort(h->ready_idx.begin() + iold, h->ready_idx.end(), [h](uint64_t x, uint64_t y) {
		const vdl2gpu_burst_t &a = *rec_at(h, x), &b = *rec_at(h, y);
		if (a.end_dec != b.end_dec)
			return a.end_dec < b.end_dec;
		if (a.stream != b.stream)
			return a.stream < b.stream;
		return a.chn < b.chn;
	});
	return VDL2GPU_OK;
}

/* harvest_ring, third part (VDL2GPU_F_FRAMES): the frames of the push's n records join the host queue, in four steps.
 * The queue is bounded like the burst queue: the oldest frames go, counted; and what has been handed out leaves the storage. */
static void trim_frame_queue(vdl2gpu_t *h)
{
	const size_t qmax = 4 * (size_t)h->rec_cap;
	if (h->fready_idx.size() - h->fready_pos > qmax) {
		const size_t drop = h->fready_idx.size() - h->fready_pos - qmax;
		h->fready_pos += drop;
		h->frames_dropped += drop;
	}
	if (h->fready_pos == h->fready_idx.size()) {
		h->fready.clear();
		h->fready_idx.clear();
		h->fready_pos = 0;
	} else if (h->fready_pos > 1024 && h->fready_pos > h->fready_idx.size() / 2) {	/* compact: entries are self-delimiting */
		std::vector<uint8_t> keep;
		std::vector<size_t> kidx;
		for (size_t i = h->fready_pos; i < h->fready_idx.size(); ++i) {
			const uint8_t *e = h->fready.data() + h->fready_idx[i];
			kidx.push_back(keep.size());
			keep.insert(keep.end(), e, e + k4_entry_bytes(reinterpret_cast<const vdl2gpu_frame_t *>(e)->len));
		}
		h->fready.swap(keep);
		h->fready_idx.swap(kidx);
		h->fready_pos = 0;
	}
}

/* `bytes` of device memory come to the host through the page-locked buffer, a buffer's worth at a time: take(chunk, its bytes) */
template <class F> static int copy_out(vdl2gpu_t *h, const void *src, size_t bytes, F &&take)
{
	const size_t pin_bytes = (size_t)h->pin_recs * sizeof(vdl2gpu_burst_t);
	for (size_t done = 0; done < bytes; done += pin_bytes) {
		const size_t m = std::min(pin_bytes, bytes - done);
		HIPCHK(h, hipMemcpyAsync(h->h_pin, (const char *)src + done, m, hipMemcpyDeviceToHost, h->copy_stream));
		HIPCHK(h, hipStreamSynchronize(h->copy_stream));
		take(reinterpret_cast<const uint8_t *>(h->h_pin), m);
	}
	return VDL2GPU_OK;
}

/* walk the entries behind `old` (56 header bytes + len data bytes, rounded up to 8): each joins the index */
static void index_frames(vdl2gpu_t *h, size_t old)
{
	const size_t hdr = offsetof(vdl2gpu_frame_t, data);
	for (size_t off = old; off + hdr <= h->fready.size();) {
		vdl2gpu_frame_t *f = reinterpret_cast<vdl2gpu_frame_t *>(h->fready.data() + off);
		if (f->len < 0 || f->len > VDL2GPU_MAXFRAME || off + hdr + (size_t)f->len > h->fready.size())
			break;
		f->ppm = (float)((double)(10500.0f * f->df) / (2.0 * M_PI * (double)f->Fr) * 1e6);	/* d8psk.c:302 */
		f->block = -1;
		h->fready_idx.push_back((uint32_t)off);
		off += k4_entry_bytes(f->len);
	}
}

/* the order vdl2gpu_poll_frames hands frames out in: by the burst's end, then stream, channel, place in the burst */
static bool frame_earlier(const vdl2gpu_frame_t &a, const vdl2gpu_frame_t &b)
{
	if (a.end_dec != b.end_dec)
		return a.end_dec < b.end_dec;
	if (a.stream != b.stream)
		return a.stream < b.stream;
	if (a.chn != b.chn)
		return a.chn < b.chn;
	return a.seq < b.seq;
}

/* the order of vdl2gpu_decode_blocks: by the caller's block, then place in the burst */
static bool frame_by_block(const vdl2gpu_frame_t &a, const vdl2gpu_frame_t &b)
{
	return a.block != b.block ? a.block < b.block : a.seq < b.seq;
}

static int collect_frames(vdl2gpu_t *h, int ring, unsigned n)
{
	const OutRing &rg = h->ring[ring];
	const unsigned arena0 = h->rec_cap * K4_SLOT;
	/* the arena's entries are the bytes up to the end of the last one that found room (k3_rebase publishes that, not the allocation
	 * counter: an allocation that fails has advanced the counter, and what lies behind the last entry is an earlier push's) */
	const unsigned nbytes = std::min(h->h_pin_cnt[ring].arena_end, h->frame_cap - arena0);
	h->frames_dropped += h->h_pin_cnt[ring].frames_dropped;
	if (!n)
		return VDL2GPU_OK;
	trim_frame_queue(h);
	const size_t old = h->fready.size(), iold = h->fready_idx.size();
	/* the records' slots: keep the occupied ones, packed like arena entries */
	TRY(copy_out(h, rg.d_frames, (size_t)n * K4_SLOT, [h](const uint8_t *pin, size_t m) {
		for (size_t o = 0; o < m; o += K4_SLOT) {
			const int len = reinterpret_cast<const vdl2gpu_frame_t *>(pin + o)->len;
			if (len > 0 && k4_fits_slot(len))
				h->fready.insert(h->fready.end(), pin + o, pin + o + k4_entry_bytes(len));
		}
	}));
	TRY(copy_out(h, (const char *)rg.d_frames + arena0, nbytes, [h](const uint8_t *pin, size_t m) { h->fready.insert(h->fready.end(), pin, pin + m); }));
	index_frames(h, old);
	const uint8_t *fd = h->fready.data();
	std::sort(h->fready_idx.begin() + iold, h->fready_idx.end(), [fd](size_t x, size_t y) {
		return frame_earlier(*reinterpret_cast<const vdl2gpu_frame_t *>(fd + x), *reinterpret_cast<const vdl2gpu_frame_t *>(fd + y));
	});
	return VDL2GPU_OK;
}

/* Move the records of the push that filled `ring` to the host queue.  blocking = false: only if
 * that push has finished (returns 1 if it has not).  The copy runs on its own stream, so a later
 * push keeps the GPU busy meanwhile. */
static int harvest_ring(vdl2gpu_t *h, int ring, bool blocking)
{
	OutRing &rg = h->ring[ring];
	if (!rg.busy)
		return 0;
	if (!blocking) {
		const hipError_t q = hipEventQuery(rg.done());
		if (q == hipErrorNotReady)
			return 1;
		if (q != hipSuccess) {
			h->err = std::string("hipEventQuery: ") + hipGetErrorString(q);
			return VDL2GPU_EHIP;
		}
	}
	const double hq0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
	HIPCHK(h, hipEventSynchronize(rg.done()));
	h->hprof[6] += std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - hq0;
	const RingCount &rec = h->h_pin_cnt[ring].rec;
	const unsigned n = std::min(rec.records, h->rec_cap);
	h->overflowed += rec.dropped;
	adapt_from_counters(h, ring);
	if (n)
		TRY(collect_records(h, ring, n));
	if (h->frames_on)
		TRY(collect_frames(h, ring, n));
	rg.busy = false;
	return 0;
}

static int harvest_all(vdl2gpu_t *h, bool blocking)
{
	/* oldest push first */
	int order[VDL2_NRING], n = 0;
	for (int r = 0; r < VDL2_NRING; ++r)
		if (h->ring[r].busy)
			order[n++] = r;
	std::sort(order, order + n, [&](int a, int b) { return h->ring[a].push < h->ring[b].push; });
	for (int k = 0; k < n; ++k) {
		const int rc = harvest_ring(h, order[k], blocking);
		if (rc < 0)
			return rc;
		if (rc == 1)
			break;	/* not finished yet; anything newer is not finished either */
	}
	return 0;
}

/* Collect everything pushed before this call, waiting for the GPU where it has to -- with the handle's lock RELEASED during every
 * wait, so that a producer thread keeps committing blocks while a consumer thread sits in vdl2gpu_poll().  A ring that the
 * producer reuses meanwhile was collected by the producer's own call first (push_impl), in order. */
static int wait_harvest(vdl2gpu_t *h, std::unique_lock<std::recursive_mutex> &lk)
{
	const uint64_t upto = h->pushes;
	for (;;) {
		int r = -1;
		for (int k = 0; k < VDL2_NRING; ++k)
			if (h->ring[k].busy && h->ring[k].push < upto && (r < 0 || h->ring[k].push < h->ring[r].push))
				r = k;
		if (r < 0)
			return 0;
		const int rc = harvest_ring(h, r, false);
		if (rc < 0)
			return rc;
		if (rc == 1) {
			hipEvent_t ev = h->ring[r].done();
			lk.unlock();
			const hipError_t e = hipEventSynchronize(ev);
			lk.lock();
			if (e != hipSuccess) {
				h->err = std::string("hipEventSynchronize(ring_done): ") + hipGetErrorString(e);
				return VDL2GPU_EHIP;
			}
		}
	}
}

/* side[k]: where the caller wants column k of the records handed out (nullptr: not; only columns the handle has are asked for) */
static int hand_out(vdl2gpu_t *h, vdl2gpu_burst_t *out, int max, void *const side[VDL2_NCOL])
{
	const int n = std::min<int>(max, (int)(h->ready_idx.size() - h->ready_pos));
	for (int i = 0; i < n; ++i) {
		const Slot s = slot_of(h, h->ready_idx[h->ready_pos + i]);
		rec_copy(out + i, s.rec, s.from_slab);
		for (int k = 0; k < VDL2_NCOL; ++k)
			if (side[k])
				memcpy((uint8_t *)side[k] + (size_t)i * col_bytes[k], s.side[k], col_bytes[k]);
	}
	h->ready_pos += (size_t)n;
	return n;
}

/* ---------------------------------------------------------------- block path */
extern "C" int vdl2gpu_decode_blocks(vdl2gpu_t *h, const vdl2gpu_burst_t *blocks, int n,
				     vdl2gpu_frame_t *frames, int max_frames, int *dropped)
{
	return vdl2gpu_decode_blocks_soft(h, blocks, nullptr, n, frames, max_frames, dropped);
}

/* the device memory of one vdl2gpu_decode_blocks call: freed on every way out of it */
struct BlockTemps {
	vdl2gpu_burst_t *blk = nullptr;
	vdl2gpu_soft_t *soft = nullptr;
	vdl2gpu_frame_t *fr = nullptr;
	FrameCounters *cnt = nullptr;
	vdl2gpu_blockrep_t *rep = nullptr;
	vdl2gpu_fb_t *fb = nullptr;
	vdl2gpu_trk_t *trk = nullptr;
	~BlockTemps()
	{
		(void)hipFree(blk);
		(void)hipFree(soft);
		(void)hipFree(fr);
		(void)hipFree(cnt);
		(void)hipFree(rep);
		(void)hipFree(fb);
		(void)hipFree(trk);
	}
};

/* k4_frames on n records of the caller's: an array of vdl2gpu_frame_t, the record count by value */
static K4Params k4_block_params(vdl2gpu_t *h, const BlockTemps &d, int n, int max_frames)
{
	K4Params k4{};
	k4.recs = d.blk;
	k4.nrecs = (unsigned)n;
	k4.rec_cap = (unsigned)n;
	k4.frames = d.fr;
	k4.nframes = d.cnt;
	k4.frame_cap = (unsigned)max_frames;
	k4.compact = 0;
	k4.tabs = h->d_k4tab;
	k4.soft = d.soft;
	k4.rep = d.rep;
	k4.fb = d.fb;
	k4.trk = d.trk;
	return k4;
}

extern "C" int vdl2gpu_decode_blocks_soft(vdl2gpu_t *h, const vdl2gpu_burst_t *blocks, const vdl2gpu_soft_t *soft, int n,
					  vdl2gpu_frame_t *frames, int max_frames, int *dropped)
{
	return vdl2gpu_decode_blocks_report(h, blocks, soft, n, frames, max_frames, dropped, nullptr);
}

extern "C" int vdl2gpu_decode_blocks_report(vdl2gpu_t *h, const vdl2gpu_burst_t *blocks, const vdl2gpu_soft_t *soft, int n,
					    vdl2gpu_frame_t *frames, int max_frames, int *dropped, vdl2gpu_blockrep_t *rep)
{
	return vdl2gpu_decode_blocks_feedback(h, blocks, soft, nullptr, n, frames, max_frames, dropped, rep);
}

extern "C" int vdl2gpu_decode_blocks_feedback(vdl2gpu_t *h, const vdl2gpu_burst_t *blocks, const vdl2gpu_soft_t *soft, const vdl2gpu_fb_t *fb, int n,
					      vdl2gpu_frame_t *frames, int max_frames, int *dropped, vdl2gpu_blockrep_t *rep)
{
	return vdl2gpu_decode_blocks_ex(h, blocks, soft, fb, n, frames, max_frames, dropped, rep, 0u);
}

/* rep: the reporting kernel, and its n reports come back beside the frames; fb: the kernel with the feedback row rule; mode:
 * VDL2GPU_BLK_ALL_FRAMES, the kernel that takes every segment between flags for a candidate, with VDL2GPU_BLK_RAW_FLAGS the one that
 * tells a flag from a stuffed data byte 0x7e (launch_blocks) */
extern "C" int vdl2gpu_decode_blocks_ex(vdl2gpu_t *h, const vdl2gpu_burst_t *blocks, const vdl2gpu_soft_t *soft, const vdl2gpu_fb_t *fb, int n,
					vdl2gpu_frame_t *frames, int max_frames, int *dropped, vdl2gpu_blockrep_t *rep, uint32_t mode)
{
	return vdl2gpu_decode_blocks_tracked(h, blocks, soft, fb, nullptr, n, frames, max_frames, dropped, rep, mode);
}

/* trk: the kernels with the second attempt of vdl2gpu_trk_t (launch_blocks) */
extern "C" int vdl2gpu_decode_blocks_tracked(vdl2gpu_t *h, const vdl2gpu_burst_t *blocks, const vdl2gpu_soft_t *soft, const vdl2gpu_fb_t *fb,
					     const vdl2gpu_trk_t *trk, int n, vdl2gpu_frame_t *frames, int max_frames, int *dropped,
					     vdl2gpu_blockrep_t *rep, uint32_t mode)
{
	if (!h || n < 0 || max_frames < 0 || (n > 0 && !blocks) || (max_frames > 0 && !frames) ||
	    (mode != 0u && mode != VDL2GPU_BLK_ALL_FRAMES && mode != (VDL2GPU_BLK_ALL_FRAMES | VDL2GPU_BLK_RAW_FLAGS)))
		return VDL2GPU_EINVAL;
	if (dropped)
		*dropped = 0;
	if (n == 0 || (max_frames == 0 && !rep))
		return 0;
	HLOCK(h);
	HIPCHK(h, hipSetDevice(h->cfg.device));
#define BLKCHK(expr)                                                          \
	do {                                                                  \
		const hipError_t e__ = (expr);                                \
		if (e__ != hipSuccess)                                        \
			return hip_failed(h, "vdl2gpu_decode_blocks", e__);   \
	} while (0)
	BlockTemps d;
	BLKCHK(hipMalloc(&d.blk, (size_t)n * sizeof(vdl2gpu_burst_t)));
	if (soft)
		BLKCHK(hipMalloc(&d.soft, (size_t)n * sizeof(vdl2gpu_soft_t)));
	BLKCHK(hipMalloc(&d.fr, (size_t)std::max(max_frames, 1) * sizeof(vdl2gpu_frame_t)));
	BLKCHK(hipMalloc(&d.cnt, sizeof *d.cnt));
	if (rep)
		BLKCHK(hipMalloc(&d.rep, (size_t)n * sizeof(vdl2gpu_blockrep_t)));
	if (fb)
		BLKCHK(hipMalloc(&d.fb, (size_t)n * sizeof(vdl2gpu_fb_t)));
	if (trk)
		BLKCHK(hipMalloc(&d.trk, (size_t)n * sizeof(vdl2gpu_trk_t)));
	/* on the stream the kernel runs on: that stream does not wait for the legacy default stream, and a
	 * plain hipMemset() that lands after the kernel's first atomics loses frames */
	BLKCHK(hipMemcpyAsync(d.blk, blocks, (size_t)n * sizeof(vdl2gpu_burst_t), hipMemcpyHostToDevice, h->copy_stream));
	if (soft)
		BLKCHK(hipMemcpyAsync(d.soft, soft, (size_t)n * sizeof(vdl2gpu_soft_t), hipMemcpyHostToDevice, h->copy_stream));
	if (fb)
		BLKCHK(hipMemcpyAsync(d.fb, fb, (size_t)n * sizeof(vdl2gpu_fb_t), hipMemcpyHostToDevice, h->copy_stream));
	if (trk)
		BLKCHK(hipMemcpyAsync(d.trk, trk, (size_t)n * sizeof(vdl2gpu_trk_t), hipMemcpyHostToDevice, h->copy_stream));
	BLKCHK(hipMemsetAsync(d.cnt, 0, sizeof *d.cnt, h->copy_stream));
	const unsigned grid = (unsigned)std::min<long long>(n, (long long)h->n_cu * 32);
	launch_blocks(h->copy_stream, grid, k4_block_params(h, d, n, max_frames), rep != nullptr, mode);
	BLKCHK(hipGetLastError());
	if (rep)	/* (no record is void here: every one of the n has been written) */
		BLKCHK(hipMemcpyAsync(rep, d.rep, (size_t)n * sizeof(vdl2gpu_blockrep_t), hipMemcpyDeviceToHost, h->copy_stream));
	BLKCHK(hipStreamSynchronize(h->copy_stream));
	FrameCounters cnt{};
	BLKCHK(hipMemcpyAsync(&cnt, d.cnt, sizeof cnt, hipMemcpyDeviceToHost, h->copy_stream));
	BLKCHK(hipStreamSynchronize(h->copy_stream));
	const int nf = (int)std::min<unsigned>(cnt.frames, (unsigned)max_frames);
	if (nf > 0) {
		BLKCHK(hipMemcpyAsync(frames, d.fr, (size_t)nf * sizeof(vdl2gpu_frame_t), hipMemcpyDeviceToHost, h->copy_stream));
		BLKCHK(hipStreamSynchronize(h->copy_stream));
	}
#undef BLKCHK
	if (dropped)
		*dropped = (int)cnt.dropped;
	std::sort(frames, frames + nf, frame_by_block);
	return nf;
}

static int poll_frames_impl(vdl2gpu_t *h, vdl2gpu_frame_t *out, int max, bool blocking)
{
	if (!h || (max > 0 && !out) || max < 0)
		return VDL2GPU_EINVAL;
	if (!h->frames_on) {
		h->err = "vdl2gpu_poll_frames needs VDL2GPU_F_FRAMES";
		return VDL2GPU_EINVAL;
	}
	HLOCK(h);
	HIPCHK(h, hipSetDevice(h->cfg.device));
	int rc = blocking ? wait_harvest(h, hlock_) : harvest_all(h, false);
	if (rc)
		return rc;
	const int n = std::min<int>(max, (int)(h->fready_idx.size() - h->fready_pos));
	for (int i = 0; i < n; ++i) {	/* only what is meaningful of the record: its head and data[0..len) */
		const uint8_t *e = h->fready.data() + h->fready_idx[h->fready_pos + i];
		const vdl2gpu_frame_t *f = reinterpret_cast<const vdl2gpu_frame_t *>(e);
		memcpy(&out[i], e, offsetof(vdl2gpu_frame_t, data) + (size_t)f->len);
	}
	h->fready_pos += (size_t)n;
	return n;
}

extern "C" int vdl2gpu_poll_frames(vdl2gpu_t *h, vdl2gpu_frame_t *out, int max)
{
	return poll_frames_impl(h, out, max, true);
}

extern "C" int vdl2gpu_poll_frames_ready(vdl2gpu_t *h, vdl2gpu_frame_t *out, int max)
{
	return poll_frames_impl(h, out, max, false);
}

extern "C" int vdl2gpu_pending(vdl2gpu_t *h)
{
	if (!h)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	HIPCHK(h, hipSetDevice(h->cfg.device));
	int rc = wait_harvest(h, hlock_);
	if (rc)
		return rc;
	return (int)(h->ready_idx.size() - h->ready_pos);
}

/* Pushes the GPU has not finished yet (0..3).  Never waits. */
extern "C" int vdl2gpu_inflight(vdl2gpu_t *h)
{
	if (!h)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	if (h->failed)
		return VDL2GPU_EHIP;
	HIPCHK(h, hipSetDevice(h->cfg.device));
	int n = 0;
	for (int r = 0; r < VDL2_NRING; ++r)
		if (h->ring[r].busy) {
			const hipError_t q = hipEventQuery(h->ring[r].done());
			if (q == hipErrorNotReady)
				++n;
			else if (q != hipSuccess) {
				h->err = std::string("hipEventQuery: ") + hipGetErrorString(q);
				return VDL2GPU_EHIP;
			}
		}
	return n;
}

/* The sixteen collectors.  side.p[k]: where the caller wants column k beside the records (nullptr: not).  who: the entry point as the
 * error texts name it.  When the handle was made without a column that is asked for, the first such column in the order of the
 * arguments is named: "who: arg needs FLAG" (named = false, the two collectors with one column: "who needs FLAG"). */
struct PollCols {
	void *p[VDL2_NCOL];
};
static int poll_impl(vdl2gpu_t *h, vdl2gpu_burst_t *out, int max, const PollCols &side, bool blocking, const char *who, bool named = true)
{
	if (!h || (max > 0 && !out) || max < 0)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	for (int k = 0; k < VDL2_NCOL; ++k)
		if (side.p[k] && !h->col_on[k]) {
			h->err = std::string(who) + (named ? std::string(": ") + col_info[k].arg : std::string()) + " needs " + col_info[k].flag_name;
			return VDL2GPU_EINVAL;
		}
	if (h->failed)
		return VDL2GPU_EHIP;
	HIPCHK(h, hipSetDevice(h->cfg.device));
	int rc = blocking ? wait_harvest(h, hlock_) : harvest_all(h, false);
	if (rc)
		return rc;
	return hand_out(h, out, max, side.p);
}

extern "C" int vdl2gpu_poll(vdl2gpu_t *h, vdl2gpu_burst_t *out, int max) { return poll_impl(h, out, max, {}, true, "vdl2gpu_poll"); }
extern "C" int vdl2gpu_poll_ready(vdl2gpu_t *h, vdl2gpu_burst_t *out, int max) { return poll_impl(h, out, max, {}, false, "vdl2gpu_poll"); }
extern "C" int vdl2gpu_poll_levels(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, int max) { return poll_impl(h, out, max, {{lv}}, true, "vdl2gpu_poll_levels", false); }	/* (lv = NULL: vdl2gpu_poll) */
extern "C" int vdl2gpu_poll_levels_ready(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, int max) { return poll_impl(h, out, max, {{lv}}, false, "vdl2gpu_poll_levels_ready", false); }
extern "C" int vdl2gpu_poll_soft(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, int max) { return poll_impl(h, out, max, {{lv, soft}}, true, "vdl2gpu_poll_soft"); }
extern "C" int vdl2gpu_poll_soft_ready(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, int max) { return poll_impl(h, out, max, {{lv, soft}}, false, "vdl2gpu_poll_soft"); }
extern "C" int vdl2gpu_poll_carrier(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, int max) { return poll_impl(h, out, max, {{lv, soft, car}}, true, "vdl2gpu_poll_carrier"); }
extern "C" int vdl2gpu_poll_carrier_ready(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, int max) { return poll_impl(h, out, max, {{lv, soft, car}}, false, "vdl2gpu_poll_carrier"); }
extern "C" int vdl2gpu_poll_report(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, vdl2gpu_blockrep_t *rep, int max) { return poll_impl(h, out, max, {{lv, soft, car, rep}}, true, "vdl2gpu_poll_report"); }
extern "C" int vdl2gpu_poll_report_ready(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, vdl2gpu_blockrep_t *rep, int max) { return poll_impl(h, out, max, {{lv, soft, car, rep}}, false, "vdl2gpu_poll_report"); }
extern "C" int vdl2gpu_poll_feedback(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, vdl2gpu_blockrep_t *rep, vdl2gpu_fb_t *fb, int max) { return poll_impl(h, out, max, {{lv, soft, car, rep, fb}}, true, "vdl2gpu_poll_feedback"); }
extern "C" int vdl2gpu_poll_feedback_ready(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, vdl2gpu_blockrep_t *rep, vdl2gpu_fb_t *fb, int max) { return poll_impl(h, out, max, {{lv, soft, car, rep, fb}}, false, "vdl2gpu_poll_feedback"); }

extern "C" int vdl2gpu_poll_symclk(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, vdl2gpu_blockrep_t *rep, vdl2gpu_fb_t *fb, vdl2gpu_symclk_t *clk, int max) { return poll_impl(h, out, max, {{lv, soft, car, rep, fb, clk}}, true, "vdl2gpu_poll_symclk"); }
extern "C" int vdl2gpu_poll_symclk_ready(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, vdl2gpu_blockrep_t *rep, vdl2gpu_fb_t *fb, vdl2gpu_symclk_t *clk, int max) { return poll_impl(h, out, max, {{lv, soft, car, rep, fb, clk}}, false, "vdl2gpu_poll_symclk"); }

extern "C" int vdl2gpu_poll_tracked(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, vdl2gpu_blockrep_t *rep, vdl2gpu_fb_t *fb, vdl2gpu_symclk_t *clk, vdl2gpu_trk_t *trk, int max) { return poll_impl(h, out, max, {{lv, soft, car, rep, fb, clk, trk}}, true, "vdl2gpu_poll_tracked"); }
extern "C" int vdl2gpu_poll_tracked_ready(vdl2gpu_t *h, vdl2gpu_burst_t *out, vdl2gpu_level_t *lv, vdl2gpu_soft_t *soft, vdl2gpu_carrier_t *car, vdl2gpu_blockrep_t *rep, vdl2gpu_fb_t *fb, vdl2gpu_symclk_t *clk, vdl2gpu_trk_t *trk, int max) { return poll_impl(h, out, max, {{lv, soft, car, rep, fb, clk, trk}}, false, "vdl2gpu_poll_tracked"); }

/* VDL2GPU_F_CARRIER: the derived values of a carrier record (include/vdl2gpu.h, vdl2gpu_carrier_t) -- the one statement of that
 * arithmetic: collect_records calls it for every record. */
extern "C" int vdl2gpu_carrier_from_sums(float df, int Fr, int nsym, int sum_e, unsigned sum_e2, vdl2gpu_carrier_t *out)
{
	if (!out || nsym <= 0 || Fr == 0)
		return VDL2GPU_EINVAL;
	const double m = (double)sum_e / nsym;
	const double dphi_d = (double)df + M_PI / 8 + m * M_PI / 128;
	const double var = (double)sum_e2 / nsym - m * m;
	out->nsym = nsym;
	out->sum_e = sum_e;
	out->sum_e2 = sum_e2;
	out->reserved = 0;
	out->dphi = (float)dphi_d;
	out->freq_hz = (float)(10500.0 * dphi_d / (2 * M_PI));
	out->ppm = (float)(10500.0 * dphi_d / (2 * M_PI * (double)Fr) * 1e6);
	out->rms_rad = (float)(sqrt(var > 0.0 ? var : 0.0) * M_PI / 128);
	return VDL2GPU_OK;
}

extern "C" int vdl2gpu_get_stats(vdl2gpu_t *h, vdl2gpu_stats_t *out)
{
	if (!h || !out)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	int rc = vdl2gpu_sync(h);
	if (rc)
		return rc;
	std::vector<ChanState> cs((size_t)h->S * VDL2_CS);
	HIPCHK(h, hipMemcpy(cs.data(), h->d_cs, cs.size() * sizeof(ChanState), hipMemcpyDeviceToHost));
	memset(out, 0, sizeof *out);
	out->samples_in = h->total_in;
	out->dec_samples = (uint64_t)(((unsigned __int128)h->total_in * 21u) / (unsigned)h->sdrclk);
	for (int s = 0; s < h->S; ++s)
		for (int c = 0; c < h->C; ++c) {
			const ChanState &x = cs[(size_t)s * VDL2_CS + c];
			out->sync_evals += x.n_eval;
			out->triggers += x.n_trig;
			out->header_rejects += x.n_reject;
			out->bursts += x.n_burst;
			out->deferrals += x.n_defer;
			out->serial_samples += x.n_slow;
			out->candidates += x.n_cand;
			out->serial_redos += x.n_redo;
		}
	out->overflowed = h->overflowed;
	out->frames_dropped = h->frames_dropped;
	{	/* the running total on the device (k2f_commit adds to it), like the channel counters above: current whether or not
		 * the caller has collected the pushes yet */
		unsigned rep = 0;
		HIPCHK(h, hipMemcpy(&rep, &h->d_outc->total.repairs, sizeof rep, hipMemcpyDeviceToHost));
		out->repairs = rep;
	}
	return VDL2GPU_OK;
}

/* Where the calling thread's time inside vdl2gpu_push() went, in seconds, summed over the pushes since the last reset (no pipeline
 * drain: it is host bookkeeping): out[0] waiting for the device buffer of the push before last, [1] enqueueing the channeliser,
 * [2] collecting the output ring this push will reuse (mostly: WAITING for the push three back to finish -- the GPU is the slower
 * side then), [3] enqueueing the rest of the front stage, [4] moving uncollected records out of the slab's way, [5] enqueueing the
 * back stage and the tail, [6] of [2] and of the polling calls: waiting for a ring's completion event, [7] pushes counted. */
extern "C" int vdl2gpu_get_host_profile(vdl2gpu_t *h, double *out8, int reset)
{
	if (!h || !out8)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	for (int i = 0; i < 7; ++i)
		out8[i] = h->hprof[i];
	out8[7] = (double)(h->pushes - h->hprof_push0);
	if (reset) {
		for (int i = 0; i < 7; ++i)
			h->hprof[i] = 0.0;
		h->hprof_push0 = h->pushes;
	}
	return VDL2GPU_OK;
}

extern "C" int vdl2gpu_get_timing(vdl2gpu_t *h, vdl2gpu_timing_t *out, int reset)
{
	if (!h || !out)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	int rc = vdl2gpu_sync(h);
	if (rc)
		return rc;
	*out = h->tm;
	{
		/* stage sums: mean of the pushes that carried stage events x all pushes (the staged ones are every
		 * stage_every-th: scaling their sum by stage_every was biased whenever pushes % stage_every != 0) */
		const double k = h->st_pushes ? (double)h->tm.pushes / (double)h->st_pushes : 0.0;
		out->channelise_ms = k * h->st_k1;
		out->scan_ms = k * h->st_scan;
		out->cluster_ms = k * h->st_cluster;
		out->resolve_ms = k * h->st_resolve;
		out->demod_ms = k * h->st_demod;
		out->other_ms = k * h->st_other;
	}
	if (reset) {
		h->tm = vdl2gpu_timing_t{};
		h->st_scan = h->st_cluster = h->st_resolve = h->st_demod = h->st_other = h->st_k1 = 0;
		h->st_pushes = 0;
	}
	return VDL2GPU_OK;
}

/* ----------------------------------------------------------------- diagnostics */
extern "C" int64_t vdl2gpu_debug_dec(vdl2gpu_t *h, int stream, int ch, float *out, int64_t max_complex)
{
	if (!h || stream < 0 || stream >= h->S || ch < 0 || ch >= h->C || !out)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	if (!h->pushes)
		return VDL2GPU_EINVAL;
	int rc = vdl2gpu_sync(h);
	if (rc)
		return rc;
	StreamState ss;
	HIPCHK(h, hipMemcpy(&ss, h->d_ss + stream, sizeof ss, hipMemcpyDeviceToHost));
	const int par = h->last_set;
	const int64_t n = std::min<int64_t>(ss.last_J, max_complex);
	if (n <= 0)
		return 0;
	HIPCHK(h, hipMemcpy(out, h->d_dec[par] + ((size_t)stream * VDL2_CS + ch) * h->cap + ss.last_fill,
			    (size_t)n * sizeof(float2), hipMemcpyDeviceToHost));
	return n;
}

extern "C" int vdl2gpu_debug_lo(vdl2gpu_t *h, int stream, int ch, float *out, int max_complex)
{
	if (!h || stream < 0 || stream >= h->S || ch < 0 || ch >= h->C || !out || max_complex < h->L)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	HIPCHK(h, hipSetDevice(h->cfg.device));
	HIPCHK(h, hipStreamSynchronize(h->stream));
	HIPCHK(h, hipMemcpy(out, h->d_lo + ((size_t)stream * VDL2_CS + ch) * h->L, (size_t)h->L * sizeof(float2), hipMemcpyDeviceToHost));
	return h->L;
}

extern "C" int vdl2gpu_debug_atan2f(vdl2gpu_t *h, const float *y, const float *x, float *out, size_t n)
{
	if (!h || !y || !x || !out)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	if (!n)
		return VDL2GPU_OK;
	HIPCHK(h, hipSetDevice(h->cfg.device));
	float *d = nullptr;
	HIPCHK(h, hipMalloc(&d, 3 * n * sizeof(float)));
	hipError_t e = hipMemcpyAsync(d, y, n * sizeof(float), hipMemcpyHostToDevice, h->stream);
	if (e == hipSuccess)
		e = hipMemcpyAsync(d + n, x, n * sizeof(float), hipMemcpyHostToDevice, h->stream);
	if (e == hipSuccess) {
		hipLaunchKernelGGL(k_atan2f, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, d, d + n, d + 2 * n, n);
		e = hipStreamSynchronize(h->stream);
	}
	if (e == hipSuccess)
		e = hipMemcpy(out, d + 2 * n, n * sizeof(float), hipMemcpyDeviceToHost);
	(void)hipFree(d);	/* (a call's temporary) */
	if (e != hipSuccess) {
		h->err = hipGetErrorString(e);
		return VDL2GPU_EHIP;
	}
	return VDL2GPU_OK;
}

extern "C" int vdl2gpu_debug_rs(vdl2gpu_t *h, uint8_t *rows, int *eras, const int *no_eras, int *ret, size_t n)
{
	if (!h || n > 0x7fffffffu / 255 || (n && (!rows || !eras || !no_eras || !ret)))
		return VDL2GPU_EINVAL;
	for (size_t i = 0; i < n; ++i) {	/* rs()'s contract: at most NROOTS erasures, at positions of the row */
		if (no_eras[i] < 0 || no_eras[i] > 6)
			return VDL2GPU_EINVAL;
		for (int k = 0; k < no_eras[i]; ++k)
			if (eras[i * 6 + k] < 0 || eras[i * 6 + k] > 254)
				return VDL2GPU_EINVAL;
	}
	HLOCK(h);
	if (!n)
		return VDL2GPU_OK;
	HIPCHK(h, hipSetDevice(h->cfg.device));
	int *d = nullptr;	/* eras[6n], no_eras[n], ret[n], then the rows */
	HIPCHK(h, hipMalloc(&d, 8 * n * sizeof(int) + 255 * n));
	int *const d_eras = d, *const d_ne = d + 6 * n, *const d_ret = d + 7 * n;
	uint8_t *const d_rows = reinterpret_cast<uint8_t *>(d + 8 * n);
	hipError_t e = hipMemcpyAsync(d_eras, eras, 6 * n * sizeof(int), hipMemcpyHostToDevice, h->stream);
	if (e == hipSuccess)
		e = hipMemcpyAsync(d_ne, no_eras, n * sizeof(int), hipMemcpyHostToDevice, h->stream);
	if (e == hipSuccess)
		e = hipMemcpyAsync(d_rows, rows, 255 * n, hipMemcpyHostToDevice, h->stream);
	if (e == hipSuccess) {
		hipLaunchKernelGGL(k4_rs_debug, dim3((unsigned)n), dim3(K4_NT), 0, h->stream, d_rows, d_eras, d_ne, d_ret, h->d_k4tab, (unsigned)n);
		e = hipGetLastError();
		if (e == hipSuccess)
			e = hipStreamSynchronize(h->stream);
	}
	if (e == hipSuccess)
		e = hipMemcpy(eras, d_eras, 6 * n * sizeof(int), hipMemcpyDeviceToHost);
	if (e == hipSuccess)
		e = hipMemcpy(ret, d_ret, n * sizeof(int), hipMemcpyDeviceToHost);
	if (e == hipSuccess)
		e = hipMemcpy(rows, d_rows, 255 * n, hipMemcpyDeviceToHost);
	(void)hipFree(d);	/* (a call's temporary, like vdl2gpu_debug_atan2f's) */
	if (e != hipSuccess) {
		h->err = hipGetErrorString(e);
		return VDL2GPU_EHIP;
	}
	return VDL2GPU_OK;
}

extern "C" int vdl2gpu_debug_counters(vdl2gpu_t *h, unsigned long long *out, int n, int reset)
{
	if (!h || !out || n < 0 || n > VDL2_DBG_WORDS)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	int rc = vdl2gpu_sync(h);
	if (rc)
		return rc;
	HIPCHK(h, hipMemcpy(out, h->d_dbg, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	if (reset) {
		HIPCHK(h, hipMemsetAsync(h->d_dbg, 0, VDL2_DBG_WORDS * sizeof(unsigned long long), h->stream));
		HIPCHK(h, hipStreamSynchronize(h->stream));
	}
	return VDL2GPU_OK;
}

/* channeliser launches since the handle was created: {k1_channelise with the LO table in LDS, k1_channelise with the table in
 * global memory, k1_pp, k1_fast}; returns how many of the four were written */
extern "C" int vdl2gpu_debug_k1(vdl2gpu_t *h, unsigned long long *out, int n)
{
	if (!h || !out || n < 0)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	n = std::min(n, 4);
	for (int i = 0; i < n; ++i)
		out[i] = h->k1_launches[i];
	return n;
}

/* rows of one of the last push's per-channel tables (K2Params::*table, `cap` rows a channel): synchronise, read the channel's count
 * word -- in block `count_block` (CTL_B_*) of the control words --, copy that many rows; returns the count */
template <class T> static int debug_rows(vdl2gpu_t *h, int stream, int ch, int *out, int max_rows, T *K2Params::*table, unsigned cap, int count_block)
{
	if (!h || stream < 0 || stream >= h->S || ch < 0 || ch >= h->C || !out)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	int rc = vdl2gpu_sync(h);
	if (rc)
		return rc;
	const K2Params &k2 = h->set[h->last_set].k2;
	const int sc = stream * VDL2_CS + ch;
	unsigned n = 0;
	HIPCHK(h, hipMemcpy(&n, k2.ctl + CTL_BLOCK(k2, count_block) + sc, sizeof n, hipMemcpyDeviceToHost));
	n = std::min(n, cap);
	n = std::min<unsigned>(n, (unsigned)max_rows);
	if (n)
		HIPCHK(h, hipMemcpy(out, k2.*table + (size_t)sc * cap, (size_t)n * sizeof(T), hipMemcpyDeviceToHost));
	return (int)n;
}

/* candidates of (stream, channel index) found by the last push's sync scan: 6 ints per candidate
 * {nrel, r, bits(p2err), bits(perr), bits(err), bits(pfr)}; returns the count */
extern "C" int vdl2gpu_debug_cands(vdl2gpu_t *h, int stream, int ch, int *out, int max_cands)
{
	return debug_rows(h, stream, ch, out, max_cands, &K2Params::cands, VDL2_CAND_CAP, CTL_B_CAND);
}

/* diagnostics: the cluster heads (cl_pack) of the last push's candidates, in vdl2gpu_debug_cands()'s order */
extern "C" int vdl2gpu_debug_clheads(vdl2gpu_t *h, int stream, int ch, int *out, int max_cands)
{
	return debug_rows(h, stream, ch, out, max_cands, &K2Params::clhead, VDL2_CAND_CAP, CTL_B_CAND);
}

/* verify result of the last push per (stream, channel slot): stream-relative position of the first
 * detector hit the tables lacked, or >= 0x7f000000 when the push verified */
extern "C" int vdl2gpu_debug_fail(vdl2gpu_t *h, int *out, int n)
{
	if (!h || !out || n < h->S * VDL2_CS)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	int rc = vdl2gpu_sync(h);
	if (rc)
		return rc;
	for (int st = 0; st < h->S; ++st)	/* (every stream from the set of its last pass) */
		HIPCHK(h, hipMemcpy(out + (size_t)st * VDL2_CS, h->set[h->last_set].k2.fail + (size_t)st * VDL2_CS, VDL2_CS * sizeof(int), hipMemcpyDeviceToHost));
	return h->S * VDL2_CS;
}

/* diagnostics: the idle segments the last push's resolver asked to have verified {lo, hi, r, pad} */
extern "C" int vdl2gpu_debug_segs(vdl2gpu_t *h, int stream, int ch, int *out, int max_segs)
{
	return debug_rows(h, stream, ch, out, max_segs, &K2Params::segs, VDL2_SEG_CAP, CTL_B_NSEG);
}

/* VDL2GPU_F_DEBUG_HEADS: the header soft bits of every sync trigger any kernel of the LAST push handled -- the
 * clusters of all eight timing classes, the resolver's serial stretches, a serial redo --, 34 x 32-bit words each:
 * {nstar lo, nstar hi, stream * 8 + channel slot, clk0, p2err, perr, err, pfr (float bits), soft[25] (float bits), pad}.
 * Returns the number of entries written to `out` (<= max_entries), in no particular order. */
extern "C" int vdl2gpu_debug_heads(vdl2gpu_t *h, uint32_t *out, int max_entries)
{
	if (!h || !out || max_entries < 0)
		return VDL2GPU_EINVAL;
	HLOCK(h);
	if (!h->d_headtap) {
		h->err = "vdl2gpu_debug_heads needs VDL2GPU_F_DEBUG_HEADS";
		return VDL2GPU_EINVAL;
	}
	int rc = vdl2gpu_sync(h);
	if (rc)
		return rc;
	unsigned n = 0;
	HIPCHK(h, hipMemcpy(&n, h->d_headtap_n, sizeof n, hipMemcpyDeviceToHost));
	n = std::min(n, h->headtap_cap);
	n = std::min<unsigned>(n, (unsigned)max_entries);
	std::vector<HeadTap> tmp(n);
	if (n)
		HIPCHK(h, hipMemcpy(tmp.data(), h->d_headtap, (size_t)n * sizeof(HeadTap), hipMemcpyDeviceToHost));
	for (unsigned i = 0; i < n; ++i) {
		uint32_t *o = out + 34 * (size_t)i;
		const HeadTap &e = tmp[i];
		o[0] = (uint32_t)((unsigned long long)e.nstar & 0xffffffffu);
		o[1] = (uint32_t)((unsigned long long)e.nstar >> 32);
		o[2] = (uint32_t)e.sc;
		o[3] = (uint32_t)e.clk0;
		memcpy(o + 4, &e.p2err, 4);
		memcpy(o + 5, &e.perr, 4);
		memcpy(o + 6, &e.err, 4);
		memcpy(o + 7, &e.pfr, 4);
		memcpy(o + 8, e.soft, 100);
		o[33] = 0;
	}
	return (int)n;
}
