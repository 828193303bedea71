/*
 * vdl2gpu_blocks.h -- the reference's block path as one HIP kernel:
 *   blk_thread()  vdlm2.c:84-161   per msgblk_t: RS(255,249) per row, HDLC bit un-stuffing,
 *                                  flag hunt, frame check, out()
 *   rs()          rs.c:81-291      errors-and-erasures Berlekamp-Massey / Chien / Forney over
 *                                  GF(256)/0x187, first root alpha^120
 *   check_frame() vdlm2.c:38-61    length >= 13, FCS-16 (crc.c) residue 0xf0b8
 *
 * One wavefront per burst record; records come from the output ring of the demodulator (device memory) or from the host.
 * Integer/byte work, bit-exact by construction: every step performs the reference's operations on the operands the reference's
 * loops read, so that miscorrections, early exits and the partially applied corrections of an uncorrectable row agree.
 * k4_frames is a driver over one function per step of blk_thread(), each on the block's K4Shared and with its own account of how the
 * step is spread over the lanes: k4_fetch_head / k4_fetch_rows, k4_rs_rows (k4_rs_row: k4_syndromes, k4_rs_bm, k4_rs_chien,
 * k4_rs_forney; k4_soft_row), k4_unstuff, k4_flag_hunt, k4_fcs_scan, k4_sort_candidates, k4_emit (k4_alloc).  k4_rs_debug runs
 * k4_rs_row alone.
 * The driver is a template over REP: k4_frames is the block path and nothing else; k4_frames_rep also keeps what the steps learn about
 * the burst (K4Rep, in LDS) and writes it out as the record's vdl2gpu_blockrep_t (VDL2GPU_F_BLOCK_REPORT, include/vdl2gpu.h).
 * ... and over FB: k4_frames_fb / k4_frames_rep_fb try the record's decision-feedback row (K4Params.fb, VDL2GPU_F_FEEDBACK) behind a
 * row that rs() fails on (k4_fb_row), in front of the soft trials.
 * ... and over ALL: the four kernels k4_frames_all* (vdl2gpu_allframes.hip) take every segment between two flags for a candidate frame,
 * not only what follows the first flag (VDL2GPU_F_ALL_FRAMES): k4_fcs_scan_all in k4_fcs_scan's place, k4_emit with each frame's own start.
 * ... and over RAW: the four kernels k4_frames_raw* (vdl2gpu_rawflags.hip) are those with VDL2GPU_F_RAW_FLAGS: k4_unstuff marks the bytes
 * that lost a stuffed zero in front of their bit 6, and a byte 0x7e with that mark is data to k4_flag_hunt and k4_fcs_scan_all, no flag.
 * ... and over TRK: the kernels k4_frames_trk* (vdl2gpu_tracked.hip) make a second attempt with the record's timing-tracked rows
 * (K4Params.trk, VDL2GPU_F_TRACKED) for a burst of which the first attempt passes no candidate: k4_trk_second, k4_trk_rows.
 */
#ifndef VDL2GPU_BLOCKS_H
#define VDL2GPU_BLOCKS_H

#define K4_NT 64
#define K4_NOLOG 255
#define K4_MAXBY (VDL2GPU_MAXROWS * 249)
#define K4_SLOT 256
#define K4_NCAND 12	/* candidate frames of one burst that the table holds; further ones are counted as dropped */
#define K4_NONE 0x7fffffff	/* no such byte (k4_flag_hunt) */

/* a compact frame entry: the head of vdl2gpu_frame_t and len data bytes, rounded up to 8 bytes (kernel and host walk the same entries) */
__host__ __device__ inline unsigned k4_entry_bytes(int len) { return ((unsigned)offsetof(vdl2gpu_frame_t, data) + (unsigned)len + 7u) & ~7u; }
/* whether a frame of len > 0 bytes fits its record's slot */
__host__ __device__ inline bool k4_fits_slot(int len) { return (unsigned)offsetof(vdl2gpu_frame_t, data) + (unsigned)len <= K4_SLOT; }

struct K4Params {
	const vdl2gpu_burst_t *recs;
	const unsigned *nrecs_dev;	/* number of records (device word), or nullptr: nrecs */
	unsigned nrecs;
	unsigned rec_cap;
	vdl2gpu_frame_t *frames;
	FrameCounters *nframes;		/* frames written (compact: to the arena) and dropped (buffer full); compact: arena bytes asked for (an
					 * allocation that fails has advanced it too) and the end of the last entry that found room */
	unsigned frame_cap;		/* records, or bytes if compact */
	int compact;			/* 0: an array of vdl2gpu_frame_t.
					 * 1: entries of 56 header bytes (the struct's head) + len data bytes.  Record i owns
					 * the K4_SLOT bytes at i * K4_SLOT: the first frame of its burst goes there when it
					 * fits (len 0: none) -- no allocation, because two thousand waves asking one
					 * device-scope counter for space at the same moment cost more than the whole block
					 * path; longer and further frames go to the arena behind rec_cap slots, entries
					 * rounded up to 8 bytes, space taken from nframes->arena_asked */
	const unsigned *fmask;		/* not nullptr (it is never read): the records come from the pipeline, where K2d's second pass tags the void ones REC_VOID (trig_sample) */
	const unsigned *tabs;		/* K4_TABW words from k4_tables: gexp[512], glog[256], crc_tab[256] */
	const vdl2gpu_soft_t *soft;	/* VDL2GPU_F_SOFT_RS: the records' reliability maps, same index: the row rule of vdl2gpu_soft_t for
					 * rows the reference cannot decode.  nullptr: the reference's block path and nothing else */
	vdl2gpu_blockrep_t *rep;	/* k4_frames_rep only (VDL2GPU_F_BLOCK_REPORT): the records' reports, same index.  k4_frames never
					 * reads it (last: the other members keep their place) */
	const vdl2gpu_fb_t *fb;		/* k4_frames_fb / k4_frames_rep_fb only (VDL2GPU_F_FEEDBACK): the records' decision-feedback rows, same
					 * index: the row rule of vdl2gpu_fb_t.  The other two kernels never read it (last, for the same reason) */
	const vdl2gpu_trk_t *trk;	/* k4_frames_trk* only (VDL2GPU_F_TRACKED): the records' timing-tracked rows, same index: the second attempt
					 * of vdl2gpu_trk_t.  No other kernel reads it (last, for the same reason) */
};

#define K4_TABW ((512 + 256 + 512) / 4)
/* A block is one wavefront: its lanes meet at every instruction, LDS operations of a wave complete in
 * order, and all a barrier has to do is keep the compiler from moving LDS accesses across it.  (A
 * __syncthreads() would also wait for every global store in flight.) */
static_assert(K4_NT == 64, "k4_frames is written for one wavefront per block");
#define K4_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
		       __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
#define K4_RECW0 192	/* words of a record fetched before its header has been looked at: header + two rows */
#define K4_TABL ((K4_TABW + K4_NT - 1) / K4_NT)	/* table words per lane */
static_assert(offsetof(vdl2gpu_burst_t, data) % 4 == 0 && sizeof(vdl2gpu_burst_t) % 4 == 0, "rows are fetched as words");

struct K4Shared {
	uint8_t gexp[512], glog[256];	/* these three in the order of K4Params.tabs */
	unsigned short crc_tab[256];
	unsigned long long recw[(sizeof(vdl2gpu_burst_t) + 7) / 8];	/* the record; its rows are corrected in place */
	uint8_t src[K4_MAXBY + 8];		/* data bytes of all rows, in order */
	unsigned dst[(K4_MAXBY + 8) / 4 + 2];	/* un-stuffed bit stream */
	int eras[6];
	int flag0;		/* index in dst[] (bytes) of the first flag, K4_NONE: none */
	int data0;		/* ... of the first byte behind it that is no flag: hdata[1] */
	int nfr;		/* candidate frames: found (k4_fcs_scan), then held in ends[] (k4_sort_candidates) */
	vdl2gpu_frame_t *room;	/* what lane 0 got from k4_alloc */
	int ends[K4_NCAND];	/* the closing flags of the candidate frames */
	/* Berlekamp-Massey work arrays live here, not in (scratch-backed) private arrays */
	uint8_t lam[8], syn[8], omg[8], root[8], loc[8];
	int rs_deg, rs_count, rs_fail;
	uint8_t save[256];	/* soft mode and the report: the received row, for the trials and for row_changed.  Behind the rows (RAW): the
				 * un-stuffer's marks, see k4_unstuff */
	int cand[4];		/* soft mode: the least reliable candidate positions, most doubtful first */
};

/* VDL2GPU_BLOCKS_DEVICE_ONLY: the translation unit wants the device functions and none of the kernels below (vdl2gpu_allframes.hip
 * defines its own on k4_frames_body) */
#ifndef VDL2GPU_BLOCKS_DEVICE_ONLY
/* GF(256)/0x187 (rs.c:17-79) and FCS-16 reflected 0x8408 (crc.c) tables, built once per handle */
__global__ void k4_tables(unsigned *out)
{
	__shared__ uint8_t t[512 + 256 + 512];
	uint8_t *gexp = t, *glog = t + 512;
	unsigned short *crc = reinterpret_cast<unsigned short *>(t + 768);
	if (threadIdx.x == 0) {
		unsigned x = 1;
		for (int i = 0; i < 255; i++) {
			gexp[i] = (uint8_t)x;
			glog[x] = (uint8_t)i;
			x <<= 1;
			if (x & 0x100)
				x ^= 0x187;
		}
		for (int i = 255; i < 512; i++)
			gexp[i] = gexp[i - 255];
		glog[0] = K4_NOLOG;
	}
	for (int v = threadIdx.x; v < 256; v += blockDim.x) {
		unsigned c = (unsigned)v;
		for (int i = 0; i < 8; i++)
			c = (c & 1) ? ((c >> 1) ^ 0x8408u) : (c >> 1);
		crc[v] = (unsigned short)c;
	}
	__syncthreads();
	for (int i = threadIdx.x; i < K4_TABW; i += blockDim.x)
		out[i] = reinterpret_cast<const unsigned *>(t)[i];
}
#endif

__device__ __forceinline__ int k4_m255(int x)
{
	while (x >= 255) {
		x -= 255;
		x = (x >> 8) + (x & 255);
	}
	return x;
}

/* k4_tables' words into registers, and from there into LDS: two steps, so that a kernel can ask for them beside its other loads */
__device__ __forceinline__ void k4_fetch_tables(const unsigned *tabs, unsigned (&tw)[K4_TABL], int lane)
{
#pragma unroll
	for (int k = 0; k < K4_TABL; ++k)
		tw[k] = (lane + K4_NT * k < K4_TABW) ? tabs[lane + K4_NT * k] : 0u;
}
__device__ __forceinline__ void k4_store_tables(K4Shared &sh, const unsigned (&tw)[K4_TABL], int lane)
{
#pragma unroll
	for (int k = 0; k < K4_TABL; ++k)
		if (lane + K4_NT * k < K4_TABW)
			reinterpret_cast<unsigned *>(sh.gexp)[lane + K4_NT * k] = tw[k];
}

/* exponents of the syndrome sums for this lane's four bytes, (120+i)(254-j) mod 255, a byte each */
__device__ __forceinline__ void k4_sexp_init(unsigned (&sexp)[4][2], int lane)
{
#pragma unroll
	for (int b = 0; b < 4; ++b) {
		const int j = lane * 4 + b;
		sexp[b][0] = sexp[b][1] = 0;
#pragma unroll
		for (int i = 0; i < 6; ++i)
			sexp[b][i / 4] |= (unsigned)k4_m255((120 + i) * (254 - (j < 255 ? j : 254))) << (8 * (i % 4));
	}
}

/* n bytes dealt out in runs of `per` = ceil(n / 64): the lane owns [*lo, *hi) */
__device__ __forceinline__ int k4_lane_span(int n, int lane, int *lo, int *hi)
{
	const int per = (n + K4_NT - 1) / K4_NT;
	*lo = lane * per < n ? lane * per : n;
	*hi = *lo + per < n ? *lo + per : n;
	return per;
}

/* inclusive scan over the lanes: v of lane l becomes op(op(v_0, v_1) ..., v_l) for an associative op(earlier, later) */
template <class T> __device__ __forceinline__ T k4_shfl_up(T v, int d) { return __shfl_up(v, d, K4_NT); }
struct K4Run { int all, trail; };	/* a stretch of the bit stream: nothing but ones?  the ones at its end */
__device__ __forceinline__ K4Run k4_shfl_up(K4Run v, int d) { return {__shfl_up(v.all, d, K4_NT), __shfl_up(v.trail, d, K4_NT)}; }
template <class T, class Op> __device__ __forceinline__ T k4_scan(T v, int lane, Op op)
{
	for (int d = 1; d < K4_NT; d <<= 1) {
		const T o = k4_shfl_up(v, d);
		if (lane >= d)
			v = op(o, v);
	}
	return v;
}

/* set_eras(), vdlm2.c:63-82: a last row of `by` data bytes has had 4 (by <= 30) or 2 (by <= 67) parity bytes less sent: the row's last
 * bytes, which become its first erasures.  Returns their number. */
__device__ __forceinline__ int k4_set_eras(K4Shared &sh, int by, int lane)
{
	const int n = by <= 30 ? 4 : (by <= 67 ? 2 : 0);
	if (lane < n)
		sh.eras[lane] = 255 - n + lane;
	return n;
}

/* rs.c:81-291 for one row whose syndromes are not all zero, in three parts, all of them spread over
 * the lanes (a single lane walking these little polynomials pays an LDS round trip per table look-up
 * and took longer than everything else in the kernel together).
 * k4_rs_bm: erasure locator and Berlekamp-Massey.  Lane i owns coefficient i of lambda (value form) and
 * of B (index form); one step of the reference's r loop is a discrepancy (XOR over the lanes), a shift
 * of B by one lane, and one update per lane -- the same field operations on the same operands as the
 * reference's loops, which read only values of the step before.  Leaves lambda in index form and its
 * degree in LDS. */
__device__ void k4_rs_bm(K4Shared &sh, const unsigned *synv, int no_eras, int lane)
{
	enum { NR = 6, NNN = 255 };
	const uint8_t *gexp = sh.gexp, *glog = sh.glog;
	{
		unsigned mine = 0;
#pragma unroll
		for (int i = 0; i < NR; i++)
			mine = (lane == i) ? synv[i] : mine;
		if (lane < NR)
			sh.syn[lane] = glog[mine];	/* index form, NOLOG for zero */
	}
	unsigned lam = (lane == 0) ? 1u : 0u;
	if (no_eras > 0) {
		if (lane == 1)
			lam = gexp[k4_m255(NNN - 1 - sh.eras[0])];
		for (int i = 1; i < no_eras; i++) {
			const int u = k4_m255(NNN - 1 - sh.eras[i]);
			const unsigned lp = __shfl_up(lam, 1, K4_NT);
			if (lane >= 1 && lane <= i + 1) {
				const unsigned lg = glog[lp];
				if (lg != K4_NOLOG)
					lam ^= gexp[k4_m255(u + lg)];
			}
		}
	}
	unsigned b = (lane <= NR) ? (unsigned)glog[lam] : (unsigned)K4_NOLOG;
	K4_SYNC();
	int el = no_eras;
	for (int r = no_eras + 1; r <= NR; r++) {
		unsigned term = 0;
		if (lane < r && lam) {
			const unsigned sy = sh.syn[r - lane - 1];
			if (sy != K4_NOLOG)
				term = gexp[k4_m255(glog[lam] + sy)];
		}
		term ^= __shfl_xor(term, 1, K4_NT);
		term ^= __shfl_xor(term, 2, K4_NT);
		term ^= __shfl_xor(term, 4, K4_NT);
		const unsigned disc = (unsigned)__builtin_amdgcn_readfirstlane((int)term);
		unsigned bprev = __shfl_up(b, 1, K4_NT);
		if (lane == 0)
			bprev = K4_NOLOG;
		if (disc == 0) {
			b = bprev;
			continue;
		}
		const unsigned dl = glog[disc];
		unsigned t = lam;
		if (lane >= 1 && lane <= NR && bprev != K4_NOLOG)
			t = lam ^ gexp[k4_m255(dl + bprev)];
		if (2 * el <= r + no_eras - 1) {
			el = r + no_eras - el;
			b = (lane <= NR && lam) ? (unsigned)k4_m255(glog[lam] - dl + NNN) : (unsigned)K4_NOLOG;
		} else
			b = bprev;
		lam = t;
	}
	const unsigned li = (lane <= NR) ? (unsigned)glog[lam] : (unsigned)K4_NOLOG;
	if (lane <= NR)
		sh.lam[lane] = (uint8_t)li;
	const unsigned long long m = __ballot(li != K4_NOLOG);	/* bit 0 is always set: lambda_0 = 1 */
	if (lane == 0) {
		sh.rs_deg = 63 - __clzll((long long)m);
		sh.rs_count = 0;
	}
}

/* Chien search, all lanes: position i (1..255) is a root when 1 + sum_j lambda_j alpha^(i j) = 0.  The
 * reference walks i upwards and stops at the deg-th root; a polynomial of degree deg has no more, so
 * listing all roots in the order of i is the same list. */
__device__ void k4_rs_chien(K4Shared &sh, int lane)
{
	const int deg = sh.rs_deg;
	int count = 0;	/* the same in every lane */
	for (int t = 0; t < 4; ++t) {
		const int i = 1 + lane + 64 * t;
		bool isroot = false;
		if (i <= 255) {
			unsigned q = 1;
			for (int j = 1; j <= deg; ++j) {
				const unsigned l = sh.lam[j];
				if (l != K4_NOLOG)
					q ^= sh.gexp[k4_m255((int)l + i * j)];
			}
			isroot = (q == 0);
		}
		const unsigned long long m = __ballot(isroot);
		if (isroot) {
			const int pos = count + __popcll(m & ((1ull << lane) - 1ull));
			if (pos < 6) {
				sh.root[pos] = (uint8_t)i;
				sh.loc[pos] = (uint8_t)((i - 1) % 255);
			}
		}
		count += __popcll(m);
	}
	if (lane == 0)
		sh.rs_count = count;
}

/* Omega and Forney.  Lane i computes omega_i, then lane j the correction for root j.  The reference
 * takes the roots last first and abandons the row at the first zero denominator, keeping the corrections
 * made so far: here, the roots above the highest one with a zero denominator.  eras[] in/out like the
 * reference's eras_pos[]. */
__device__ void k4_rs_forney(K4Shared &sh, uint8_t *data, int lane)
{
	enum { NR = 6, NNN = 255, FIRST = 120 };
	const uint8_t *gexp = sh.gexp, *glog = sh.glog;
	const uint8_t *lam = sh.lam, *syn = sh.syn;
	const int deg = sh.rs_deg, count = sh.rs_count;
	if (deg != count) {
		if (lane == 0)
			sh.rs_fail = 1;
		return;
	}
	unsigned tmp = 0;
	if (lane < NR) {
		for (int j = (deg < lane) ? deg : lane; j >= 0; j--)
			if (syn[lane - j] != K4_NOLOG && lam[j] != K4_NOLOG)
				tmp ^= gexp[k4_m255(syn[lane - j] + lam[j])];
		sh.omg[lane] = glog[tmp];
	}
	if (lane == NR)
		sh.omg[NR] = K4_NOLOG;
	const unsigned long long mo = __ballot(lane < NR && tmp != 0);
	const int dego = mo ? 63 - __clzll((long long)mo) : 0;
	K4_SYNC();
	unsigned num1 = 0, num2 = 0, den = 1;
	int loc = 0;
	if (lane < count) {
		const int root = sh.root[lane];
		loc = sh.loc[lane];
		for (int i = dego; i >= 0; i--)
			if (sh.omg[i] != K4_NOLOG)
				num1 ^= gexp[k4_m255(sh.omg[i] + i * root)];
		num2 = gexp[k4_m255(root * (FIRST - 1) + NNN)];
		den = 0;
		const int top = (deg < NR - 1 ? deg : NR - 1) & ~1;
		for (int i = top; i >= 0; i -= 2)
			if (lam[i + 1] != K4_NOLOG)
				den ^= gexp[k4_m255(lam[i + 1] + i * root)];
	}
	const unsigned long long bad = __ballot(lane < count && den == 0);
	const int jstop = bad ? 63 - __clzll((long long)bad) : -1;
	if (lane < count && lane > jstop && num1)
		data[loc] ^= gexp[k4_m255(glog[num1] + glog[num2] + NNN - glog[den])];
	if (!bad && lane < count)
		sh.eras[lane] = loc;
	if (lane == 0)
		sh.rs_fail = bad ? 1 : 0;
}

/* syndromes S_i = sum_j data[j] alpha^((120+i)(254-j)) of one row, reduced over the lanes: every lane returns all six */
__device__ __forceinline__ unsigned k4_syndromes(const K4Shared &sh, const uint8_t *row, const unsigned (&sexp)[4][2], unsigned (&syn)[6], int lane)
{
#pragma unroll
	for (int i = 0; i < 6; ++i)
		syn[i] = 0;
#pragma unroll
	for (int b = 0; b < 4; ++b) {
		const int j = lane * 4 + b;
		if (j < 255) {
			const unsigned d = row[j];
			if (d) {
				const unsigned lg = sh.glog[d];
#pragma unroll
				for (int i = 0; i < 6; ++i)
					syn[i] ^= sh.gexp[lg + ((sexp[b][i / 4] >> (8 * (i % 4))) & 0xffu)];
			}
		}
	}
	{	/* field sums: XOR over the lanes, four syndromes to a word */
		unsigned s03 = syn[0] | (syn[1] << 8) | (syn[2] << 16) | (syn[3] << 24), s45 = syn[4] | (syn[5] << 8);
		for (int d = 32; d > 0; d >>= 1) {
			s03 ^= __shfl_xor(s03, d, K4_NT);
			s45 ^= __shfl_xor(s45, d, K4_NT);
		}
		syn[0] = s03 & 0xffu;
		syn[1] = (s03 >> 8) & 0xffu;
		syn[2] = (s03 >> 16) & 0xffu;
		syn[3] = s03 >> 24;
		syn[4] = s45 & 0xffu;
		syn[5] = s45 >> 8;
	}
	return syn[0] | syn[1] | syn[2] | syn[3] | syn[4] | syn[5];
}

/* rs() of one row with sh.eras[0..nera) (rs.c:81-291): false when it returns -1.  anyp: where the caller wants to know whether a
 * syndrome of the row was non-zero (all zero: rs() returns 0 at once, and sh.rs_count is not written) */
__device__ __forceinline__ bool k4_rs_row(K4Shared &sh, uint8_t *row, int nera, const unsigned (&sexp)[4][2], int lane, unsigned *anyp = nullptr)
{
	unsigned syn[6];
	const unsigned any = k4_syndromes(sh, row, sexp, syn, lane);
	if (anyp)
		*anyp = any;
	K4_SYNC();
	bool ok = true;
	if (any) {	/* wave-uniform: every lane holds the reduced syndromes */
		k4_rs_bm(sh, syn, nera, lane);
		K4_SYNC();
		k4_rs_chien(sh, lane);
		K4_SYNC();
		k4_rs_forney(sh, row, lane);
		K4_SYNC();
		ok = sh.rs_fail == 0;
	}
	K4_SYNC();
	return ok;
}

/* The soft row rule (vdl2gpu.h, vdl2gpu_soft_t) for a row the reference's rs() has just failed on: `row` holds what it left, sh.save
 * the received row.  The candidates' keys (rel << 8 | position) go through up to four wave-wide minimum searches; each trial starts
 * from the received row.  Without a success the reference's result is written back: it is what rs() leaves, computed again from the
 * same row and erasures.  Returns the number of candidates of the trial that replaced the row (2 or 4), 0: none did. */
/* COPY: k4_frames and k4_frames_rep call copy 0, the two kernels with feedback rows copy 1 -- the same text twice in the library.  With
 * all four calling one function k4_frames_rep is allocated other registers (45 scalar spills for 53), and what a handle without
 * VDL2GPU_F_FEEDBACK runs stays what it was. */
template <int COPY = 0>
__device__ int k4_soft_row(K4Shared &sh, uint8_t *row, const uint8_t *rel, int by, int e0, int pr, const unsigned (&sexp)[4][2], int lane)
{
	const int smax = e0 + 4 <= 4 ? 4 : 2;
	unsigned key[4];
#pragma unroll
	for (int b = 0; b < 4; ++b) {
		const int j = lane * 4 + b;
		const bool cand = j < by || (j >= 249 && j < 249 + pr);
		key[b] = cand ? ((unsigned)rel[j] << 8 | (unsigned)j) : 0xffffffffu;
	}
	int ncand = 0;
	for (int t = 0; t < smax; ++t) {
		unsigned m = key[0];
#pragma unroll
		for (int b = 1; b < 4; ++b)
			m = key[b] < m ? key[b] : m;
		for (int d = 32; d > 0; d >>= 1) {
			const unsigned o = __shfl_xor(m, d, K4_NT);
			m = o < m ? o : m;
		}
		if (m == 0xffffffffu)
			break;
#pragma unroll
		for (int b = 0; b < 4; ++b)
			key[b] = key[b] == m ? 0xffffffffu : key[b];
		if (lane == 0)
			sh.cand[t] = (int)(m & 0xffu);
		++ncand;
	}
	K4_SYNC();
	for (int s = 2; s <= 4; s += 2) {
		if (e0 + s > 4 || s > ncand)
			break;
		for (int i = lane; i < 255; i += K4_NT)
			row[i] = sh.save[i];
		k4_set_eras(sh, by, lane);	/* set_eras()'s positions, then the candidates */
		if (lane >= e0 && lane < e0 + s)
			sh.eras[lane] = sh.cand[lane - e0];
		K4_SYNC();
		if (k4_rs_row(sh, row, e0 + s, sexp, lane)) {
			unsigned syn[6];
			const unsigned any = k4_syndromes(sh, row, sexp, syn, lane);
			K4_SYNC();
			if (!any)
				return s;
		}
	}
	for (int i = lane; i < 255; i += K4_NT)
		row[i] = sh.save[i];
	k4_set_eras(sh, by, lane);
	K4_SYNC();
	k4_rs_row(sh, row, e0, sexp, lane);
	return 0;
}

/* The feedback row rule (vdl2gpu.h, vdl2gpu_fb_t, step 2) for a row the reference's rs() has just failed on: the record's feedback row
 * (global memory) goes where the row was, rs() runs on it with the same fixed erasures, and it stays if that returns >= 0 and leaves
 * all six syndromes zero. */
__device__ __forceinline__ bool k4_fb_row(K4Shared &sh, uint8_t *row, const uint8_t *fbrow, int by, int e0, const unsigned (&sexp)[4][2], int lane)
{
	for (int i = lane; i < 255; i += K4_NT)
		row[i] = fbrow[i];
	k4_set_eras(sh, by, lane);
	K4_SYNC();
	if (!k4_rs_row(sh, row, e0, sexp, lane))
		return false;
	unsigned syn[6];
	const unsigned any = k4_syndromes(sh, row, sexp, syn, lane);
	K4_SYNC();
	return !any;
}

/* ... and when neither it nor a soft trial follows: what the reference left, computed again from the received row in sh.save */
__device__ __forceinline__ void k4_ref_row_again(K4Shared &sh, uint8_t *row, int by, int e0, const unsigned (&sexp)[4][2], int lane)
{
	for (int i = lane; i < 255; i += K4_NT)
		row[i] = sh.save[i];
	k4_set_eras(sh, by, lane);
	K4_SYNC();
	k4_rs_row(sh, row, e0, sexp, lane);
}

/* ---- the record (msgblk_t, vdlm2.c:84-98): its front -- header and two rows -- into registers, and from there into LDS; the
 * remaining rows follow once the header has been read there */
__device__ __forceinline__ void k4_fetch_head(const vdl2gpu_burst_t *g, unsigned (&rw)[K4_RECW0 / K4_NT], int lane)
{
#pragma unroll
	for (int k = 0; k < K4_RECW0 / K4_NT; ++k)
		rw[k] = reinterpret_cast<const unsigned *>(g)[lane + K4_NT * k];
}

__device__ __forceinline__ void k4_fetch_rows(K4Shared &sh, const vdl2gpu_burst_t *g, int nbrow, int lane)
{
	for (int i = K4_RECW0 + lane; i < ((int)offsetof(vdl2gpu_burst_t, data) + nbrow * VDL2GPU_ROWLEN + 3) / 4; i += K4_NT)
		reinterpret_cast<unsigned *>(sh.recw)[i] = reinterpret_cast<const unsigned *>(g)[i];
}

/* ---- RS per row (rows in order: eras_pos[] carries over, vdlm2.c:104-113), with the soft row rule behind a row that rs() fails on when
 * the record has a reliability map (soft: the record's, or nullptr).  The rows' data bytes go to sh.src; returns their number.
 * REP: rep (in LDS, zeroed) gets the rows' part of the report -- row_roots and row_how from the reference's run on the received row
 * (k4_rs_row's result, sh.rs_count as k4_rs_debug reads it) and from what k4_soft_row says; row_changed from a comparison of the final
 * row with the received one in sh.save, four bytes a lane, masked to the transmitted positions and counted over the wave; the three sums
 * are kept in registers (they are the same in every lane) and stored once. */
/* FB: fb is the record's feedback rows; a row rs() fails on first tries fb->data[r] (k4_fb_row); the soft trials follow only if that
 * fails too, and without them the reference's result is put back (k4_soft_row does that itself). */
template <bool REP, bool FB>
__device__ __forceinline__ int k4_rs_rows(K4Shared &sh, const vdl2gpu_soft_t *soft, int nbrow, int nlbyte, const unsigned (&sexp)[4][2], int lane,
					  vdl2gpu_blockrep_t *rep, const vdl2gpu_fb_t *fb)
{
	uint8_t *const rows = reinterpret_cast<uint8_t *>(sh.recw) + offsetof(vdl2gpu_burst_t, data);
	if (lane < 6)
		sh.eras[lane] = 0;
	K4_SYNC();
	int nby = 0;
	unsigned changed = 0, failed = 0, rescued = 0;	/* (REP) */
	for (int r = 0; r < nbrow; ++r) {
		const int by = r == nbrow - 1 ? nlbyte : 249;
		const int nera = k4_set_eras(sh, by, lane);	/* (a full row has none) */
		uint8_t *const row = rows + r * VDL2GPU_ROWLEN;
		if (REP || FB || soft) {
			for (int i = lane; i < 255; i += K4_NT)
				sh.save[i] = row[i];
			K4_SYNC();
		}
		if constexpr (REP) {
			const BurstGeom g = burst_geom(nbrow, nlbyte);
			const int pr = r < g.nf_rows - 1 ? 6 : (r == g.nf_rows - 1 ? g.nf_last : 0);	/* the transmitted parity of row r */
			unsigned any;
			const bool ok = k4_rs_row(sh, row, nera, sexp, lane, &any);
			const int roots = !ok ? -1 : (any ? sh.rs_count : 0);
			unsigned how = !any ? VDL2GPU_ROW_CLEAN : (ok ? VDL2GPU_ROW_REF : VDL2GPU_ROW_FAIL);
			if constexpr (FB) {
				if (!ok) {
					if (k4_fb_row(sh, row, &fb->data[r][0], by, nera, sexp, lane))
						how = VDL2GPU_ROW_FEEDBACK;
					else if (soft && nera + 2 <= 4) {
						const int s = k4_soft_row<1>(sh, row, &soft->rel[r][0], by, nera, pr, sexp, lane);
						how = s == 2 ? VDL2GPU_ROW_SOFT2 : (s == 4 ? VDL2GPU_ROW_SOFT4 : VDL2GPU_ROW_FAIL);
					} else
						k4_ref_row_again(sh, row, by, nera, sexp, lane);
				}
			} else if (!ok && soft && nera + 2 <= 4) {
				const int s = k4_soft_row(sh, row, &soft->rel[r][0], by, nera, pr, sexp, lane);
				how = s == 2 ? VDL2GPU_ROW_SOFT2 : (s == 4 ? VDL2GPU_ROW_SOFT4 : VDL2GPU_ROW_FAIL);
			}
			K4_SYNC();	/* the row is final */
			unsigned nch = 0;
#pragma unroll
			for (int b = 0; b < 4; ++b) {
				const int j = lane * 4 + b;
				const bool sent = j < by || (j >= 249 && j < 249 + pr);
				nch += (unsigned)__popcll(__ballot(sent && row[j < 255 ? j : 254] != sh.save[j < 255 ? j : 254]));
			}
			if (lane == 0) {
				rep->row_roots[r] = (int8_t)roots;
				rep->row_how[r] = (uint8_t)how;
				rep->row_changed[r] = (uint8_t)nch;
			}
			changed += nch;
			failed += how == VDL2GPU_ROW_FAIL;
			rescued += how == VDL2GPU_ROW_SOFT2 || how == VDL2GPU_ROW_SOFT4 || (FB && how == VDL2GPU_ROW_FEEDBACK);
		} else if constexpr (FB) {
			if (!k4_rs_row(sh, row, nera, sexp, lane) && !k4_fb_row(sh, row, &fb->data[r][0], by, nera, sexp, lane)) {
				if (soft && nera + 2 <= 4) {
					const BurstGeom g = burst_geom(nbrow, nlbyte);
					const int pr = r < g.nf_rows - 1 ? 6 : (r == g.nf_rows - 1 ? g.nf_last : 0);	/* the transmitted parity of row r */
					k4_soft_row<1>(sh, row, &soft->rel[r][0], by, nera, pr, sexp, lane);
				} else
					k4_ref_row_again(sh, row, by, nera, sexp, lane);
			}
		} else if (!k4_rs_row(sh, row, nera, sexp, lane) && soft) {
			const BurstGeom g = burst_geom(nbrow, nlbyte);
			const int pr = r < g.nf_rows - 1 ? 6 : (r == g.nf_rows - 1 ? g.nf_last : 0);	/* the transmitted parity of row r */
			if (nera + 2 <= 4)
				k4_soft_row(sh, row, &soft->rel[r][0], by, nera, pr, sexp, lane);
		}
		for (int i = lane; i < by; i += K4_NT)
			sh.src[nby + i] = rows[r * VDL2GPU_ROWLEN + i];
		nby += by;
	}
	if (REP && lane == 0) {
		rep->bytes_changed = (uint16_t)changed;
		rep->rows_failed = (uint16_t)failed;
		rep->rows_rescued = (uint16_t)rescued;
	}
	return nby;
}

/* ---- HDLC bit un-stuffing (vdlm2.c:116-128) of sh.src[0..nby) into sh.dst; returns the number of bits kept.  A stuffed zero is a
 * zero after exactly five ones: the run of ones in front of a bit does not depend on what was dropped before, so every lane knows the
 * run it starts in from a scan of (all ones?, trailing ones) and drops its own zeros; a prefix sum of the kept counts places its bits.
 * A zero is a stuffed one iff exactly five ones stand in front of it.  With the (at most six relevant) bits in front of a byte put
 * below it, that is a bit pattern test on the whole byte. */
__device__ __forceinline__ unsigned k4_stuffed(unsigned v, int t)
{
	const int tt = t < 6 ? t : 6;
	const unsigned W = (v << 6) | (((1u << tt) - 1u) << (6 - tt));
	const unsigned D = ~W & (W << 1) & (W << 2) & (W << 3) & (W << 4) & (W << 5) & ~(W << 6);
	return (D >> 6) & 0xffu;
}

/* ones at the end of the stream after byte v, t of them in front of it: those above the byte's highest zero (bit 7 downwards) */
__device__ __forceinline__ int k4_run_after(unsigned v, int t) { return v == 0xffu ? t + 8 : __clz((int)((~v & 0xffu) << 24)); }

/* RAW (VDL2GPU_F_RAW_FLAGS, include/vdl2gpu.h): the un-stuffer also leaves one bit per un-stuffed byte in marks[], bit q & 31 of word
 * q >> 5: a zero was dropped in front of the byte's bit 6.  A byte that un-stuffs to 0x7e can have lost a zero nowhere else (its bit 0 is
 * a kept zero, five ones follow), so for such a byte the mark says "the six ones were not adjacent in the stuffed stream": a data byte,
 * no flag -- the reference's t is 1, not 6, at the byte's last bit.  The lane knows where each of its dropped zeros falls in the output. */
#define K4_MARKW 64	/* words of marks: one bit for each of K4_MAXBY bytes, and a word behind them for k4_lane_marks */
static_assert(K4_MAXBY <= 32 * (K4_MARKW - 1) && K4_MARKW == K4_NT, "one mark per un-stuffed byte; every lane clears one word");

/* They live in sh.save: the received row is dead once k4_rs_rows is through, and the RAW kernels keep their siblings' LDS */
static_assert(sizeof(K4Shared::save) >= 4 * K4_MARKW && offsetof(K4Shared, save) % 4 == 0, "the marks fit the saved row's place, as words");

/* the marks of the lane's un-stuffed bytes [c0, c0 + 32): bit i - c0 is byte i's (a lane's span is 32 bytes at most) */
static_assert((K4_MAXBY + K4_NT - 1) / K4_NT <= 32, "a lane's marks are one word");
__device__ __forceinline__ unsigned k4_lane_marks(const unsigned *marks, int c0)
{
	const unsigned long long w = (unsigned long long)marks[(c0 >> 5) + 1] << 32 | marks[c0 >> 5];
	return (unsigned)(w >> (c0 & 31));
}

template <bool RAW = false>
__device__ __forceinline__ int k4_unstuff(K4Shared &sh, int nby, int lane, unsigned *marks = nullptr)
{
	for (int i = lane; i < nby / 4 + 2; i += K4_NT)
		sh.dst[i] = 0u;
	if constexpr (RAW)
		marks[lane] = 0u;	/* (K4_MARKW == K4_NT) */
	K4_SYNC();
	int b0, b1;	/* lane owns bytes [b0, b1) */
	k4_lane_span(nby, lane, &b0, &b1);
	K4Run run = {1, 0};
	for (int i = b0; i < b1; ++i) {
		const unsigned v = sh.src[i];
		run.all &= v == 0xffu;
		run.trail = k4_run_after(v, run.trail);
	}
	/* run of ones in front of the lane's first bit: scan of t' = all ? t + trail : trail */
	run = k4_scan(run, lane, [](K4Run a, K4Run b) { return K4Run{a.all & b.all, b.all ? a.trail + b.trail : b.trail}; });
	int tin = __shfl_up(run.trail, 1, K4_NT);
	if (lane == 0)
		tin = 0;
	int nkeep = 0;
	for (int i = b0, t = tin; i < b1; ++i) {
		const unsigned v = sh.src[i];
		nkeep += 8 - __popc(k4_stuffed(v, t));
		t = k4_run_after(v, t);
	}
	const int kept_incl = k4_scan(nkeep, lane, [](int a, int b) { return a + b; });	/* prefix sum of the kept bits */
	{
		int t = tin, o = kept_incl - nkeep;
		unsigned long long acc = 0;	/* bits of the output word being filled, and what spills over */
		int w = o >> 5;
		for (int i = b0; i < b1; ++i) {
			unsigned v = sh.src[i];
			unsigned dr = k4_stuffed(v, t);
			t = k4_run_after(v, t);
			int nbits = 8;
			while (dr) {	/* squeeze the dropped zeros out, highest first (there are at most two) */
				const int d = 31 - __clz((int)dr);
				v = (v & ((1u << d) - 1u)) | ((v >> (d + 1)) << d);
				dr &= ~(1u << d);
				--nbits;
				if constexpr (RAW) {
					const int at = o + d - __popc(dr);	/* bits kept in front of this zero: those below it in v that stay */
					if ((at & 7) == 6)
						atomicOr(&marks[at >> 8], 1u << ((at >> 3) & 31));
				}
			}
			acc |= (unsigned long long)v << (o & 31);
			o += nbits;
			if ((o >> 5) != w) {
				atomicOr(&sh.dst[w], (unsigned)acc);
				acc >>= 32;
				++w;
			}
		}
		if ((unsigned)acc)
			atomicOr(&sh.dst[w], (unsigned)acc);
	}
	K4_SYNC();
	return __shfl(kept_incl, K4_NT - 1, K4_NT);
}

/* ---- first flag: the byte at which the OR of all bytes so far equals 0x7e (vdlm2.c:129-133); flags right behind the first one are
 * swallowed (k == 1, vdlm2.c:134-135).  The lane owns the un-stuffed bytes [c0, c1).  Returns the first byte behind the flags,
 * hdata[1], or K4_NONE: no flag, or nothing but flags behind it.  RAW: only a true flag is swallowed (marks[], see k4_unstuff). */
template <bool RAW = false>
__device__ __forceinline__ int k4_flag_hunt(K4Shared &sh, int c0, int c1, int lane, const unsigned *marks = nullptr)
{
	const uint8_t *B = reinterpret_cast<const uint8_t *>(sh.dst);
	unsigned lor = 0;	/* OR of all bytes in front of the lane's */
	for (int i = c0; i < c1; ++i)
		lor |= B[i];
	lor = __shfl_up(k4_scan(lor, lane, [](unsigned a, unsigned b) { return a | b; }), 1, K4_NT);
	if (lane == 0) {
		lor = 0;
		sh.flag0 = K4_NONE;
		sh.data0 = K4_NONE;
	}
	K4_SYNC();
	for (int i = c0; i < c1; ++i) {
		lor |= B[i];
		if (lor == 0x7eu) {
			atomicMin(&sh.flag0, i);
			break;
		}
		if (lor & ~0x7eu)
			break;	/* a bit outside 0x7e is set for good: no flag will ever be seen */
	}
	K4_SYNC();
	const int m0 = sh.flag0;
	unsigned data7e = 0;	/* RAW: a data byte 0x7e is hdata[1] like any other */
	if constexpr (RAW)
		data7e = k4_lane_marks(marks, c0);
	if (m0 != K4_NONE)
		for (int i = c0 > m0 + 1 ? c0 : m0 + 1; i < c1; ++i) {
			const bool flag = B[i] == 0x7eu && !(RAW && ((data7e >> (i - c0)) & 1u));
			if (!flag) {
				atomicMin(&sh.data0, i);
				break;
			}
		}
	K4_SYNC();
	return sh.data0;
}

/* ---- hdata[] = 0x7e, B[m1], B[m1+1], ...; every later 0x7e closes a candidate frame hdata[0..k] whose FCS runs over hdata[1..k-1]
 * (check_frame, vdlm2.c:38-61).  All candidates start at m1, so one running FCS serves -- computed lane-parallel: the FCS is linear,
 * the state at the start of a lane's bytes is (state one lane earlier, advanced over `per` zero bytes) xor (FCS from zero of that
 * lane's bytes); that recurrence is scanned in log2(64) doubling steps, the advance map (16 columns, one per lane) being squared
 * alongside.  Leaves the closing flags of the frames that check in sh.ends, in any order, and their number in sh.nfr.
 * REP: every lane also counts the 0x7e bytes it meets (B[m1] is none) and those of them that close a candidate of l < 13; the two
 * counts (at most K4_MAXBY < 65536 and at most 10: l < 13 ends at m1 + 10) are added up over the wave in one word and returned:
 * cand | too_short << 16.  The candidates of l >= 13 with the wrong FCS are the rest: cand - too_short - sh.nfr.  Without REP: 0.
 * ALL (VDL2GPU_F_ALL_FRAMES, include/vdl2gpu.h): every 0x7e at q >= m1 closes the segment that began behind the flag before it (s_0 = m1,
 * s_{j+1} = q_j + 1, l_j = q_j - s_j + 2), and the FCS starts again from 0xffff behind it.  A lane whose bytes hold such a flag ends in a
 * state that does not depend on the lanes before it -- the FCS from 0xffff over what follows its last flag -- so the scan's element is
 * (reset, x) with (r_a, x_a) o (r_b, x_b) = r_b ? (1, x_b) : (r_a, A^n_b x_a ^ x_b): associative, and the advance map and its squaring
 * are untouched.  The lane that holds m1 starts from 0xffff and is a reset by construction.  A maximum scan of the lanes' last flags gives
 * every lane the start of the segment its first byte lies in.  sh.ends[] gets q << 16 | s of the segments that pass, in stream order
 * (ranks from a prefix sum of the lanes' counts: the first K4_NCAND of the burst are the ones kept), sh.nfr their number; the counts
 * follow the same rule: too_short is l_j < 13, flags side by side (l_j = 2) included.
 * RAW (VDL2GPU_F_RAW_FLAGS): "a flag" is a byte 0x7e without the un-stuffer's mark (k4_unstuff); a marked one is a data byte like any other. */
/* segments that pass are 12 bytes apart at least (l >= 13), so a lane meets at most three closing flags of such */
#define K4_ALL_LANE_MAX 3
static_assert((K4_MAXBY + K4_NT - 1) / K4_NT <= 12 * K4_ALL_LANE_MAX, "a lane's span holds at most K4_ALL_LANE_MAX passing segments' ends");
static_assert(K4_MAXBY < 65536, "a candidate's closing flag and start share a word");

template <bool REP, bool RAW = false>
__device__ __forceinline__ unsigned k4_fcs_scan_all(K4Shared &sh, int m1, int per, int c0, int c1, int lane, const unsigned *marks = nullptr)
{
	const uint8_t *B = reinterpret_cast<const uint8_t *>(sh.dst);
	unsigned data7e = 0;	/* RAW: the lane's bytes that are no flag whatever their value, bit i - c0 (k4_lane_marks) */
	if constexpr (RAW)
		data7e = k4_lane_marks(marks, c0);
	unsigned col = 0;	/* the advance map, one state bit per lane */
	if (lane < 16) {
		col = 1u << lane;
		for (int i = 0; i < per; ++i)
			col = (col >> 8) ^ sh.crc_tab[col & 0xffu];
	}
	const int L1 = m1 / per;	/* lane that holds m1 */
	const int b0 = (lane == L1) ? m1 : c0;	/* the lane's first byte that counts */
	unsigned x = 0;		/* FCS over the lane's own bytes: from 0xffff behind m1 and behind every flag, else from zero */
	int reset = lane == L1;	/* ... which is then all there is to its end state */
	int last = -1;		/* the lane's last flag */
	if (lane >= L1) {
		x = reset ? 0xffffu : 0u;
		for (int i = b0; i < c1; ++i) {
			const unsigned v = B[i];
			if (v == 0x7eu && !(RAW && ((data7e >> (i - c0)) & 1u))) {
				x = 0xffffu;
				reset = 1;
				last = i;
			} else
				x = (x >> 8) ^ sh.crc_tab[(x ^ v) & 0xffu];
		}
	}
	for (int d = 1; d < K4_NT; d <<= 1) {
		unsigned xl = __shfl_up(x, d, K4_NT);
		int rl = __shfl_up(reset, d, K4_NT);
		if (lane < d) {
			xl = 0;
			rl = 0;
		}
		unsigned y = 0, nc = 0;
#pragma unroll
		for (int b = 0; b < 16; ++b) {
			const unsigned cb = (unsigned)__builtin_amdgcn_readlane((int)col, b);
			y ^= (0u - ((xl >> b) & 1u)) & cb;
			nc ^= (0u - ((col >> b) & 1u)) & cb;
		}
		if (!reset) {	/* exact for whole lanes; the last, partial lane's end state is not needed */
			x ^= y;
			reset = rl;
		}
		col = nc;
	}
	const unsigned crc_in = __shfl_up(x, 1, K4_NT);	/* state at the lane's first byte */
	const int flag_in = __shfl_up(k4_scan(last, lane, [](int a, int b) { return a > b ? a : b; }), 1, K4_NT);	/* last flag in front of it */
	unsigned counts = 0;
	unsigned mine[K4_ALL_LANE_MAX] = {};	/* the segments that pass and end in this lane's bytes */
	int npass = 0;
	if (lane >= L1) {
		unsigned c = (lane == L1) ? 0xffffu : crc_in;
		int s = (lane == L1 || flag_in < 0) ? m1 : flag_in + 1;
		for (int q = b0; q < c1; ++q) {
			const unsigned v = B[q];
			if (v == 0x7eu && !(RAW && ((data7e >> (q - c0)) & 1u))) {
				const int l = q - s + 2;
				if (l >= 13 && c == 0xf0b8u) {
					const unsigned w = (unsigned)q << 16 | (unsigned)s;
#pragma unroll
					for (int k = 0; k < K4_ALL_LANE_MAX; ++k)
						mine[k] = npass == k ? w : mine[k];
					++npass;
				}
				if (REP)
					counts += 1u + (l < 13 ? 1u << 16 : 0u);
				c = 0xffffu;
				s = q + 1;
			} else
				c = (c >> 8) ^ sh.crc_tab[(c ^ v) & 0xffu];
		}
	}
	const int upto = k4_scan(npass, lane, [](int a, int b) { return a + b; });	/* passing segments up to and with this lane's */
#pragma unroll
	for (int k = 0; k < K4_ALL_LANE_MAX; ++k)
		if (k < npass && upto - npass + k < K4_NCAND)
			sh.ends[upto - npass + k] = (int)mine[k];
	if (lane == K4_NT - 1)
		sh.nfr = upto;
	if (REP) {
		for (int d = 32; d > 0; d >>= 1)
			counts += __shfl_xor(counts, d, K4_NT);
	}
	K4_SYNC();
	return counts;
}

template <bool REP, bool ALL = false, bool RAW = false>
__device__ __forceinline__ unsigned k4_fcs_scan(K4Shared &sh, int m1, int per, int c0, int c1, int lane, const unsigned *marks = nullptr)
{
	static_assert(ALL || !RAW, "VDL2GPU_F_RAW_FLAGS is a mode of VDL2GPU_F_ALL_FRAMES");
	if constexpr (ALL)
		return k4_fcs_scan_all<REP, RAW>(sh, m1, per, c0, c1, lane, marks);
	const uint8_t *B = reinterpret_cast<const uint8_t *>(sh.dst);
	unsigned col = 0;	/* the advance map, one state bit per lane */
	if (lane < 16) {
		col = 1u << lane;
		for (int i = 0; i < per; ++i)
			col = (col >> 8) ^ sh.crc_tab[col & 0xffu];
	}
	const int L1 = m1 / per;	/* lane that holds m1 (per >= 1 since there are more than m1 bytes) */
	unsigned x = 0;	/* FCS over the lane's own bytes, from 0xffff at m1, from zero behind it */
	if (lane >= L1) {
		x = (lane == L1) ? 0xffffu : 0u;
		for (int i = (lane == L1) ? m1 : c0; i < c1; ++i)
			x = (x >> 8) ^ sh.crc_tab[(x ^ B[i]) & 0xffu];
	}
	for (int d = 1; d < K4_NT; d <<= 1) {
		unsigned xl = __shfl_up(x, d, K4_NT);
		if (lane < d)
			xl = 0;
		unsigned y = 0, nc = 0;
#pragma unroll
		for (int b = 0; b < 16; ++b) {
			const unsigned cb = (unsigned)__builtin_amdgcn_readlane((int)col, b);
			y ^= (0u - ((xl >> b) & 1u)) & cb;
			nc ^= (0u - ((col >> b) & 1u)) & cb;
		}
		x ^= y;	/* exact for whole lanes; the last, partial lane's end state is not needed */
		col = nc;
	}
	const unsigned crc_in = __shfl_up(x, 1, K4_NT);	/* state at the lane's first byte */
	if (lane == 0)
		sh.nfr = 0;
	K4_SYNC();
	unsigned counts = 0;
	if (lane >= L1) {
		unsigned c = (lane == L1) ? 0xffffu : crc_in;
		for (int q = (lane == L1) ? m1 : c0; q < c1; ++q) {
			const unsigned v = B[q];
			if (v == 0x7eu && (q - m1 + 2) >= 13 && c == 0xf0b8u) {
				const int k = atomicAdd(&sh.nfr, 1);
				if (k < K4_NCAND)
					sh.ends[k] = q;
			}
			if (REP && v == 0x7eu)
				counts += 1u + ((q - m1 + 2) < 13 ? 1u << 16 : 0u);
			c = (c >> 8) ^ sh.crc_tab[(c ^ v) & 0xffu];
		}
	}
	if (REP) {
		static_assert(K4_MAXBY < 65536, "two counts to a word, 16 bits each");
		for (int d = 32; d > 0; d >>= 1)
			counts += __shfl_xor(counts, d, K4_NT);
	}
	K4_SYNC();
	return counts;
}

/* ---- frames in stream order (there is almost never more than one); more CRC-clean frames in one burst than the table holds are
 * counted as dropped, not silent */
__device__ __forceinline__ void k4_sort_candidates(K4Shared &sh, unsigned *dropped, int lane)
{
	if (lane == 0) {
		const int nf0 = sh.nfr < K4_NCAND ? sh.nfr : K4_NCAND;
		if (sh.nfr > K4_NCAND)
			atomicAdd(dropped, (unsigned)(sh.nfr - K4_NCAND));
		for (int i = 1; i < nf0; ++i)
			for (int j = i; j > 0 && sh.ends[j] < sh.ends[j - 1]; --j) {
				const int t = sh.ends[j];
				sh.ends[j] = sh.ends[j - 1];
				sh.ends[j - 1] = t;
			}
		sh.nfr = nf0;
	}
	K4_SYNC();
}

/* ---- out() (vdlm2.c:140-158).  One lane asks for the room of a frame that does not go to its record's slot: an arena entry (compact)
 * or the next vdl2gpu_frame_t; nullptr when the buffer is full, and the frame is counted as dropped */
__device__ __forceinline__ vdl2gpu_frame_t *k4_alloc(const K4Params &p, int len)
{
	if (p.compact) {
		const unsigned sz = k4_entry_bytes(len);
		const unsigned base = p.rec_cap * K4_SLOT;
		const unsigned at = base + atomicAdd(&p.nframes->arena_asked, sz);	/* byte offset */
		if (at + sz <= p.frame_cap) {
			atomicAdd(&p.nframes->frames, 1u);
			atomicMax(&p.nframes->arena_end, at + sz - base);	/* the counter never goes back: the entries that found room are a prefix of the arena */
			return reinterpret_cast<vdl2gpu_frame_t *>(reinterpret_cast<char *>(p.frames) + at);
		}
	} else {
		const unsigned at = atomicAdd(&p.nframes->frames, 1u);
		if (at < p.frame_cap)
			return p.frames + at;
	}
	atomicAdd(&p.nframes->dropped, 1u);
	return nullptr;
}

/* the burst's frames: the first one into the record's slot when there is one (myslot) and it fits, the others where k4_alloc says.
 * ALL: a frame starts where its entry in sh.ends says (k4_fcs_scan), not at m1 */
template <bool ALL = false>
__device__ __forceinline__ void k4_emit(K4Shared &sh, const K4Params &p, vdl2gpu_frame_t *myslot, unsigned ib, int m1, int lane)
{
	const vdl2gpu_burst_t *const rec = reinterpret_cast<const vdl2gpu_burst_t *>(sh.recw);
	const uint8_t *B = reinterpret_cast<const uint8_t *>(sh.dst);
	const int nf = sh.nfr;
	for (int f = 0; f < nf; ++f) {
		int start = m1, len = sh.ends[f] - m1 + 2;
		if constexpr (ALL) {
			start = sh.ends[f] & 0xffff;
			len = (sh.ends[f] >> 16) - start + 2;
		}
		const bool inslot = myslot && f == 0 && k4_fits_slot(len);	/* uniform */
		if (!inslot) {
			if (lane == 0)
				sh.room = k4_alloc(p, len);
			K4_SYNC();
		}
		vdl2gpu_frame_t *const fr = inslot ? myslot : sh.room;
		if (fr) {
			if (lane == 0) {
				fr->stream = rec->stream;
				fr->chn = rec->chn;
				fr->Fr = rec->Fr;
				fr->nbrow = rec->nbrow;
				fr->nlbyte = rec->nlbyte;
				fr->len = len;
				fr->block = (int32_t)ib;
				fr->seq = f;
				fr->df = rec->df;
				fr->ppm = rec->ppm;
				fr->trig_dec = rec->trig_dec;
				fr->end_dec = rec->end_dec;
				fr->data[0] = 0x7e;
			}
			for (int i = lane; i < len - 1 && i + 1 < VDL2GPU_MAXFRAME; i += K4_NT)
				fr->data[i + 1] = B[start + i];
		}
		K4_SYNC();
	}
	K4_SYNC();
}

/* REP: the record's report goes together in LDS (K4Rep: zeroed, then every step adds what it knows) and leaves as twelve words from
 * twelve lanes on every way out of the loop body but a void record's, which the host drops. */
union K4Rep {
	vdl2gpu_blockrep_t r;
	unsigned w[sizeof(vdl2gpu_blockrep_t) / 4];
};
static_assert(sizeof(vdl2gpu_blockrep_t) == 48 && alignof(vdl2gpu_blockrep_t) == 4, "the report is written as twelve words");

__device__ __forceinline__ void k4_rep_store(const K4Rep &rp, vdl2gpu_blockrep_t *g, int lane)
{
	K4_SYNC();
	if (lane < (int)(sizeof(vdl2gpu_blockrep_t) / 4))
		reinterpret_cast<unsigned *>(g)[lane] = rp.w[lane];
}

/* ---- TRK: attempt B's rows (vdl2gpu.h, vdl2gpu_trk_t).  The rows in sh.recw are what attempt A's row rule left.  Row by row the
 * record's tracked row goes to `trial` (sh.dst: dead between the attempts, the un-stuffer clears it), rs() runs on it with the row's fixed
 * erasures, and if that returns >= 0 and leaves all six syndromes zero the row is taken.  REP: rep (in LDS, attempt A's report) gets
 * VDL2GPU_ROW_TRACKED and row_changed against the RECEIVED row, which is read again from the record in memory (grec); the three sums
 * are formed again from the rows' entries.  With a row taken sh.src is built again.  Returns the number of rows taken. */
template <bool REP>
__device__ __forceinline__ int k4_trk_rows(K4Shared &sh, const vdl2gpu_burst_t *grec, const vdl2gpu_trk_t *trk, int nbrow, int nlbyte,
					   const unsigned (&sexp)[4][2], int lane, vdl2gpu_blockrep_t *rep)
{
	uint8_t *const rows = reinterpret_cast<uint8_t *>(sh.recw) + offsetof(vdl2gpu_burst_t, data);
	uint8_t *const trial = reinterpret_cast<uint8_t *>(sh.dst);
	int taken = 0;
	for (int r = 0; r < nbrow; ++r) {
		const int by = r == nbrow - 1 ? nlbyte : 249;
		const int nera = k4_set_eras(sh, by, lane);
		for (int i = lane; i < 255; i += K4_NT)
			trial[i] = trk->data[r][i];
		K4_SYNC();
		bool ok = k4_rs_row(sh, trial, nera, sexp, lane);
		if (ok) {
			unsigned syn[6];
			const unsigned any = k4_syndromes(sh, trial, sexp, syn, lane);
			K4_SYNC();
			ok = !any;
		}
		if (!ok)	/* (wave-uniform) */
			continue;
		++taken;
		uint8_t *const row = rows + r * VDL2GPU_ROWLEN;
		for (int i = lane; i < 255; i += K4_NT)
			row[i] = trial[i];
		K4_SYNC();
		if constexpr (REP) {
			const BurstGeom g = burst_geom(nbrow, nlbyte);
			const int pr = r < g.nf_rows - 1 ? 6 : (r == g.nf_rows - 1 ? g.nf_last : 0);	/* the transmitted parity of row r */
			unsigned nch = 0;
#pragma unroll
			for (int b = 0; b < 4; ++b) {
				const int j = lane * 4 + b;
				const bool sent = j < by || (j >= 249 && j < 249 + pr);
				nch += (unsigned)__popcll(__ballot(sent && row[j < 255 ? j : 254] != grec->data[r][j < 255 ? j : 254]));
			}
			if (lane == 0) {
				rep->row_how[r] = VDL2GPU_ROW_TRACKED;
				rep->row_changed[r] = (uint8_t)nch;
			}
		}
	}
	if (taken) {
		int nby = 0;
		for (int r = 0; r < nbrow; ++r) {
			const int by = r == nbrow - 1 ? nlbyte : 249;
			for (int i = lane; i < by; i += K4_NT)
				sh.src[nby + i] = rows[r * VDL2GPU_ROWLEN + i];
			nby += by;
		}
		if (REP && lane == 0) {
			unsigned changed = 0, failed = 0, rescued = 0;
			for (int r = 0; r < nbrow; ++r) {
				const unsigned how = rep->row_how[r];
				changed += rep->row_changed[r];
				failed += how == VDL2GPU_ROW_FAIL;
				rescued += how == VDL2GPU_ROW_SOFT2 || how == VDL2GPU_ROW_SOFT4 || how == VDL2GPU_ROW_FEEDBACK || how == VDL2GPU_ROW_TRACKED;
			}
			rep->bytes_changed = (uint16_t)changed;
			rep->rows_failed = (uint16_t)failed;
			rep->rows_rescued = (uint16_t)rescued;
		}
	}
	K4_SYNC();
	return taken;
}

/* TRK: an attempt has passed no candidate -- is there another one to make?  Behind attempt A (second == false): yes if the record has
 * tracked rows and k4_trk_rows takes one; attempt A's report is kept in rpa first.  Behind attempt B: no, and A's report comes back. */
template <bool REP>
__device__ __forceinline__ bool k4_trk_second(K4Shared &sh, const K4Params &p, unsigned ib, K4Rep &rp, K4Rep &rpa, int nbrow, int nlbyte,
					      const unsigned (&sexp)[4][2], int lane, bool second)
{
	if (second || !p.trk) {
		if (REP && second) {
			K4_SYNC();
			if (lane < (int)(sizeof(vdl2gpu_blockrep_t) / 4))
				rp.w[lane] = rpa.w[lane];
			K4_SYNC();
		}
		return false;
	}
	if constexpr (REP) {
		K4_SYNC();
		if (lane < (int)(sizeof(vdl2gpu_blockrep_t) / 4))
			rpa.w[lane] = rp.w[lane];
		K4_SYNC();
	}
	return k4_trk_rows<REP>(sh, p.recs + ib, p.trk + ib, nbrow, nlbyte, sexp, lane, &rp.r) > 0;
}

/* FB: p.fb holds the records' decision-feedback rows for the row rule of vdl2gpu_fb_t */
/* ALL: every segment between flags is a candidate frame (VDL2GPU_F_ALL_FRAMES), see k4_fcs_scan */
/* RAW: ... and a flag is six adjacent ones of the stuffed stream (VDL2GPU_F_RAW_FLAGS), see k4_unstuff */
/* TRK: p.trk holds the records' timing-tracked rows: a burst of which the steps behind k4_rs_rows pass no candidate goes through them a
 * second time with the rows k4_trk_rows takes (vdl2gpu.h, vdl2gpu_trk_t: attempts A and B).  Without TRK the loop below runs once */
template <bool REP, bool FB = false, bool ALL = false, bool RAW = false, bool TRK = false>
__device__ __forceinline__ void k4_frames_body(const K4Params &p)
{
	__shared__ K4Shared sh;
	__shared__ K4Rep rp;	/* (REP; never touched without it) */
	__shared__ K4Rep rpa;	/* (REP and TRK: attempt A's report while attempt B is under way) */
	unsigned *const marks = RAW ? reinterpret_cast<unsigned *>(sh.save) : nullptr;	/* (behind k4_rs_rows: see k4_unstuff) */
	const int lane = threadIdx.x;
	/* Everything the first record needs from memory is asked for at once -- the tables, the record
	 * count and the front of record blockIdx.x -- because this kernel runs beside the next push's
	 * channeliser, which keeps the memory queues full: every dependent round trip costs microseconds. */
	unsigned tw[K4_TABL], rw[K4_RECW0 / K4_NT] = {};
	k4_fetch_tables(p.tabs, tw, lane);
	if (blockIdx.x < p.rec_cap)
		k4_fetch_head(p.recs + blockIdx.x, rw, lane);
	unsigned nrecs = p.nrecs_dev ? *p.nrecs_dev : p.nrecs;
	nrecs = nrecs > p.rec_cap ? p.rec_cap : nrecs;
	if (blockIdx.x >= nrecs)
		return;
	k4_store_tables(sh, tw, lane);
	const vdl2gpu_burst_t *const rec = reinterpret_cast<const vdl2gpu_burst_t *>(sh.recw);	/* the copy in LDS */
	unsigned sexp[4][2];
	k4_sexp_init(sexp, lane);
	for (unsigned ib = blockIdx.x; ib < nrecs; ib += gridDim.x) {
		if (ib != blockIdx.x) {
			K4_SYNC();	/* the previous record's frame bytes have been read */
			k4_fetch_head(p.recs + ib, rw, lane);
		}
#pragma unroll
		for (int k = 0; k < K4_RECW0 / K4_NT; ++k)
			reinterpret_cast<unsigned *>(sh.recw)[lane + K4_NT * k] = rw[k];
		K4_SYNC();
		const int nbrow = rec->nbrow, nlbyte = rec->nlbyte;
		vdl2gpu_frame_t *const myslot = p.compact ? reinterpret_cast<vdl2gpu_frame_t *>(reinterpret_cast<char *>(p.frames) + (size_t)ib * K4_SLOT) : nullptr;
		if (myslot && lane == 0)
			myslot->len = 0;
		if (p.fmask && rec->trig_sample == REC_VOID)	/* (device-side tag) a burst of the first selection that a repair round made void: K2d's second pass says so */
			continue;
		const bool badhead = nbrow < 1 || nbrow > VDL2GPU_MAXROWS || nlbyte < 0 || nlbyte > 249;
		if constexpr (REP) {
			if (lane < (int)(sizeof(vdl2gpu_blockrep_t) / 4))
				rp.w[lane] = 0u;
			K4_SYNC();
			if (badhead) {
				if (lane == 0)
					rp.r.status = 1;
				k4_rep_store(rp, p.rep + ib, lane);
			}
		}
		if (badhead)
			continue;
		k4_fetch_rows(sh, p.recs + ib, nbrow, lane);
		const int nby = k4_rs_rows<REP, FB>(sh, p.soft ? p.soft + ib : nullptr, nbrow, nlbyte, sexp, lane, &rp.r, FB ? p.fb + ib : nullptr);
		bool second = false, again;	/* (TRK) attempt B is under way; another attempt follows */
		do {
			again = false;
			const int nbits = k4_unstuff<RAW>(sh, nby, lane, marks);
			const int nb = nbits >> 3;	/* whole un-stuffed bytes */
			int c0, c1;	/* of them, the lane's */
			const int per = k4_lane_span(nb, lane, &c0, &c1);
			const int m1 = k4_flag_hunt<RAW>(sh, c0, c1, lane, marks);
			if (REP && lane == 0) {
				rp.r.stuffed = (uint16_t)(8 * nby - nbits);
				rp.r.nbytes = (uint16_t)nb;
				rp.r.flag_at = (int16_t)(sh.flag0 == K4_NONE ? -1 : sh.flag0);
			}
			if (m1 == K4_NONE) {
				if constexpr (TRK) {
					if (k4_trk_second<REP>(sh, p, ib, rp, rpa, nbrow, nlbyte, sexp, lane, second)) {
						second = again = true;
						continue;
					}
				}
				if constexpr (REP)
					k4_rep_store(rp, p.rep + ib, lane);
				K4_SYNC();
				continue;
			}
			const unsigned counts = k4_fcs_scan<REP, ALL, RAW>(sh, m1, per, c0, c1, lane, marks);
			if (REP && lane == 0) {
				const unsigned cand = counts & 0xffffu, too_short = counts >> 16, frames = (unsigned)sh.nfr;	/* (nfr: before k4_sort_candidates caps it) */
				rp.r.cand = (uint16_t)cand;
				rp.r.too_short = (uint16_t)too_short;
				rp.r.bad_fcs = (uint16_t)(cand - too_short - frames);	/* every 0x7e behind hdata[1] is one of the three */
				rp.r.frames = (uint16_t)frames;
			}
			if constexpr (TRK) {
				if (sh.nfr == 0 && k4_trk_second<REP>(sh, p, ib, rp, rpa, nbrow, nlbyte, sexp, lane, second)) {
					second = again = true;
					continue;
				}
			}
			k4_sort_candidates(sh, &p.nframes->dropped, lane);
			k4_emit<ALL>(sh, p, myslot, ib, m1, lane);
			if constexpr (REP)
				k4_rep_store(rp, p.rep + ib, lane);
		} while (TRK && again);
	}
}

#ifndef VDL2GPU_BLOCKS_DEVICE_ONLY
__global__ __launch_bounds__(K4_NT)
void k4_frames(K4Params p)
{
	k4_frames_body<false>(p);
}

/* VDL2GPU_F_BLOCK_REPORT and vdl2gpu_decode_blocks_report: the same block path, and p.rep[i] for every record i that is not void */
__global__ __launch_bounds__(K4_NT)
void k4_frames_rep(K4Params p)
{
	k4_frames_body<true>(p);
}

/* VDL2GPU_F_FEEDBACK and vdl2gpu_decode_blocks_feedback: the same two with the records' feedback rows (p.fb) in the row rule */
__global__ __launch_bounds__(K4_NT)
void k4_frames_fb(K4Params p)
{
	k4_frames_body<false, true>(p);
}

__global__ __launch_bounds__(K4_NT)
void k4_frames_rep_fb(K4Params p)
{
	k4_frames_body<true, true>(p);
}

/* vdl2gpu_debug_rs: k4_rs_row as k4_frames calls it, one wavefront per row, so that a test can hold what it leaves in a row --
 * repaired, miscorrected, given up half way -- against rs() itself.  ret: -1, or the number of roots (0: zero syndromes, eras untouched);
 * eras[0..ret) are written back on success like the reference's eras_pos[]. */
__global__ __launch_bounds__(K4_NT)
void k4_rs_debug(uint8_t *rows, int *eras, const int *no_eras, int *ret, const unsigned *tabs, unsigned n)
{
	__shared__ K4Shared sh;
	const int lane = threadIdx.x;
	const unsigned ib = blockIdx.x;
	if (ib >= n)
		return;
	unsigned tw[K4_TABL];
	k4_fetch_tables(tabs, tw, lane);
	k4_store_tables(sh, tw, lane);
	unsigned sexp[4][2];
	k4_sexp_init(sexp, lane);
	uint8_t *const row = sh.src;
	uint8_t *const grow = rows + (size_t)ib * 255;
	for (int i = lane; i < 255; i += K4_NT)
		row[i] = grow[i];
	if (lane < 6)
		sh.eras[lane] = eras[(size_t)ib * 6 + lane];
	if (lane == 0)
		sh.rs_count = 0;	/* zero syndromes: k4_rs_row returns before anything sets it */
	K4_SYNC();
	const bool ok = k4_rs_row(sh, row, no_eras[ib], sexp, lane);
	const int count = ok ? sh.rs_count : -1;
	for (int i = lane; i < 255; i += K4_NT)
		grow[i] = row[i];
	if (lane < count)
		eras[(size_t)ib * 6 + lane] = sh.eras[lane];
	if (lane == 0)
		ret[ib] = count;
}

/* VDL2GPU_F_ALL_FRAMES and vdl2gpu_decode_blocks_ex with VDL2GPU_BLK_ALL_FRAMES: the four kernels above with ALL, defined in
 * vdl2gpu_allframes.hip (a translation unit of their own, so that this one compiles to what it was without them) */
__global__ void k4_frames_all(K4Params p);
__global__ void k4_frames_all_rep(K4Params p);
__global__ void k4_frames_all_fb(K4Params p);
__global__ void k4_frames_all_rep_fb(K4Params p);
/* VDL2GPU_F_RAW_FLAGS and VDL2GPU_BLK_RAW_FLAGS: those four with RAW, defined in vdl2gpu_rawflags.hip for the same reason */
__global__ void k4_frames_raw(K4Params p);
__global__ void k4_frames_raw_rep(K4Params p);
__global__ void k4_frames_raw_fb(K4Params p);
__global__ void k4_frames_raw_rep_fb(K4Params p);
#endif	/* VDL2GPU_BLOCKS_DEVICE_ONLY */

#endif
