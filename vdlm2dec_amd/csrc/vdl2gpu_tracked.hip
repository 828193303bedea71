/*
 * vdl2gpu_tracked.hip -- VDL2GPU_F_TRACKED (include/vdl2gpu.h, vdl2gpu_trk_t): a burst's payload sliced a second time with a sampling
 * instant that may move by a quarter sample from one segment of 256 symbols to the next (k_tracked_rows), the column's export to the
 * slab (k_export_tracked), and the block path's kernels that make a second attempt with those rows (k4_frames_body with TRK).
 *
 * A translation unit of its own, compiled by its own hipcc -c and linked into libvdl2gpu.so, for the reason vdl2gpu_symclk.hip is
 * one: the kernels of vdl2gpu.hip keep their registers and the record of them its set of names; these are recorded in
 * kernel_resources_tracked.txt.  The filter, the slicer and the soft-bit look-up are those of vdl2gpu_dsp.h, so that a phase is the
 * payload decode's bit for bit; the constant tables they read are compiled into this unit once more (vdl2_tables.inc, internal
 * linkage: those of vdl2gpu.hip are untouched).
 */
#define VDL2GPU_TYPES_NO_TABLES
#define VDL2GPU_BLOCKS_DEVICE_ONLY
#include "vdl2gpu_types.h"
#include "vdl2gpu_geom.h"
/* (the RS steps of vdl2gpu_blocks.h are plain functions that the compiler inlines into each of their two callers elsewhere; with the
 * second attempt as a third caller it stops, and the calls cost the kernels with feedback rows 56 bytes of scratch a lane: in this
 * unit they are inlined by attribute) */
#pragma clang attribute push(__attribute__((always_inline)), apply_to = function)
#include "vdl2gpu_blocks.h"
#pragma clang attribute pop
#include "vdl2gpu_tracked.h"

#define VDL2_TABLE_BEGIN(name, n) static __constant__ uint32_t c_##name[n] = {
#define VDL2_F32(x) x,
#define VDL2_TABLE_END };
#include "vdl2_tables.inc"
#undef VDL2_TABLE_BEGIN
#undef VDL2_F32
#undef VDL2_TABLE_END
#include "vdl2gpu_dsp.h"

/* ------------------------------------------------------------ the tracked slice */

/* A segment's symbols are slots 1 .. 256 of its span, slot 0 the symbol in front of the segment (the differential slice of the
 * segment's first symbol takes both phases with the segment's own d).  A slot's window is KTR_WIN samples: the 17 of a filter pass and
 * one more, because the stream times ceil((4 t + d) / 4) of a segment's candidates d are one sample apart at most.  Window of slot j
 * begins at sample 8 j of the span. */
#define KTR_WIN 18
#define KTR_SPAN (8 * KTR_NT + KTR_WIN)
#define KTR_MAXC 4	/* candidates of a segment: four in segment 0, three behind it */
/* where sample i of the span lies in LDS: the padding of k_symclk_sums (a word behind every 8 samples: the lanes' windows begin 18 banks
 * apart, and the 32 lanes of a ds_read_b64 pass take 32 different pairs of banks) */
__device__ __forceinline__ constexpr int ktr_at(int i) { return i + (i >> 3); }
__device__ __forceinline__ constexpr int ktr_ceil4(int d) { return (d + 3) >> 2; }	/* ceil(d / 4), d of either sign */

struct KtrShared {
	union {
		float2 sx[ktr_at(KTR_SPAN - 1) + 1];	/* a segment's span of the plane */
		struct {				/* ... and, once every lane holds its window, */
			float ph[KTR_MAXC][KTR_NT];	/* the candidates' phases by symbol */
			unsigned short ci[KTR_MAXC][KTR_NT];	/* and their table indices by symbol */
		};
		unsigned long long rows[sizeof(vdl2gpu_trk_t) / 8];	/* behind the last segment: the entry as it goes out */
	};
	unsigned short idx[VDL2GPU_TRK_SEGS * VDL2GPU_TRK_SEG];	/* the winners' table indices (0 .. 256) by symbol */
	float smf[72];					/* mflt[], zero padded, and the atanf range table: what k2_fir_phase_tab reads */
	float atab[VDL2_ATAN_ROWS * VDL2_ATAN_STRIDE];
	int part[KTR_NT / 64][KTR_MAXC];		/* the wavefronts' sums of e^2 */
	float ph0[KTR_MAXC];				/* the candidates' phases of slot 0 (outside the union: written while the span is still read) */
};

/* candidate j of segment s whose predecessor chose d: segment 0 tries 0, -1, -2, -3, a later one d, d - 1, d + 1 */
__device__ __forceinline__ int ktr_cand(int s, int d, int j) { return s ? (j == 0 ? d : (j == 1 ? d - 1 : d + 1)) : -j; }

/* One workgroup per record, KTR_NT lanes.  Segment by segment, in order (d_s starts from d_{s-1}):
 *   1. the span of the channel's plane goes to LDS: zeros for stream times past end_dec (the definition) and for what a lane without a
 *      symbol would read; nothing outside the push's frames is read;
 *   2. lane 0 forms the candidates' phases of slot 0 from its window in registers; then lane l takes the window of slot l + 1, behind a
 *      barrier the span is dead, and the phase of every candidate from those registers goes to LDS where the span was;
 *   3. lane l slices its symbol against slot l under every candidate (k2_grey_index) and the integer costs are added up: xor butterfly
 *      within each wavefront, then the four partial sums by every lane -- integers, no order to state;
 *   4. the winner (every lane finds the same one) leaves its indices in LDS, two bytes each.
 * Behind the last segment one lane per transmitted byte builds it from the Grey tables and the scrambler and scatters it into the entry
 * in LDS, and the entry goes out whole: 256 stores of 8 bytes, zeros and the trailer included.
 * Every test on a record is block-uniform (its fields are), so the barriers are. */
__global__ __launch_bounds__(KTR_NT)
void k_tracked_rows(KTrackedParams p)
{
	static_assert(KTR_NT == 256 && sizeof(vdl2gpu_trk_t) == 8 * KTR_NT, "four wavefronts; a lane writes one 8-byte word of the entry");
	__shared__ KtrShared sh;
	const int l = (int)threadIdx.x;
	if (l < 72)
		sh.smf[l] = l < 65 ? d_tab(c_mflt, l) : 0.0f;
	if (l < VDL2_ATAN_ROWS * VDL2_ATAN_STRIDE)
		sh.atab[l] = vdl2_atan_tab_entry(l);
	unsigned n = *p.count;
	n = n < p.rec_cap ? n : p.rec_cap;
	for (unsigned r = blockIdx.x; r < n; r += gridDim.x) {
		const vdl2gpu_burst_t *rec = p.recs + r;
		if (rec->trig_sample == REC_VOID)	/* (device-side tag) void: the host drops the record */
			continue;
		const int nbrow = rec->nbrow, nlbyte = rec->nlbyte, stream = rec->stream;
		/* the channel slot, found as k_symclk_sums finds it */
		int sc = -1;
		if (stream >= 0 && stream < p.nstreams && nbrow >= 1 && nbrow <= VDL2GPU_MAXROWS && nlbyte >= 0 && nlbyte <= 249) {
			/* every wavefront asks its lanes 0 .. nbch - 1 for the slots of the stream with the record's (chn, Fr): the one end_sample
			 * names if that is one of them, else the first */
			const int j = l & 63, jj = j < VDL2_CS ? j : 0;
			const ChanCfg c = p.cfg[stream * VDL2_CS + jj];
			const int chn = rec->chn, Fr = rec->Fr;
			const unsigned m = (unsigned)__ballot((j < p.nbch) & (j < VDL2_CS) & (c.chn == chn) & (c.Fr == Fr));
			const long long hint = rec->end_sample - (long long)stream * VDL2_CS;
			if (hint >= 0 && hint < VDL2_CS && ((m >> hint) & 1u))
				sc = stream * VDL2_CS + (int)hint;
			else if (m)
				sc = stream * VDL2_CS + __ffs((int)m) - 1;
		}
		unsigned long long *const outw = reinterpret_cast<unsigned long long *>(p.out + r);
		/* the burst's last symbol as a frame of the plane: from here on every time is such a frame, an int.  (A record's burst lies
		 * in the push's planes; one that does not is none) */
		const long long er = rec->end_dec - p.dec_base;
		if (er < 0 || er >= (1LL << 30))
			sc = -1;
		if (sc < 0) {	/* a record that is none: zeros */
			outw[l] = 0ull;
			continue;
		}
		int nbytes;
		{
			const BurstGeom g = burst_geom(nbrow, nlbyte);
			nbytes = g.ND + g.NF;
		}
		const int nsym = (25 + 8 * nbytes - 1) / 3 - 7;	/* n: the symbols k = 8 .. kmax */
		const int nseg = (nsym + VDL2GPU_TRK_SEG - 1) / VDL2GPU_TRK_SEG;
		const int t7 = (int)er - 8 * nsym;	/* frame of symbol k = 7, slot 0 of segment 0 */
		const float df = rec->df;
		const float2 *x = p.dec + (size_t)sc * p.cap;
		/* the last frame of the plane that counts: the burst's last symbol (past end_dec a sample is 0 by definition), and nothing
		 * outside the push's frames is read */
		const int flast = (int)er < p.frames - 1 ? (int)er : p.frames - 1;
		int d = 0, dmin = 0, dmax = 0, dfirst = 0;
		for (int s = 0; s < nseg; ++s) {
			const int i0 = VDL2GPU_TRK_SEG * s;
			const int cnt = nsym - i0 < VDL2GPU_TRK_SEG ? nsym - i0 : VDL2GPU_TRK_SEG;
			const int ncand = s ? 3 : 4;
			const int mlo = ktr_ceil4(s ? d - 1 : -3);	/* the earliest stream time of the candidates, relative to the symbol's */
			const int f0 = t7 + 8 * i0 + mlo - 16;	/* frame of the span's sample 0 */
			__syncthreads();	/* (the lanes are done with the union and with part; the first time: the tables are there) */
			const int iend = flast - f0 < 8 * cnt + KTR_WIN - 1 ? flast - f0 : 8 * cnt + KTR_WIN - 1;	/* the span's last sample that is read */
			/* (f0 + i < 0 does not occur for a record of the ring: a plane carries VDL2_CARRY_FRAMES = 49152 frames in front of the
			 * push's own, the longest burst is VDL2_LONGEST_BURST = 43592 frames from its trigger to end_dec, its trigger lies in the
			 * push or -- decoded a push late -- in the one before, whose frames the carry holds, and the span begins at most
			 * 8 + 16 + 6 frames in front of the first payload symbol (vdl2gpu_types.h asserts the same room for the levels' wider
			 * window).  The test only keeps a broken invariant from reading outside the plane) */
			for (int i = l; i < KTR_SPAN; i += KTR_NT) {
				float2 v = make_float2(0.0f, 0.0f);
				if (i <= iend && f0 + i >= 0)
					v = x[f0 + i];
				sh.sx[ktr_at(i)] = v;
			}
			__syncthreads();
			/* The candidates for slot 0 (lane 0 alone: the symbol in front of the segment), then for slot l + 1, each time in the order
			 * of their stream times -- d - 1, d, d + 1 behind segment 0 -- so that one filter in the code serves: it reads the window's
			 * first 17 samples, and the window moves up by its one sample when a candidate's stream time is the later one.  Between
			 * the two passes every lane has its window in registers and the span is dead: the phases go where it was.
			 * (k2_fir_phase_tab: the payload decode's arithmetic and result bits) */
			float2 w[KTR_WIN];
			int shifted = 0;
#pragma unroll 1
			for (int jj = 0; jj < 2 * ncand; ++jj) {
				const bool front = jj < ncand;
				if (jj == 0 || jj == ncand) {	/* (uniform) */
					const int at = front ? 0 : 9 * (l + 1);	/* ktr_at(8 slot): slot 0 is the same address in every lane, a broadcast */
#pragma unroll
					for (int t = 0; t < KTR_WIN; ++t)
						w[t] = sh.sx[at + ktr_at(t)];
					shifted = 0;
					if (!front)
						__syncthreads();
				}
				const int o = front ? jj : jj - ncand;
				const int j = s ? (o == 0 ? 1 : (o == 1 ? 0 : 2)) : o;
				const int dj = ktr_cand(s, d, j), mj = ktr_ceil4(dj);
				if (mj - mlo != shifted) {	/* (uniform; 0 -> 1 once at most in a pass) */
#pragma unroll
					for (int t = 0; t < KTR_WIN - 1; ++t)
						w[t] = w[t + 1];
					shifted = 1;
				}
				if (!front)
					sh.ph[j][l] = k2_fir_phase_tab(w, 4 * mj - dj, sh.smf, sh.atab);
				else if (l == 0)
					sh.ph0[j] = k2_fir_phase_tab(w, 4 * mj - dj, sh.smf, sh.atab);
			}
			__syncthreads();
#pragma unroll 1
			for (int j = 0; j < ncand; ++j) {
				const int idx = k2_grey_index(sh.ph[j][l], l ? sh.ph[j][l - 1] : sh.ph0[j], df);
				sh.ci[j][l] = (unsigned short)idx;
				const int e = (idx & 31) - 16;
				int cost = l < cnt ? e * e : 0;
#pragma unroll
				for (int b = 32; b >= 1; b >>= 1)
					cost += __shfl_xor(cost, b, 64);
				if ((l & 63) == 0)
					sh.part[l >> 6][j] = cost;
			}
			__syncthreads();
			int win = 0, best = 0;
#pragma unroll 1
			for (int j = 0; j < ncand; ++j) {
				const int c = sh.part[0][j] + sh.part[1][j] + sh.part[2][j] + sh.part[3][j];
				if (j == 0 || c < best) {	/* a later candidate wins only with a strictly smaller cost */
					best = c;
					win = j;
				}
			}
			d = ktr_cand(s, d, win);
			if (s == 0)
				dfirst = dmin = dmax = d;
			dmin = d < dmin ? d : dmin;
			dmax = d > dmax ? d : dmax;
			if (l < cnt)
				sh.idx[i0 + l] = sh.ci[win][l];
		}
		__syncthreads();	/* (the indices are complete; the union is free) */
		sh.rows[l] = 0ull;
		__syncthreads();
		uint8_t *const rows = reinterpret_cast<uint8_t *>(sh.rows);
		const BurstGeom g = burst_geom(nbrow, nlbyte);
		for (int b = l; b < nbytes; b += KTR_NT) {
			const int q0 = 25 + 8 * b;
			const unsigned pnb = p.pn8[b];
			unsigned byte = 0;
#pragma unroll
			for (int i = 0; i < 8; ++i) {
				const int q = q0 + i, k = q / 3;
				const float v = k2_soft_bit((int)sh.idx[k - 8], q - 3 * k, (int)((pnb >> i) & 1u));
				if ((double)v > 0.5)
					byte |= 1u << i;
			}
			int row, col;
			burst_scatter(g, b, &row, &col);
			rows[row * VDL2GPU_ROWLEN + col] = (uint8_t)byte;
		}
		__syncthreads();
		if (l == 0) {	/* the trailer: d_first, d_last, d_min, d_max, nseg, three zero bytes */
			uint8_t *const t = rows + offsetof(vdl2gpu_trk_t, d_first);
			t[0] = (uint8_t)(int8_t)dfirst;
			t[1] = (uint8_t)(int8_t)d;
			t[2] = (uint8_t)(int8_t)dmin;
			t[3] = (uint8_t)(int8_t)dmax;
			t[4] = (uint8_t)nseg;
		}
		__syncthreads();
		outw[l] = sh.rows[l];
	}
}

/* The column beside the records, device ring -> page-locked slab: all 2048 bytes of every record slot below the count.  One wavefront
 * per record, like k_export_feedback. */
__global__ __launch_bounds__(256)
void k_export_tracked(const unsigned *count, unsigned cap, const vdl2gpu_trk_t *src, vdl2gpu_trk_t *dst)
{
	unsigned n = *count;
	n = n < cap ? n : cap;
	const unsigned lane = threadIdx.x & 63u;
	for (unsigned r = blockIdx.x * 4u + (threadIdx.x >> 6); r < n; r += gridDim.x * 4u)
		for (unsigned i = lane; i < sizeof(vdl2gpu_trk_t) / 8; i += 64u)
			reinterpret_cast<unsigned long long *>(dst + r)[i] = reinterpret_cast<const unsigned long long *>(src + r)[i];
}

/* ------------------------------------------------------------ the block path with the second attempt */
/* k4_frames_body with TRK for every combination a handle or a call can ask for: report x feedback rows x mode */
#define K4_TRK_KERNEL(name, REP, FB, ALL, RAW) \
	__global__ __launch_bounds__(K4_NT) void name(K4Params p) { k4_frames_body<REP, FB, ALL, RAW, true>(p); }
K4_TRK_KERNEL(k4_frames_trk, false, false, false, false)
K4_TRK_KERNEL(k4_frames_trk_rep, true, false, false, false)
K4_TRK_KERNEL(k4_frames_trk_fb, false, true, false, false)
K4_TRK_KERNEL(k4_frames_trk_rep_fb, true, true, false, false)
K4_TRK_KERNEL(k4_frames_trk_all, false, false, true, false)
K4_TRK_KERNEL(k4_frames_trk_all_rep, true, false, true, false)
K4_TRK_KERNEL(k4_frames_trk_all_fb, false, true, true, false)
K4_TRK_KERNEL(k4_frames_trk_all_rep_fb, true, true, true, false)
K4_TRK_KERNEL(k4_frames_trk_raw, false, false, true, true)
K4_TRK_KERNEL(k4_frames_trk_raw_rep, true, false, true, true)
K4_TRK_KERNEL(k4_frames_trk_raw_fb, false, true, true, true)
K4_TRK_KERNEL(k4_frames_trk_raw_rep_fb, true, true, true, true)
#undef K4_TRK_KERNEL

K4Kernel k4_frames_trk_kernel(bool rep, bool fb, uint32_t mode)
{
	static const K4Kernel table[3][2][2] = {
		{ { k4_frames_trk, k4_frames_trk_rep }, { k4_frames_trk_fb, k4_frames_trk_rep_fb } },
		{ { k4_frames_trk_all, k4_frames_trk_all_rep }, { k4_frames_trk_all_fb, k4_frames_trk_all_rep_fb } },
		{ { k4_frames_trk_raw, k4_frames_trk_raw_rep }, { k4_frames_trk_raw_fb, k4_frames_trk_raw_rep_fb } },
	};
	return table[mode & VDL2GPU_BLK_RAW_FLAGS ? 2 : (mode & VDL2GPU_BLK_ALL_FRAMES ? 1 : 0)][fb ? 1 : 0][rep ? 1 : 0];
}
