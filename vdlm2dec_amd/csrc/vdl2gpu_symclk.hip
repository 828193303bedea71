/*
 * vdl2gpu_symclk.hip -- VDL2GPU_F_SYMCLK (include/vdl2gpu.h, vdl2gpu_symclk_t): every burst's symbol timing, clock drift and fine
 * arrival time.  The two kernels (the sums of the square-law timing estimator, and the column's export to the slab), and the host
 * arithmetic that derives the rest from the sums (vdl2gpu_symclk_from_sums: public, pure, and what collect_records calls).
 *
 * A translation unit of its own, compiled by its own hipcc -c and linked into libvdl2gpu.so, for the reason vdl2gpu_allframes.hip
 * is one: the kernels of vdl2gpu.hip keep their registers and the record of them its set of names; these two are recorded in
 * kernel_resources_symclk.txt.  vdl2gpu.hip launches them through the prototypes of vdl2gpu_symclk.h.
 */
#define VDL2GPU_TYPES_NO_TABLES
#include "vdl2gpu_types.h"
#include "vdl2gpu_geom.h"
#include "vdl2gpu_symclk.h"

#include <cmath>
#include <cstring>

/* ------------------------------------------------------------ device side */

#define KSC_SPAN (8 * KSC_NT + 16)	/* samples a segment touches: from 23 in front of its first symbol to its last symbol */
/* where sample i of the span lies in LDS: a lane's 24 samples begin 8 apart, and 8 float2 are 16 banks -- one word of padding
 * behind every 8 samples makes that 18 (gcd with the 64 banks: 2, so the 32 lanes of a ds_read_b64 pass take 32 different pairs) */
__device__ __forceinline__ constexpr int ksc_at(int i) { return i + (i >> 3); }

/* One workgroup, one segment of one record: KSC_NT lanes, lane l = symbol k = 256 s + l.
 *   1. the span of the channel's plane goes to LDS (zeros where a lane has no symbol; nothing outside the push's frames is read);
 *   2. every lane forms the eight |S(n_k - d, 0)|^2 of its symbol from 24 samples in registers: S in float, taps in ascending
 *      order, multiply then add (-ffp-contract=off), exactly as lev_pow (vdl2gpu_machine.h) forms it;
 *   3. the eight sums in the order include/vdl2gpu.h fixes: xor butterfly 32 .. 1 within each wavefront, then
 *      ((w0 + w1) + w2) + w3 by lane d < 8, which stores e[s][d] (plain vector stores);
 *   4. segment 0's workgroup writes the integer fields and zeros for what the host derives; a workgroup with s >= nseg zeros e[s][].
 * Every test on a record is block-uniform (its fields are), so the barriers are. */
__global__ __launch_bounds__(KSC_NT)
void k_symclk_sums(KSymclkParams p)
{
	static_assert(KSC_NT == 256, "four wavefronts: the order of summation is stated for that");
	__shared__ float2 sx[ksc_at(KSC_SPAN - 1) + 1];
	__shared__ float part[KSC_NT / 64][8];
	const int s = (int)blockIdx.x, l = (int)threadIdx.x;
	unsigned n = *p.count;
	n = n < p.rec_cap ? n : p.rec_cap;
	for (unsigned r = blockIdx.y; r < n; r += gridDim.y) {
		const vdl2gpu_burst_t *rec = p.recs + r;
		if (rec->trig_sample == REC_VOID)	/* (device-side tag) void: the host drops the record */
			continue;
		vdl2gpu_symclk_t *out = p.out + r;
		const int nbrow = rec->nbrow, nlbyte = rec->nlbyte, stream = rec->stream;
		/* the channel slot: K2d leaves it in end_sample, the serial machine leaves 0 there -- so the slot is the one of the record's
		 * stream whose (chn, Fr) are the record's, end_sample's if that is one (channels of a stream that share both are told apart
		 * only then) */
		int sc = -1;
		if (stream >= 0 && stream < p.nstreams && nbrow >= 1 && nbrow <= VDL2GPU_MAXROWS && nlbyte >= 0 && nlbyte <= 249) {
			const long long hint = rec->end_sample;
			const int chn = rec->chn, Fr = rec->Fr;
			if (hint >= (long long)stream * VDL2_CS && hint < (long long)stream * VDL2_CS + p.nbch && p.cfg[hint].chn == chn && p.cfg[hint].Fr == Fr)
				sc = (int)hint;
			else
				for (int j = p.nbch - 1; j >= 0; --j)
					if (p.cfg[stream * VDL2_CS + j].chn == chn && p.cfg[stream * VDL2_CS + j].Fr == Fr)
						sc = stream * VDL2_CS + j;
		}
		const int nsym = sc >= 0 ? burst_geom(nbrow, nlbyte).nsym : 0;
		const int nseg = (nsym + VDL2GPU_SYMCLK_SEG - 1) / VDL2GPU_SYMCLK_SEG;
		const long long first = rec->end_dec - 8LL * (nsym - 1);
		if (s == 0 && l == 0) {
			out->sym_first_dec = nsym ? first : 0;
			out->nsym = nsym;
			out->nseg = nseg;
			out->toa_sample = 0.0;	/* the host derives these four (vdl2gpu_symclk_from_sums) */
			out->tau0 = 0.0f;
			out->clock_ppm = 0.0f;
			out->tau_rms = 0.0f;
			out->reserved = 0;
		}
		if (s >= nseg) {	/* (also a record that is none: nseg = 0) */
			if (l < 8)
				out->e[s][l] = 0.0f;
			continue;
		}
		const int k0 = VDL2GPU_SYMCLK_SEG * s;
		const int cnt = nsym - k0 < VDL2GPU_SYMCLK_SEG ? nsym - k0 : VDL2GPU_SYMCLK_SEG;
		const long long t0 = first + 8LL * k0 - 23 - p.dec_base;	/* frame of the span's sample 0 */
		const float2 *x = p.dec + (size_t)sc * p.cap;
		__syncthreads();	/* (the previous record's lanes are done with sx and part) */
		for (int i = l; i < KSC_SPAN; i += KSC_NT) {
			const long long f = t0 + i;
			float2 v = make_float2(0.0f, 0.0f);
			if (i < 8 * cnt + 16 && f >= 0 && f < p.frames && f < p.cap)
				v = x[f];
			sx[ksc_at(i)] = v;
		}
		__syncthreads();
		float2 w[24];
#pragma unroll
		for (int t = 0; t < 24; ++t)
			w[t] = sx[9 * l + ksc_at(t)];	/* ksc_at(8 l + t) */
		float acc[8];
#pragma unroll
		for (int d = 0; d < 8; ++d) {
			float sr = 0.0f, si = 0.0f;
#pragma unroll
			for (int j = 0; j < KSC_TAPS; ++j) {
				const float2 v = w[7 - d + j];	/* stream time n_k - d - 16 + j */
				const float m = p.taps[j];
				sr += v.x * m;
				si += v.y * m;
			}
			acc[d] = l < cnt ? sr * sr + si * si : 0.0f;
		}
#pragma unroll
		for (int d = 0; d < 8; ++d) {
#pragma unroll
			for (int b = 32; b >= 1; b >>= 1)
				acc[d] += __shfl_xor(acc[d], b, 64);
		}
		if ((l & 63) == 0) {
#pragma unroll
			for (int d = 0; d < 8; ++d)
				part[l >> 6][d] = acc[d];
		}
		__syncthreads();
		if (l < 8)
			out->e[s][l] = ((part[0][l] + part[1][l]) + part[2][l]) + part[3][l];
	}
}

/* The column beside the records, device ring -> page-locked slab: all 744 bytes of every record slot below the count, 93 words of
 * 8 bytes.  One wavefront per record, like k_export_feedback. */
__global__ __launch_bounds__(256)
void k_export_symclk(const unsigned *count, unsigned cap, const vdl2gpu_symclk_t *src, vdl2gpu_symclk_t *dst)
{
	static_assert(sizeof(vdl2gpu_symclk_t) % 8 == 0, "copied as 8-byte words");
	unsigned n = *count;
	n = n < cap ? n : cap;
	const unsigned lane = threadIdx.x & 63u;
	for (unsigned r = blockIdx.x * 4u + (threadIdx.x >> 6); r < n; r += gridDim.x * 4u)
		for (unsigned i = lane; i < sizeof(vdl2gpu_symclk_t) / 8; i += 64u)
			reinterpret_cast<unsigned long long *>(dst + r)[i] = reinterpret_cast<const unsigned long long *>(src + r)[i];
}

/* ------------------------------------------------------------ host side */

namespace {
/* the constant tables once more, as host data (vdl2gpu.hip holds them in constant memory of the device) */
struct HostTables {
#define VDL2_TABLE_BEGIN(name, n) static constexpr uint32_t name[n] = {
#define VDL2_F32(x) x,
#define VDL2_TABLE_END };
#include "vdl2_tables.inc"
#undef VDL2_TABLE_BEGIN
#undef VDL2_F32
#undef VDL2_TABLE_END
};
}

void symclk_taps(float *taps17)
{
	for (int j = 0; j < KSC_TAPS; ++j)
		memcpy(taps17 + j, &HostTables::mflt[4 * j], sizeof(float));
}

/* The derived values of a symbol-clock record (include/vdl2gpu.h, vdl2gpu_symclk_t): the one statement of that arithmetic. */
extern "C" int vdl2gpu_symclk_from_sums(int64_t sym_first_dec, int nsym, const float *e, unsigned sdrinrate, vdl2gpu_symclk_t *out, double *tau_s)
{
	if (!out || !e || nsym <= 0 || nsym > VDL2GPU_SYMCLK_SEG * VDL2GPU_SYMCLK_SEGS || !sdrinrate)
		return VDL2GPU_EINVAL;
	const int nseg = (nsym + VDL2GPU_SYMCLK_SEG - 1) / VDL2GPU_SYMCLK_SEG;
	/* exp(+2 pi i d / 8), d = 0 .. 7, exactly where it is exact */
	static const double cs[8] = { 1.0, M_SQRT1_2, 0.0, -M_SQRT1_2, -1.0, -M_SQRT1_2, 0.0, M_SQRT1_2 };
	static const double sn[8] = { 0.0, M_SQRT1_2, 1.0, M_SQRT1_2, 0.0, -M_SQRT1_2, -1.0, -M_SQRT1_2 };
	double tau[VDL2GPU_SYMCLK_SEGS], c[VDL2GPU_SYMCLK_SEGS], m[VDL2GPU_SYMCLK_SEGS];
	double W = 0.0, Wc = 0.0, Wt = 0.0;
	for (int s = 0; s < nseg; ++s) {
		double zr = 0.0, zi = 0.0;
		for (int d = 0; d < 8; ++d) {
			zr += (double)e[8 * s + d] * cs[d];
			zi += (double)e[8 * s + d] * sn[d];
		}
		double t = -(4.0 / M_PI) * atan2(zi, zr);
		if (t <= -4.0)
			t += 8.0;
		if (s > 0) {
			while (t - tau[s - 1] > 4.0)
				t -= 8.0;
			while (t - tau[s - 1] <= -4.0)
				t += 8.0;
		}
		tau[s] = t;
		const int k0 = VDL2GPU_SYMCLK_SEG * s;
		m[s] = (double)(nsym - k0 < VDL2GPU_SYMCLK_SEG ? nsym - k0 : VDL2GPU_SYMCLK_SEG);
		c[s] = (double)k0 + (m[s] - 1.0) / 2.0;
		W += m[s];
		Wc += m[s] * c[s];
		Wt += m[s] * t;
	}
	double tau0 = tau[0], ppm = NAN, rms = NAN;
	if (nseg > 1) {
		const double mc = Wc / W, mt = Wt / W;
		double Scc = 0.0, Sct = 0.0;
		for (int s = 0; s < nseg; ++s) {
			Scc += m[s] * (c[s] - mc) * (c[s] - mc);
			Sct += m[s] * (c[s] - mc) * (tau[s] - mt);
		}
		const double slope = Sct / Scc;
		tau0 = mt - slope * mc;
		double R = 0.0;
		for (int s = 0; s < nseg; ++s) {
			const double r = tau[s] - (tau0 + slope * c[s]);
			R += m[s] * r * r;
		}
		ppm = -slope / 8.0 * 1e6;
		rms = sqrt(R / W);
	}
	/* D: the centroid delay of the sub-phase-0 taps (tap j weighs the sample 16 - j before the newest) */
	float taps[KSC_TAPS];
	symclk_taps(taps);
	double g = 0.0, gd = 0.0;
	for (int j = 0; j < KSC_TAPS; ++j) {
		g += (double)taps[j];
		gd += (double)(16 - j) * (double)taps[j];
	}
	const double D = gd / g;
	memmove(out->e, e, (size_t)nseg * 8 * sizeof(float));	/* (e may be out->e) */
	memset(&out->e[0][0] + nseg * 8, 0, (size_t)(VDL2GPU_SYMCLK_SEGS - nseg) * 8 * sizeof(float));
	out->sym_first_dec = sym_first_dec;
	out->nsym = nsym;
	out->nseg = nseg;
	out->toa_sample = ((double)sym_first_dec + tau0 - D + 0.5) * (double)sdrinrate / 84000.0 - 0.5;
	out->tau0 = (float)tau0;
	out->clock_ppm = (float)ppm;
	out->tau_rms = (float)rms;
	out->reserved = 0;
	if (tau_s)
		memcpy(tau_s, tau, (size_t)nseg * sizeof(double));
	return VDL2GPU_OK;
}
