/* vdl2gpu_k1.h -- K1: channeliser kernels.  Part of the device side of libvdl2gpu.so; included by vdl2gpu_kernels.h only. */
#ifndef VDL2GPU_K1_H
#define VDL2GPU_K1_H

/* ======================================================================= K1
 * Channeliser: ingest conversion (rtl.c:285-292) + complex mix with the LO
 * table + integrate-and-dump to 84 kS/s (d8psk.c:366-381), all channels of a
 * stream from ONE read of the wideband samples.
 *
 * The dump schedule has a closed form: with c0 = decimator
 * clock at the start of the push, local output j ends at local input
 *     le(j) = ceil(((j+1)*SDRCLK - c0) / 21) - 1
 * so every output window is independent and the whole push is time-parallel.
 * Each lane owns one (output window, channel) and adds its 23/24 (2 MS/s) ..
 * 119/120 (10 MS/s) products in stream order, which keeps the float sum
 * identical to the reference's serial loop.  The window straddling a push
 * boundary continues from the partial sum carried in StreamState.acc.
 */
#define K1_THREADS 256
#define K1_OPB 32		/* outputs per pass (256 threads / 8 channel lanes) */
#define K1_PASSES 8

/* push-relative index of the last input sample of output j of a push that starts at c0 of the 21/SDRCLK clock (the host lays
 * out the kernels' periods with the same function) */
__host__ __device__ __forceinline__ long long k1_win_end(long long j, int sdrclk, int c0)
{
	return ((j + 1) * (long long)sdrclk - c0 + 20) / 21 - 1;
}

/* real input (F32R, S16R): the sample is x + 0i and the mixer is D += x * wf (d8psk.c WITH_AIR), no cross terms */
#define K1_REAL(FMT_) ((FMT_) == VDL2GPU_FMT_F32R || (FMT_) == VDL2GPU_FMT_S16R)

template <int FMT> __device__ __forceinline__ float2 k1_load(const char *raw, long long i)
{
	if (FMT == VDL2GPU_FMT_CU8) {
		const uchar2 b = reinterpret_cast<const uchar2 *>(raw)[i];
		return make_float2((float)b.x - (float)127.37, (float)b.y - (float)127.37);
	} else if (FMT == VDL2GPU_FMT_CS16) {
		const short2 v = reinterpret_cast<const short2 *>(raw)[i];
		return make_float2((float)v.x, (float)v.y);
	} else if (FMT == VDL2GPU_FMT_CF32) {
		return reinterpret_cast<const float2 *>(raw)[i];
	} else if (FMT == VDL2GPU_FMT_CS8) {
		const char2 b = reinterpret_cast<const char2 *>(raw)[i];	/* signed: no offset (the 127.37 is cu8's) */
		return make_float2((float)b.x, (float)b.y);
	} else if (FMT == VDL2GPU_FMT_S16R) {
		return make_float2((float)reinterpret_cast<const short *>(raw)[i], 0.0f);
	} else {
		return make_float2(reinterpret_cast<const float *>(raw)[i], 0.0f);
	}
}

/* ---- VDL2GPU_F_EXACT_FO: the residual oscillator at the dump (K1Rot, include/vdl2gpu.h) ----
 * ROT is a template parameter of the three kernels' bodies; the kernels of a handle without the flag are the <.., false>
 * instantiations under their old names and parameters.  A lane works out the phase index of its first output once (k1r_mod:
 * no 64-bit division) and steps it from output to output by adding a host-made increment and subtracting M once if need be. */

/* x mod M for x < 2^56: the quotient from one double multiplication by rM = RN(1 / M) -- off by one at most, the relative
 * error is a few 2^-53 and the quotient below 2^39 -- the remainder in integers, exact */
__device__ __forceinline__ unsigned k1r_mod(unsigned long long x, unsigned M, double rM)
{
	const unsigned long long q = (unsigned long long)((double)x * rM);
	long long r = (long long)(x - q * M);
	if (r < 0)
		r += M;
	if (r >= (long long)M)
		r -= M;
	return (unsigned)r;
}

__device__ __forceinline__ unsigned k1r_add(unsigned a, unsigned b, unsigned M)	/* a, b < M < 2^31 */
{
	const unsigned t = a + b;
	return t >= M ? t - M : t;
}

/* (xr yr - xi yi, xr yi + xi yr): every product and the sum or difference rounded on its own (-ffp-contract=off) */
__device__ __forceinline__ float2 k1r_cmul(float2 x, float2 y)
{
	const float a = x.x * y.x, b = x.y * y.y, c = x.x * y.y, d = x.y * y.x;
	return make_float2(a - b, c + d);
}

/* D' = D (x) (T_hi[k >> 12] (x) T_lo[k & 4095]) */
__device__ __forceinline__ float2 k1r_rotate(float2 d, unsigned k, const K1Rot &r)
{
	return k1r_cmul(d, k1r_cmul(r.hi[k >> 12], r.lo[k & 4095]));
}

/* phase index of the channel's output 21 ql + i, ql counted from the period of the push's output 0, without its tab[i] */
__device__ __forceinline__ unsigned k1r_period(const unsigned *tab, long long ql, const K1Rot &r)
{
	return k1r_mod((unsigned long long)tab[22] * r.sq0 + (unsigned long long)tab[21] * (unsigned long long)ql, r.M, r.rM);
}

/* GLO (rates off the 25 kHz grid whose LO table does not fit LDS beside the windows: 3072 entries x 8 channels at 15.36 MS/s,
 * 6144 at 30.72): the table stays in global memory -- a few hundred KB per stream, L2-resident -- and LDS holds the windows
 * and a tile of LO values, K1G_T steps of every lane's window at a time.  A wavefront (2 channels x 32 windows) fills its own
 * rows of the tile: 16 consecutive lanes load 16 consecutive table entries of a window's channel (8 bytes a lane, a 128-byte
 * run; the index wraps at L), and every lane then takes its K1G_T values of step t from row t -- the same values in the same
 * order as from the table in LDS, so the sums are the same floats. */
#define K1G_T 16
/* entry (step tt of the tile, lane row): rows rotated by tt, so that the 16 steps a loader writes side by side and the 64 lanes
 * that read one step both spread over the banks */
__device__ __forceinline__ int k1g_slot(int tt, int row)
{
	return tt * K1_THREADS + ((row + tt) & (K1_THREADS - 1));
}

template <int FMT, bool GLO, bool ROT> __device__ __forceinline__ void k1_channelise_body(const K1Params &p, const K1Rot &r)
{
	extern __shared__ float2 k1_smem[];
	float2 *lo_s = k1_smem;					/* [(L+maxwin)][8]; GLO: the tile [K1G_T][256] */
	float2 *xs = k1_smem + (GLO ? (size_t)K1G_T * K1_THREADS : (size_t)(p.L + p.maxwin) * VDL2_CS);	/* [32*maxwin] */
	const int tid = threadIdx.x;
	const int s = (int)blockIdx.y;
	const float2 *lo = p.lo + (size_t)s * VDL2_CS * p.L;
	if (!GLO)
	for (int idx = tid; idx < (p.L + p.maxwin) * VDL2_CS; idx += K1_THREADS) {
		const int n = idx >> 3, c = idx & 7;
		lo_s[idx] = lo[c * p.L + (n % p.L)];
	}
	const char *raw = (const char *)p.raw + (size_t)s * p.stream_stride;
	StreamState *ss = p.ss + s;
	const long long fill = VDL2_CARRY_FRAMES;	/* a push's output always starts at that frame */
	const long long jb = p.jbeg + (long long)blockIdx.x * (K1_OPB * K1_PASSES);
	if (blockIdx.x == 0 && tid == 0 && p.jbeg == 0) {
		ss->last_fill = fill;
		ss->last_J = p.J;
	}
	/* lane = (channel, output): 32 consecutive outputs of one channel per half-wave,
	 * so a plane store is a 256-byte run */
	const int o = tid & 31, c = tid >> 5;
	float2 *dec = p.dec + ((size_t)s * VDL2_CS + c) * p.cap + fill;
	/* ROT: output jb + o stands at place ri of its schedule period, whose phase index is rq; a pass later it is 32 = 21 + 11 on */
	const unsigned *rtab = nullptr;
	int ri = 0;
	unsigned rq = 0, rP = 0;
	bool ron = false;
	if constexpr (ROT) {
		rtab = r.tab + ((size_t)s * VDL2_CS + c) * K1R_TAB;
		const long long t = r.i0 + jb + o;
		ri = (int)(t % 21);
		rq = k1r_period(rtab, t / 21, r);
		rP = rtab[21];
		ron = rtab[23] != 0;
	}
	for (int pass = 0; pass < K1_PASSES; ++pass) {
		const long long jp = jb + (long long)pass * K1_OPB;
		if (jp > p.jend)
			break;
		const long long jhi = (jp + K1_OPB - 1 < p.jend) ? jp + K1_OPB - 1 : p.jend;
		const long long in_lo = (jp == 0) ? 0 : k1_win_end(jp - 1, p.sdrclk, p.c0) + 1;
		const long long in_hi = (jhi == p.J) ? p.N - 1 : k1_win_end(jhi, p.sdrclk, p.c0);
		const int cnt = (int)(in_hi - in_lo + 1);
		__syncthreads();
		if (FMT == VDL2GPU_FMT_CU8 && p.quirk) {
			/* rtl.c:285-292 as written: within every hand-off block of 32768 samples, sample k lands in slot
			 * k + 1, slot 0 stays 0 (BSS) and the block's last sample is lost.  Pushes are whole
			 * blocks in this mode, so the position in the block is the position in the push modulo 32768. */
			for (int i = tid; i < cnt; i += K1_THREADS) {
				const long long gi = in_lo + i;
				xs[i] = (gi & 32767) ? k1_load<FMT>(raw, gi - 1) : make_float2(0.0f, 0.0f);
			}
		} else
		for (int i = tid; i < cnt; i += K1_THREADS)
			xs[i] = k1_load<FMT>(raw, in_lo + i);
		__syncthreads();
		const long long j = jp + o;
		/* (the two branches share their set-up and their mixer loops in text only: with them factored out the compiler allots
		 * the LDS kernels other registers, and those kernels are to stay instruction for instruction what they were) */
		if constexpr (GLO) {
			const bool on = j <= p.jend && c < p.nbch;
			long long a = 0;
			int n = 0;
			if (on) {
				a = (j == 0) ? 0 : k1_win_end(j - 1, p.sdrclk, p.c0) + 1;
				n = (int)(((j == p.J) ? p.N - 1 : k1_win_end(j, p.sdrclk, p.c0)) - a + 1);
			}
			const float2 *xp = xs + (int)(a - in_lo);
			const int w0 = (int)((p.no0 + a) % p.L);	/* table index of the window's first step */
			float dre = 0.0f, dim = 0.0f;
			int nf = n;
			if (on && j == 0) {
				const float2 cy = ss->acc[p.parity][c];
				dre = cy.x;
				dim = cy.y;
				nf += p.nf0;
			}
			const int lane = tid & 63, wrow = tid & ~63;
			for (int t0 = 0; t0 < p.maxwin; t0 += K1G_T) {	/* (uniform: every window is maxwin steps at most) */
				__syncthreads();	/* the previous tile has been read */
#pragma unroll 4
				for (int it = 0; it < K1G_T; ++it) {
					const int e = it * 64 + lane;
					const int rr = e / K1G_T, tt = e % K1G_T;	/* the wavefront's lane rr, step t0 + tt of its window */
					const int rw = __shfl(w0, rr), rn = __shfl(n, rr);
					if (t0 + tt < rn)	/* a true modulo: with a custom SDRCLK a window can be many tables long (L = 128, maxwin = 512) */
						lo_s[k1g_slot(tt, wrow + rr)] = lo[((wrow + rr) >> 5) * p.L + (rw + t0 + tt) % p.L];
				}
				__syncthreads();
				const int te = (n - t0 < K1G_T) ? n - t0 : K1G_T;
				if (K1_REAL(FMT)) {
					for (int t = 0; t < te; ++t) {
						const float x = xp[t0 + t].x;
						const float2 w = lo_s[k1g_slot(t, tid)];
						dre += x * w.x;
						dim += x * w.y;
					}
				} else {
					for (int t = 0; t < te; ++t) {
						const float2 x = xp[t0 + t];
						const float2 w = lo_s[k1g_slot(t, tid)];
						const float pr = x.x * w.x - x.y * w.y;
						const float pi = x.x * w.y + x.y * w.x;
						dre += pr;
						dim += pi;
					}
				}
			}
			if (on) {
				if (j == p.J) {
					ss->acc[p.parity ^ 1][c] = make_float2(dre, dim);
				} else {
					const float fn = (float)nf;
					float2 v = make_float2(dre / fn, dim / fn);
					if constexpr (ROT)
						if (ron)
							v = k1r_rotate(v, k1r_add(rq, rtab[ri], r.M), r);
					dec[j] = v;
				}
			}
		} else
		if (j <= p.jend && c < p.nbch) {
			const long long a = (j == 0) ? 0 : k1_win_end(j - 1, p.sdrclk, p.c0) + 1;
			const long long b = (j == p.J) ? p.N - 1 : k1_win_end(j, p.sdrclk, p.c0);
			const int n = (int)(b - a + 1);
			const float2 *xp = xs + (int)(a - in_lo);
			const float2 *wp = lo_s + (size_t)((p.no0 + a) % p.L) * VDL2_CS + c;
			float dre = 0.0f, dim = 0.0f;
			int nf = n;
			if (j == 0) {
				const float2 cy = ss->acc[p.parity][c];
				dre = cy.x;
				dim = cy.y;
				nf += p.nf0;
			}
			if (K1_REAL(FMT)) {
				for (int t = 0; t < n; ++t) {
					const float x = xp[t].x;
					const float2 w = wp[t * VDL2_CS];
					dre += x * w.x;
					dim += x * w.y;
				}
			} else {
				for (int t = 0; t < n; ++t) {
					const float2 x = xp[t];
					const float2 w = wp[t * VDL2_CS];
					const float pr = x.x * w.x - x.y * w.y;
					const float pi = x.x * w.y + x.y * w.x;
					dre += pr;
					dim += pi;
				}
			}
			if (j == p.J) {
				ss->acc[p.parity ^ 1][c] = make_float2(dre, dim);
			} else {
				const float fn = (float)nf;
				float2 v = make_float2(dre / fn, dim / fn);
				if constexpr (ROT)
					if (ron)
						v = k1r_rotate(v, k1r_add(rq, rtab[ri], r.M), r);
				dec[j] = v;
			}
		}
		if constexpr (ROT) {
			rq = k1r_add(rq, rP, r.M);
			ri += 11;
			if (ri >= 21) {
				ri -= 21;
				rq = k1r_add(rq, rP, r.M);
			}
		}
	}
}

template <int FMT> __global__ __launch_bounds__(K1_THREADS)
void k1_channelise(K1Params p)
{
	k1_channelise_body<FMT, false, false>(p, K1Rot{});
}

/* the variant with the LO table in global memory: the second template parameter, so that the kernels above keep their names */
template <int FMT, bool GLO> __global__ __launch_bounds__(K1_THREADS)
void k1_channelise(K1Params p)
{
	static_assert(GLO, "k1_channelise<FMT> is the kernel with the table in LDS");
	k1_channelise_body<FMT, true, false>(p, K1Rot{});
}

/* VDL2GPU_F_EXACT_FO: either variant with the rotation at its dump (a third template parameter and a second argument) */
template <int FMT, bool GLO, bool ROT> __global__ __launch_bounds__(K1_THREADS)
void k1_channelise(K1Params p, K1Rot r)
{
	static_assert(ROT, "without the rotation the kernels are k1_channelise<FMT> and k1_channelise<FMT, true>");
	k1_channelise_body<FMT, GLO, true>(p, r);
}

/* ---- K1 fast path: whole periods of the schedule, any rate ----------------------------
 * The dump schedule and the LO phase repeat every PER = 4*SDRCLK inputs = 84 outputs (1 ms of air
 * time; 2000 inputs at 2 MS/s, 10000 at 10 MS/s), so 64 consecutive periods are 64 copies of the
 * same program: same window boundaries, same LO value at every step, different samples.  That is
 * the wavefront: LANE = PERIOD, WAVE = CHANNEL, eight waves (the stream's eight channels) to a
 * workgroup that shares the samples.
 *
 *   LO      wave-uniform, so it lives in SGPRs: one s_load_dwordx16 per 8 samples from the
 *           channel's table, and the mixer's packed multiplies take it as their scalar operand.
 *           No LO registers per lane, hence no limit on the window length (119/120 samples at
 *           10 MS/s cost what 23/24 do at 2 MS/s).
 *   x       a workgroup fetches a chunk of 32 samples of each of its 64 periods with ONE 16-byte
 *           load per thread (8 threads cover a period's 128 contiguous bytes), converts once
 *           (rtl.c:287-289 / SURVEY A.1) and parks float2 in LDS, row = period.  The next chunk is
 *           in flight in registers while this one is mixed.  Every lane reads its own row: one
 *           conflict-free ds_read_b64 per sample and wave, nothing to broadcast.
 *   mixer   per sample and channel the reference's eight roundings as four packed-FP32
 *           instructions (k1_cmac_s), accumulated in stream order: bit-identical to d8psk.c:368.
 *   out     a lane finishes a window of ITS period every 23/24 samples; eight of them are parked in
 *           a wave-private LDS tile [window][period] and leave as 64-byte runs of the channel plane
 *           (4 lanes x 16 bytes), instead of 8-byte scattered stores.
 *
 * A workgroup's task is (64 periods) x (a run of `wpt` windows of the period), so that a push is
 * several thousand tasks whatever its length.  All control flow is wave-uniform (scalar branches).
 * Gfx950 issues plain FP32 at 2 cycles and packed FP32 at 4 per wave64, so the mixer costs
 * 16 issue cycles per sample and channel either way: that, not HBM, bounds this kernel
 * (scripts/micro/valu_rate.hip measures 4.6-4.9 cycles per packed op with all SIMDs busy). */
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v16f __attribute__((ext_vector_type(16)));

/* acc += x * w for complex x (VGPR pair), w (SGPR pair) with the reference's operation order
 *   pr = x.re*w.re - x.im*w.im;  pi = x.re*w.im + x.im*w.re;  acc += (pr, pi)
 * as four packed-FP32 VALU ops:
 *   a = (x.re*w.re, x.re*w.im)          v_pk_mul_f32, op_sel picks x.re twice
 *   b = (x.im*(-w.im), x.im*w.re)       v_pk_mul_f32, halves of w swapped, low lane negated
 *   acc += (a + b)                      2 x v_pk_add_f32
 * a.lo + b.lo = x.re*w.re + (-(x.im*w.im)) is bit-identical to the subtraction.  One volatile
 * block: the compiler must not turn the uniform branches around it into selects. */
__device__ __forceinline__ void k1_cmac_s(v2f &acc, v2f x, v2f w)
{
	v2f a, b;
	asm volatile("v_pk_mul_f32 %1, %3, %4 op_sel_hi:[0,1]\n\t"
		     "v_pk_mul_f32 %2, %3, %4 op_sel:[1,1] op_sel_hi:[1,0] neg_lo:[0,1]\n\t"
		     "s_nop 0\n\t"
		     "v_pk_add_f32 %1, %1, %2\n\t"
		     "s_nop 0\n\t"
		     "v_pk_add_f32 %0, %0, %1"
		     : "+v"(acc), "=&v"(a), "=&v"(b)
		     : "v"(x), "s"(w));
}

/* real input (air.c:206-208): D += x * wf is (x*w.re, x*w.im), no cross terms (d8psk.c:368 with a float Cbuff) */
__device__ __forceinline__ void k1_rmac_s(v2f &acc, float x, v2f w)
{
	v2f a;
	asm volatile("v_pk_mul_f32 %1, %2, %3 op_sel_hi:[0,1]\n\t"
		     "s_nop 0\n\t"
		     "v_pk_add_f32 %0, %0, %1"
		     : "+v"(acc), "=&v"(a)
		     : "v"((v2f){x, x}), "s"(w));
}

/* Eight samples in one block, software-pipelined so that no instruction reads what the one before it
 * wrote (gfx950 needs a wait state there for packed FP32, and a wave that spends it on s_nop gives the
 * slot away): A/B = the two products of a sample, T = their sum, S = acc += T, in the order
 *   A0 B0 A1 B1 T0 A2 B2 T1 S0 A3 B3 T2 S1 ... A7 B7 T6 S5 T7 S6 . S7
 * -- the S chain is the reference's accumulation order, sample by sample. */
#define K1_A(t, x, w) "v_pk_mul_f32 " t ", " x ", " w " op_sel_hi:[0,1]\n\t"
#define K1_B(t, x, w) "v_pk_mul_f32 " t ", " x ", " w " op_sel:[1,1] op_sel_hi:[1,0] neg_lo:[0,1]\n\t"
#define K1_T(a, b) "v_pk_add_f32 " a ", " a ", " b "\n\t"
#define K1_S(a) "v_pk_add_f32 %0, %0, " a "\n\t"
__device__ __forceinline__ void k1_cmac8_s(v2f &acc, const v2f (&x)[8], const v16f w)
{
	v2f a0, b0, a1, b1, a2, b2;
	asm volatile(
		K1_A("%1", "%7", "%15") K1_B("%2", "%7", "%15")
		K1_A("%3", "%8", "%16") K1_B("%4", "%8", "%16")
		K1_T("%1", "%2")
		K1_A("%5", "%9", "%17") K1_B("%6", "%9", "%17")
		K1_T("%3", "%4")
		K1_S("%1")
		K1_A("%1", "%10", "%18") K1_B("%2", "%10", "%18")
		K1_T("%5", "%6")
		K1_S("%3")
		K1_A("%3", "%11", "%19") K1_B("%4", "%11", "%19")
		K1_T("%1", "%2")
		K1_S("%5")
		K1_A("%5", "%12", "%20") K1_B("%6", "%12", "%20")
		K1_T("%3", "%4")
		K1_S("%1")
		K1_A("%1", "%13", "%21") K1_B("%2", "%13", "%21")
		K1_T("%5", "%6")
		K1_S("%3")
		K1_A("%3", "%14", "%22") K1_B("%4", "%14", "%22")
		K1_T("%1", "%2")
		K1_S("%5")
		K1_T("%3", "%4")
		K1_S("%1")
		"s_nop 0\n\t"
		K1_S("%3")
		: "+v"(acc), "=&v"(a0), "=&v"(b0), "=&v"(a1), "=&v"(b1), "=&v"(a2), "=&v"(b2)
		: "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(x[4]), "v"(x[5]), "v"(x[6]), "v"(x[7]),
		  "s"((v2f){w[0], w[1]}), "s"((v2f){w[2], w[3]}), "s"((v2f){w[4], w[5]}), "s"((v2f){w[6], w[7]}),
		  "s"((v2f){w[8], w[9]}), "s"((v2f){w[10], w[11]}), "s"((v2f){w[12], w[13]}), "s"((v2f){w[14], w[15]}));
}

/* What a block of 8 samples needs, requested in one go and waited for once: the 8 LO values of the wave's
 * channel (one s_load_dwordx16 into SGPRs) and 8 consecutive float2 of this lane's LDS row -- as eight
 * ds_read_b64: the LDS serves those at 256 bytes a clock, the ds_read2_b64 the compiler would merge them into
 * gets half of that, and at one read per sample and wave the LDS is nearly as busy as the VALU. */
__device__ __forceinline__ void k1_load_block(v16f &w, v2f (&x)[8], const float2 *lo, const unsigned a)
{
	asm volatile("s_load_dwordx16 %8, %10, 0x0\n\t"
		     "ds_read_b64 %0, %9\n\tds_read_b64 %1, %9 offset:8\n\tds_read_b64 %2, %9 offset:16\n\t"
		     "ds_read_b64 %3, %9 offset:24\n\tds_read_b64 %4, %9 offset:32\n\tds_read_b64 %5, %9 offset:40\n\t"
		     "ds_read_b64 %6, %9 offset:48\n\tds_read_b64 %7, %9 offset:56\n\ts_waitcnt lgkmcnt(0)"
		     : "=&v"(x[0]), "=&v"(x[1]), "=&v"(x[2]), "=&v"(x[3]), "=&v"(x[4]), "=&v"(x[5]), "=&v"(x[6]), "=&v"(x[7]), "=&s"(w)
		     : "v"(a), "s"(lo)
		     : "memory");
}

/* D /= nf (d8psk.c:377) in k1_pp and k1_fast, fn = (float)nf and rfn = RN(1 / fn).  q0 = x * rfn, q = fma(fma(-q0, fn, x), rfn, q0)
 * is the correctly rounded quotient for every |x| >= 1e-30 and nf in {23, 24, 59, 60, 71, 72, 119, 120} (exhaustively checked:
 * tests/ctests/div_check.c).  Where any lane of the wavefront holds a smaller |x| (a window of zeros), or the caller's window
 * lengths are not of that set (`proven` false), the wavefront takes the plain IEEE division. */
__device__ __forceinline__ v2f k1_div_exact(v2f acc, float fn, float rfn, bool proven = true)
{
	float qr, qi;
	if (proven && __all(fabsf(acc.x) >= 1e-30f && fabsf(acc.y) >= 1e-30f)) {
		const float q0r = acc.x * rfn, q0i = acc.y * rfn;
		qr = fmaf(fmaf(-q0r, fn, acc.x), rfn, q0r);
		qi = fmaf(fmaf(-q0i, fn, acc.y), rfn, q0i);
	} else {
		qr = acc.x / fn;
		qi = acc.y / fn;
	}
	return (v2f){qr, qi};
}

#define K1P_THREADS 512
#define K1P_CH 32		/* samples of every period per chunk */
#define K1P_XROW (K1P_CH + 1)	/* LDS row of a period: +1 keeps the lanes' reads on distinct banks */
#define K1P_OROW 65
#define K1P_PER_OUT 84

template <int FMT> struct K1Fmt;
template <> struct K1Fmt<VDL2GPU_FMT_CU8> { enum { BYTES = 2, SPB = 8 }; };	/* SPB: samples per 16-byte piece */
template <> struct K1Fmt<VDL2GPU_FMT_CS16> { enum { BYTES = 4, SPB = 4 }; };
template <> struct K1Fmt<VDL2GPU_FMT_CF32> { enum { BYTES = 8, SPB = 2 }; };
template <> struct K1Fmt<VDL2GPU_FMT_F32R> { enum { BYTES = 4, SPB = 4 }; };
template <> struct K1Fmt<VDL2GPU_FMT_CS8> { enum { BYTES = 2, SPB = 8 }; };
template <> struct K1Fmt<VDL2GPU_FMT_S16R> { enum { BYTES = 2, SPB = 8 }; };	/* eight reals to a piece */

/* one 16-byte piece of raw samples -> SPB converted samples */
template <int FMT> __device__ __forceinline__ void k1_piece_cvt(const uint4 v, float2 *out)
{
	const unsigned w[4] = {v.x, v.y, v.z, v.w};
	if constexpr (FMT == VDL2GPU_FMT_CU8) {
#pragma unroll
		for (int u = 0; u < 8; ++u) {
			const unsigned h = (w[u >> 1] >> (16 * (u & 1))) & 0xffffu;
			out[u] = make_float2((float)(h & 0xffu) - (float)127.37, (float)(h >> 8) - (float)127.37);
		}
	} else if constexpr (FMT == VDL2GPU_FMT_CS16) {
#pragma unroll
		for (int u = 0; u < 4; ++u)
			out[u] = make_float2((float)(short)(w[u] & 0xffffu), (float)(short)(w[u] >> 16));
	} else if constexpr (FMT == VDL2GPU_FMT_CF32) {
		out[0] = make_float2(__uint_as_float(w[0]), __uint_as_float(w[1]));
		out[1] = make_float2(__uint_as_float(w[2]), __uint_as_float(w[3]));
	} else if constexpr (FMT == VDL2GPU_FMT_CS8) {
#pragma unroll
		for (int u = 0; u < 8; ++u) {
			const unsigned h = w[u >> 1] >> (16 * (u & 1));
			out[u] = make_float2((float)(signed char)(h & 0xffu), (float)(signed char)((h >> 8) & 0xffu));
		}
	} else if constexpr (FMT == VDL2GPU_FMT_S16R) {
#pragma unroll
		for (int u = 0; u < 8; ++u)
			out[u] = make_float2((float)(short)((w[u >> 1] >> (16 * (u & 1))) & 0xffffu), 0.0f);
	} else {
#pragma unroll
		for (int u = 0; u < 4; ++u)
			out[u] = make_float2(__uint_as_float(w[u]), 0.0f);
	}
}


template <int FMT> __global__ __launch_bounds__(K1P_THREADS, 6)
void k1_pp(K1PParams p)
{
	constexpr bool ROT = false;
	const K1Rot r{};
#include "vdl2gpu_k1_pp.inc"
}

/* VDL2GPU_F_EXACT_FO: the same with the rotation at its dump */
template <int FMT, bool ROT> __global__ __launch_bounds__(K1P_THREADS, 6)
void k1_pp(K1PParams p, K1Rot r)
{
	static_assert(ROT, "without the rotation the kernel is k1_pp<FMT>");
#include "vdl2gpu_k1_pp.inc"
}

/* ---- K1 fast path: SDRINRATE 2 MS/s (SDRCLK 500, LO period 80) ------------------------
 * k1_fast: a workgroup of two wavefronts owns 16 consecutive windows of a superperiod (8000 inputs = 336 outputs) x 8
 * channels for many superperiods, the lane's 23/24 LO values in VGPRs, the samples shared through LDS, one barrier per pair
 * of superperiods.  The kernel is described where it is written: vdl2gpu_k1_fast.inc.  Here: its mixers, its counted
 * loads and stores, its constants.  (The packed complex multiply-add and the A/B/T/S schedule notation: k1_cmac_s and
 * k1_cmac8_s above.) */

/* one sample with its LO value in VGPRs: the 24th of a long window */
__device__ __forceinline__ void k1_cmac1_v(v2f &acc, v2f x, v2f w)
{
	v2f a, b;
	asm volatile(K1_A("%1", "%3", "%4") K1_B("%2", "%3", "%4") "s_nop 0\n\t" K1_T("%1", "%2") "s_nop 0\n\t" K1_S("%1")
		     : "+v"(acc), "=&v"(a), "=&v"(b)
		     : "v"(x), "v"(w));
}
/* four consecutive float2 from LDS at byte offset OFS behind address a, requested and not waited for (the offset is an
 * immediate: as part of the address the compiler keeps one register per block and copy of the slice) */
template <int OFS> __device__ __forceinline__ void k1_lds_issue4(v2f (&x)[4], const unsigned a)
{
	asm volatile("ds_read_b64 %0, %4 offset:%5\n\tds_read_b64 %1, %4 offset:%6\n\tds_read_b64 %2, %4 offset:%7\n\tds_read_b64 %3, %4 offset:%8"
		     : "=&v"(x[0]), "=&v"(x[1]), "=&v"(x[2]), "=&v"(x[3])
		     : "v"(a), "n"(OFS), "n"(OFS + 8), "n"(OFS + 16), "n"(OFS + 24)
		     : "memory");
}
/* Four (three) samples with the LO values in VGPRs and two pairs of temporaries; no instruction reads what the one
 * before it wrote (the packed operations' forwarding hazard), one s_nop where that cannot be arranged. */
__device__ __forceinline__ void k1_cmac4_v(v2f &acc, const v2f (&x)[4], const v2f *w)
{
	v2f a0, b0, a1, b1;
	asm volatile(
		K1_A("%1", "%5", "%9") K1_B("%2", "%5", "%9")
		K1_A("%3", "%6", "%10") K1_B("%4", "%6", "%10")
		K1_T("%1", "%2")
		K1_T("%3", "%4")
		K1_S("%1")
		K1_A("%1", "%7", "%11")
		K1_S("%3")
		K1_B("%2", "%7", "%11")
		K1_A("%3", "%8", "%12") K1_B("%4", "%8", "%12")
		K1_T("%1", "%2")
		K1_T("%3", "%4")
		K1_S("%1")
		"s_nop 0\n\t"
		K1_S("%3")
		: "+v"(acc), "=&v"(a0), "=&v"(b0), "=&v"(a1), "=&v"(b1)
		: "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(x[3]), "v"(w[0]), "v"(w[1]), "v"(w[2]), "v"(w[3]));
}
__device__ __forceinline__ void k1_cmac3_v(v2f &acc, const v2f (&x)[4], const v2f *w)
{
	v2f a0, b0, a1, b1;
	asm volatile(
		K1_A("%1", "%5", "%8") K1_B("%2", "%5", "%8")
		K1_A("%3", "%6", "%9") K1_B("%4", "%6", "%9")
		K1_T("%1", "%2")
		K1_T("%3", "%4")
		K1_S("%1")
		K1_A("%1", "%7", "%10")
		K1_S("%3")
		K1_B("%2", "%7", "%10")
		"s_nop 0\n\t"
		K1_T("%1", "%2")
		"s_nop 0\n\t"
		K1_S("%1")
		: "+v"(acc), "=&v"(a0), "=&v"(b0), "=&v"(a1), "=&v"(b1)
		: "v"(x[0]), "v"(x[1]), "v"(x[2]), "v"(w[0]), "v"(w[1]), "v"(w[2]));
}

#define K1F_THREADS 128		/* two wavefronts: channels 0-3 and 4-7 of the same 16 windows */
#define K1F_WAVES_OF(FMT_) ((FMT_) == VDL2GPU_FMT_CF32 ? 4 : 5)	/* wavefronts per SIMD the kernel is built for: 96 registers (cf32 holds its
								 * raw samples in twice as many: 128, 4 wavefronts) */
#define K1F_DEPTH 2		/* superperiods of raw samples in flight per wavefront (registers) */
#define K1F_CHUNK 8		/* superperiods per ticket (even: the two LDS copies and register sets alternate) */
#define K1F_PER_IN 8000		/* a SUPERPERIOD: 4 periods of the schedule = 336 outputs = 21 lines of 16 */
#define K1F_PER_OUT 336
#define K1F_ROLES 21

/* raw samples as the wave's loads deliver them: one 32-bit register per sample (64 for cf32) */
template <int FMT> struct K1Raw { typedef unsigned T; };
template <> struct K1Raw<VDL2GPU_FMT_CF32> { typedef unsigned T __attribute__((ext_vector_type(2))); };

/* The sample loads are written in assembly because their waits are: a wave keeps DEPTH periods of samples in
 * flight, and before it converts one it must only wait until the loads of THAT period have landed -- memory
 * operations of a wave complete in issue order, so "at most as many outstanding as were issued after them".
 * The compiler, seeing loads in a loop with a conditional body, waits for everything (vmcnt(0)): every period
 * then costs a full memory round trip, store acknowledgement included, and the kernel is latency-bound. */
template <int FMT, int OFS = 0> __device__ __forceinline__ void k1_raw_issue(typename K1Raw<FMT>::T &r, const unsigned voff, const char *sbase)
{
	if constexpr (FMT == VDL2GPU_FMT_CU8 || FMT == VDL2GPU_FMT_CS8)
		asm volatile("global_load_ushort %0, %1, %2 offset:%3" : "=v"(r) : "v"(voff), "s"(sbase), "n"(OFS) : "memory");
	else if constexpr (FMT == VDL2GPU_FMT_S16R)	/* sign-extended by the load: the register is the sample as an int */
		asm volatile("global_load_sshort %0, %1, %2 offset:%3" : "=v"(r) : "v"(voff), "s"(sbase), "n"(OFS) : "memory");
	else if constexpr (FMT == VDL2GPU_FMT_CF32)
		asm volatile("global_load_dwordx2 %0, %1, %2 offset:%3" : "=v"(r) : "v"(voff), "s"(sbase), "n"(OFS) : "memory");
	else
		asm volatile("global_load_dword %0, %1, %2 offset:%3" : "=v"(r) : "v"(voff), "s"(sbase), "n"(OFS) : "memory");
}

template <int FMT> __device__ __forceinline__ float2 k1_raw_cvt(typename K1Raw<FMT>::T v)
{
	if constexpr (FMT == VDL2GPU_FMT_CU8) {
		return make_float2((float)(v & 0xffu) - (float)127.37, (float)((v >> 8) & 0xffu) - (float)127.37);
	} else if constexpr (FMT == VDL2GPU_FMT_CS16) {
		return make_float2((float)(short)(v & 0xffffu), (float)(short)(v >> 16));
	} else if constexpr (FMT == VDL2GPU_FMT_CF32) {
		return make_float2(__uint_as_float(v.x), __uint_as_float(v.y));
	} else if constexpr (FMT == VDL2GPU_FMT_CS8) {
		return make_float2((float)(signed char)(v & 0xffu), (float)(signed char)((v >> 8) & 0xffu));
	} else if constexpr (FMT == VDL2GPU_FMT_S16R) {
		return make_float2((float)(int)v, 0.0f);
	} else {
		return make_float2(__uint_as_float(v), 0.0f);
	}
}

/* One memory instruction that is always ISSUED (k1_fast's waits count it) with only the lanes of a ballot enabled: the asm
 * text of INSN_ between the save of exec and its return.  The block names the ballot as operand [m] and clobbers s2, s3.
 * (k1_store_masked below and k1_fast's ticket request.) */
#define K1_MASKED_ISSUE(INSN_) "s_mov_b64 s[2:3], exec\n\t" "s_mov_b64 exec, %[m]\n\t" INSN_ "\n\t" "s_mov_b64 exec, s[2:3]"

/* a global_store_dwordx2 of the `on` lanes; the address is a workgroup-uniform base (scalar registers) plus the lane's 32-bit
 * byte offset */
__device__ __forceinline__ void k1_store_masked(const float2 *sbase, unsigned voff, v2f v, bool on)
{
	asm volatile(K1_MASKED_ISSUE("global_store_dwordx2 %0, %1, %2")
		     :: "v"(voff), "v"(v), "s"(sbase), [m] "s"(__ballot(on)) : "memory", "s2", "s3");
}

/* VDL2GPU_F_EXACT_FO: one table entry of the rotation, requested and not waited for (the loop counts it among its loads) */
__device__ __forceinline__ void k1r_issue(v2f &v, const unsigned voff, const float2 *sbase)
{
	asm volatile("global_load_dwordx2 %0, %1, %2" : "=v"(v) : "v"(voff), "s"(sbase) : "memory");
}
#define K1F_ROT_WAVES 4		/* wavefronts per SIMD of the rotating instantiations: the phase index and the four table entries in
				 * flight per pair do not fit the 96 registers of five */


template <int FMT> __global__ __launch_bounds__(K1F_THREADS, K1F_WAVES_OF(FMT))
void k1_fast(K1Params p)
{
	constexpr bool ROT = false;
	const K1Rot r{};
#include "vdl2gpu_k1_fast.inc"
}

/* VDL2GPU_F_EXACT_FO: the same with the rotation at its dump */
template <int FMT, bool ROT> __global__ __launch_bounds__(K1F_THREADS, K1F_ROT_WAVES)
void k1_fast(K1Params p, K1Rot r)
{
	static_assert(ROT, "without the rotation the kernel is k1_fast<FMT>");
#include "vdl2gpu_k1_fast.inc"
}

#endif
