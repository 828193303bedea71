/* vdl2gpu_k1_pp.inc -- the body of k1_pp, included by vdl2gpu_k1.h once per kernel: into the kernel of a handle without
 * VDL2GPU_F_EXACT_FO with ROT = false and an empty K1Rot r in scope (the text around `if constexpr (ROT)` is then the kernel as
 * it always was, instruction for instruction), and into the rotating kernel with ROT its template parameter and r its
 * second argument.  (As a function shared by the two, the compiler allotted the old kernel other registers; tried again when the
 * profiling build and the ablation switches had gone from k1_fast, with the same outcome.) */
	constexpr int B = K1Fmt<FMT>::BYTES, SPB = K1Fmt<FMT>::SPB;
	constexpr int NPIECE = K1P_CH / SPB;			/* 16-byte pieces per period and chunk */
	constexpr int NPT = (64 * NPIECE + K1P_THREADS - 1) / K1P_THREADS;	/* pieces per thread */
	__shared__ float2 xs[8 + 64 * K1P_XROW + 8];	/* 8 entries of pad on either side: blocks of 8 are read whole */
	__shared__ float2 os[8][8 * K1P_OROW];
	const int tid = threadIdx.x;
	const int lane = tid & 63;
	const int c = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int s = (int)blockIdx.y;
	const int blk = (int)(blockIdx.x / (unsigned)p.nsub), sub = (int)(blockIdx.x % (unsigned)p.nsub);
	const int k0 = sub * p.wpt, k1 = k0 + p.wpt;		/* this task's windows of the period */
	const int pb = blk * 64;				/* its first period, counted from per_lo */
	const int nper = (p.per_n - pb < 64) ? p.per_n - pb : 64;
	const long long fill = VDL2_CARRY_FRAMES;
	const bool active = c < p.nbch;
	const char *raw = (const char *)p.raw + (size_t)s * p.stream_stride + (size_t)p.sbase0 * B;	/* first sample of period per_lo */
	if (p.edge_state && blockIdx.x == 0 && tid < VDL2_CS) {	/* what k1_channelise leaves at a push's two ends (see k1_fast) */
		StreamState *ss = p.ss + s;
		if (tid == 0) {
			ss->last_fill = VDL2_CARRY_FRAMES;
			ss->last_J = p.J;
		}
		ss->acc[p.parity ^ 1][tid] = make_float2(0.0f, 0.0f);	/* the push ends on a window boundary: nothing carried */
	}

	/* loader role: NPT pieces (period lp, piece lj) */
	const char *lptr[NPT];
	int lcol[NPT];
	bool lval[NPT];
#pragma unroll
	for (int j = 0; j < NPT; ++j) {
		const int q = tid + j * K1P_THREADS;
		const int lp = q / NPIECE, lj = q % NPIECE;
		lval[j] = q < 64 * NPIECE;
		const int pp = lp < nper ? lp : nper - 1;	/* lanes beyond the last period re-read it (and store nothing) */
		lptr[j] = raw + ((long long)(pb + pp) * p.per_in - p.d) * B + lj * 16;
		lcol[j] = 8 + (lp < 64 ? lp : 63) * K1P_XROW + lj * SPB;
	}

	int k = k0;
	int i = (k0 == 0) ? 0 : p.wend[k0 - 1] + 1;		/* period-relative sample index */
	int wend = p.wend[k0];
	int nf = wend - i + 1;
	const int i_stop = p.wend[k1 - 1] + 1;
	int wi = (p.ph0 + i) % p.L;
	int slot = 0, kflush = k0;
	v2f acc = {0.0f, 0.0f};
	const float2 *lo = p.lo_ext + ((size_t)s * VDL2_CS + (active ? c : 0)) * p.lo_stride + 8;	/* 8 entries of front pad */
	const unsigned xrow = (unsigned)(size_t)(__attribute__((address_space(3))) const float2 *)&xs[8 + lane * K1P_XROW];
	const int m0 = (i + p.d) / K1P_CH, m1 = (i_stop - 1 + p.d) / K1P_CH;
	float2 *decp = p.dec + ((size_t)s * VDL2_CS + (active ? c : 0)) * p.cap + fill + (p.per_lo + pb) * K1P_PER_OUT;
	/* ROT: window k of the lane's period stands at place ri of its schedule period (a period of 84 outputs is four of those),
	 * whose phase index is rq; the two table entries of a window's rotation are fetched when the window begins */
	const unsigned *rtab = nullptr;
	int ri = 0;
	unsigned rq = 0, rP = 0;
	bool ron = false;
	float2 rh = make_float2(1.0f, 0.0f), rl = rh;
	auto rot_fetch = [&]() {
		const unsigned kx = k1r_add(rq, rtab[ri], r.M);
		rh = r.hi[kx >> 12];
		rl = r.lo[kx & 4095];
	};
	if constexpr (ROT) {
		rtab = r.tab + ((size_t)s * VDL2_CS + (active ? c : 0)) * K1R_TAB;
		const int t = r.i0 + k0;
		ri = t % 21;
		rq = k1r_period(rtab, 4 * (p.per_lo + pb + lane) + t / 21, r);
		rP = rtab[21];
		ron = rtab[23] != 0;
		rot_fetch();
	}

	uint4 rr[NPT];
#pragma unroll
	for (int j = 0; j < NPT; ++j)
		rr[j] = *reinterpret_cast<const uint4 *>(lptr[j] + (long long)m0 * K1P_CH * B);
	for (int m = m0; m <= m1; ++m) {
		__syncthreads();	/* the previous chunk has been read by every wave */
#pragma unroll
		for (int j = 0; j < NPT; ++j)
			if (lval[j]) {
				float2 cv[SPB];
				k1_piece_cvt<FMT>(rr[j], cv);
#pragma unroll
				for (int u = 0; u < SPB; ++u)
					xs[lcol[j] + u] = cv[u];
			}
		if (m < m1) {
#pragma unroll
			for (int j = 0; j < NPT; ++j)
				rr[j] = *reinterpret_cast<const uint4 *>(lptr[j] + (long long)(m + 1) * K1P_CH * B);
		}
		__syncthreads();
		if (!active)
			continue;
		const int cb = m * K1P_CH - p.d;	/* period-relative index of the chunk's first sample */
		const int hi = (i_stop < cb + K1P_CH) ? i_stop : cb + K1P_CH;
		while (i < hi) {
			/* a piece: the samples up to the window's or the chunk's end, as blocks of 8 and a tail */
			const int lim = (hi < wend + 1) ? hi : wend + 1;
			int n = lim - i;
			unsigned xa = xrow + (unsigned)(i - cb) * 8u;
			const float2 *lp = lo + wi;
			i = lim;
			wi += n;
			if (wi >= p.L)
				wi -= p.L;
			for (; n >= 8; n -= 8) {
				v16f w;
				v2f xr[8];
				k1_load_block(w, xr, lp, xa);
				if constexpr (K1_REAL(FMT)) {
#pragma unroll
					for (int u = 0; u < 8; ++u)
						k1_rmac_s(acc, xr[u].x, (v2f){w[2 * u], w[2 * u + 1]});
				} else
					k1_cmac8_s(acc, xr, w);
				lp += 8;
				xa += 64;
			}
			if (n) {
				/* the tail: read the 8 entries that END with it (what lies before is the row's or the table's
				 * front pad or earlier samples) and enter the unrolled sequence n steps before its end */
				v16f w;
				v2f xr[8];
				k1_load_block(w, xr, lp - (8 - n), xa - (unsigned)(8 - n) * 8u);
#define K1_TAIL(u) if constexpr (K1_REAL(FMT)) k1_rmac_s(acc, xr[u].x, (v2f){w[2 * (u)], w[2 * (u) + 1]}); \
		   else k1_cmac_s(acc, xr[u], (v2f){w[2 * (u)], w[2 * (u) + 1]});
				switch (n) {
				case 7: K1_TAIL(1)
				case 6: K1_TAIL(2)
				case 5: K1_TAIL(3)
				case 4: K1_TAIL(4)
				case 3: K1_TAIL(5)
				case 2: K1_TAIL(6)
				default: K1_TAIL(7)
				}
#undef K1_TAIL
			}
			if (i > wend) {
				/* D /= nf (d8psk.c:377); the host says whether this rate's two window lengths are proven (fast_div) */
				const v2f q = k1_div_exact(acc, (float)nf, (nf == p.nf_lo) ? p.rcp_lo : p.rcp_hi, p.fast_div);
				float2 v = make_float2(q.x, q.y);
				if constexpr (ROT)
					if (ron)
						v = k1r_cmul(v, k1r_cmul(rh, rl));
				os[c][slot * K1P_OROW + lane] = v;
				acc = (v2f){0.0f, 0.0f};
				++slot;
				++k;
				if (slot == 8 || k == k1) {
					/* 8 windows x 64 periods -> 64-byte runs of the plane: lane = (period, pair of windows) */
					__builtin_amdgcn_wave_barrier();
#pragma unroll
					for (int it = 0; it < 4; ++it) {
						const int pp = it * 16 + (lane >> 2), q = lane & 3;
						if (pp < nper && 2 * q < slot) {
							const float2 v0 = os[c][(2 * q) * K1P_OROW + pp];
							float2 *dst = decp + (long long)pp * K1P_PER_OUT + kflush + 2 * q;
							if (2 * q + 1 < slot) {
								const float2 v1 = os[c][(2 * q + 1) * K1P_OROW + pp];
								typedef float k1_v4a8 __attribute__((ext_vector_type(4), aligned(8)));
								*reinterpret_cast<k1_v4a8 *>(dst) = (k1_v4a8){v0.x, v0.y, v1.x, v1.y};
							} else
								*dst = v0;
						}
					}
					__builtin_amdgcn_wave_barrier();
					kflush = k;
					slot = 0;
				}
				if (k < k1) {
					const int e = p.wend[k];
					nf = e - wend;
					wend = e;
					if constexpr (ROT) {
						if (++ri == 21) {
							ri = 0;
							rq = k1r_add(rq, rP, r.M);
						}
						rot_fetch();
					}
				}
			}
		}
	}
