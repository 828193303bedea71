/* vdl2gpu_k1_fast.inc -- the body of k1_fast, included by vdl2gpu_k1.h once per kernel: into the kernel of a handle without
 * VDL2GPU_F_EXACT_FO with ROT = false and an empty K1Rot r in scope (the text around `if constexpr (ROT)` is then the kernel as
 * it always was, instruction for instruction), and into the rotating kernel with ROT its template parameter and r its
 * second argument.  (As a function shared by the two, the compiler allotted the old kernel other registers; tried again when the
 * profiling build and the ablation switches had gone from k1_fast, with the same outcome.) */
	typedef typename K1Raw<FMT>::T raw_t;
	constexpr int B = K1Fmt<FMT>::BYTES;
	/* LDS: every window has its own row of 25 float2 (24 samples + 1 of padding: rows of 50 dwords put the 8 windows of
	 * a half-wave read on 8 different bank pairs; laid end to end, windows 4 apart -- 95 or 96 samples -- shared banks),
	 * a pair of slices per iteration, two copies of the pair used in turn (one barrier per iteration) */
	__shared__ float2 xs[2][2][16 * 25 + 8];	/* [copy][half of the pair] */
	__shared__ int s_next;
	const int tid = threadIdx.x;
	const int lane = tid & 63, wv = tid >> 6;
	const int s = (int)blockIdx.y;
	/* A workgroup owns 16 consecutive outputs -- ONE 128-byte line of every channel plane -- of a superperiod (4
	 * periods of the schedule: 8000 inputs, 336 outputs, 21 lines) for many superperiods: lane = (window, channel),
	 * 16 windows x 4 channels to a wavefront, the two wavefronts share the windows' ~381 samples through LDS.  A
	 * wavefront's store is four whole, aligned lines.  (Runs of 64 bytes -- 8 windows per wavefront -- reached HBM as
	 * partial lines once the read stream pushed them out of the L2 before their other halves arrived: the same
	 * traffic moved in 128 us instead of 86, scripts/micro/store_shape.hip.)
	 *
	 * The kernel is built around what a SIMD needs to stay busy: one wavefront issues a packed operation every 9 cycles
	 * at best, four of them together one every 3.5, eight one every 1.5 - 2 (scripts/micro/clock_rate.hip, valu_rate.hip)
	 * -- three to four wavefronts per SIMD must be mixing at any time.  Hence 96 registers (5 wavefronts per SIMD: the
	 * 24 LO values of the lane's window take 48 of them, samples come from LDS four at a time), and a grid that is
	 * resident as a whole (the launch sizes it): a workgroup's start-up -- cold code, LO values, first samples -- is
	 * paid once per ~70 superperiods. */
	/* Work is handed out in TICKETS of K1F_CHUNK superperiods.  Workgroup b runs on XCD x = b % 8 and has role
	 * g = (b / 8) % 21; the workgroups of one (role, XCD) form a family that shares a counter and takes the superperiods
	 * per_lo + x + 8 i, i = 0, 1, .. in chunks: ticket t = i in [t C, t C + C).  The first ticket of a workgroup is its
	 * rank in the family, the next one comes from the counter while the current one is being worked on -- a workgroup on
	 * a SIMD that advances slowly (more wavefronts, a busier CU, another kernel's wavefronts beside it) simply takes
	 * fewer tickets.  With a fixed share each the launch lasted as long as its slowest SIMD: 104 us for wavefronts that
	 * lived 88 us on average.  A family's superperiods are neighbours of the other roles' on the same XCD: at any time the
	 * grid reads one contiguous band of the input and writes one contiguous band of each plane, each L2 its own eighth. */
	const int x = (int)(blockIdx.x & 7);
	const int g = (int)((blockIdx.x >> 3) % K1F_ROLES);
	const int rank = (int)(blockIdx.x / (8 * K1F_ROLES)), nfam = (int)(gridDim.x / (8 * K1F_ROLES));
	const int n_x = ((int)p.per_n - x + 7) >> 3;			/* superperiods of this XCD */
	if (rank * K1F_CHUNK >= n_x)	/* its first ticket is empty */
		return;
	if (p.edge_state && blockIdx.x == 0 && tid < VDL2_CS) {	/* (rank 0 of XCD 0: never empty) what k1_channelise leaves at a push's two ends */
		StreamState *ss = p.ss + s;
		if (tid == 0) {
			ss->last_fill = VDL2_CARRY_FRAMES;
			ss->last_J = p.J;
		}
		ss->acc[p.parity ^ 1][tid] = make_float2(0.0f, 0.0f);	/* the push ends on a window boundary: nothing carried */
	}
	const unsigned *ctr = p.tickets + ((size_t)s * K1F_ROLES + g) * 8 + x;	/* ticket = nfam + (old value - tbase[x]) */
	const unsigned tbase = p.tbase[x];
	const int kk = lane >> 2, c = wv * 4 + (lane & 3);
	const bool active = c < p.nbch;
	const char *raw = (const char *)p.raw + (size_t)s * p.stream_stride;
	/* The schedule repeats exactly every superperiod (336 * SDRCLK = 21 * 8000): window jr of ANY superperiod ends
	 * e(jr) samples behind the superperiod's nominal start pp * 8000, e(jr) = ceil(((jr + 1) * 500 - c0) / 21) - 1
	 * (k1_win_end with the superperiod's 168000 taken out; 21 * 32 keeps the division's numerator positive), and the
	 * sample at `rel` belongs to window ceil((21 (rel + 1) + c0 - 20) / 500) - 1.  Everything in front of the loop is
	 * 32-bit arithmetic on these two, no table and no barrier: every instruction here is executed exactly once and
	 * fetched cold (~330 cycles per 64-byte line of code), so this part is written for size.
	 * The slice of this workgroup: from the first sample of window 16g to the last of window 16g + 15. */
	const int c0 = p.c0;
	auto e_rel = [c0](int jr) { return ((jr + 1) * 500 - c0 + 20 + 21 * 32) / 21 - 32 - 1; };
	const int e0 = e_rel(g * 16 - 1);
	const int slen = e_rel(g * 16 + 15) - e0;
	const int ek = e_rel(g * 16 + kk - 1);
	const int off = ek - e0, nwin = e_rel(g * 16 + kk) - ek;
	/* threads fetch samples tid, tid+128, tid+256 of the slice (clamped: the tail re-reads the last sample) and park
	 * each in the row of the window it belongs to */
	unsigned vo[3];	/* [1] = [0] + 128 B is never clamped: the loads use [0] with an immediate offset */
	int xd[3];
#pragma unroll 1
	for (int u = 0; u < 3; ++u) {
		int i = tid + u * K1F_THREADS;
		i = i < slen ? i : slen - 1;
		const int rel = e0 + 1 + i;
		const int jr = (21 * (rel + 1) + c0 - 20 + 499) / 500 - 1;	/* numerator > 0 for every sample of the slice */
		const int x = (jr - g * 16) * 25 + (rel - e_rel(jr - 1) - 1);
		if (u == 0) { vo[0] = (unsigned)i * B; xd[0] = x; }
		else if (u == 1) { vo[1] = (unsigned)i * B; xd[1] = x; }
		else { vo[2] = (unsigned)i * B; xd[2] = x; }
	}
	/* index i of the family: superperiod per_lo + x + 8 i.  An ITERATION takes a pair (2 p, 2 p + 1): two slices in
	 * flight (one register set each), one wait, one barrier and one turn of the bookkeeping for two superperiods of
	 * mixing -- with one superperiod per iteration a wavefront spent as long outside the mixer as in it, and a SIMD
	 * needs three of its five mixing. */
	constexpr int CP = K1F_CHUNK / 2;	/* pairs per ticket */
	static_assert(K1F_DEPTH == 2 && K1F_CHUNK % 2 == 0 && CP >= 4, "the loop below is written for pairs and a ticket known at the fourth pair");
	const char *rbase = raw + ((p.per_lo + x) * K1F_PER_IN + e0 + 1) * B;	/* the slice in the family's first superperiod; workgroup-uniform */
	constexpr long long pbytes = (long long)K1F_PER_IN * B * 8;
	int p0 = rank * CP;	/* this iteration's pair */
	raw_t rr[2][3];
	/* the six loads of pair pr: superperiods 2 pr and 2 pr + 1 of the family (the family's last pair may lack its second
	 * half: the loads then fetch the first again) */
	auto issue_pair = [&](int pr) {
		const int ia = 2 * pr, ib = ia + 1 < n_x ? ia + 1 : ia;
		const char *rb = rbase + pbytes * ia;
		k1_raw_issue<FMT>(rr[0][0], vo[0], rb);
		k1_raw_issue<FMT, K1F_THREADS * B>(rr[0][1], vo[0], rb);
		k1_raw_issue<FMT>(rr[0][2], vo[2], rb);
		rb = rbase + pbytes * ib;
		k1_raw_issue<FMT>(rr[1][0], vo[0], rb);
		k1_raw_issue<FMT, K1F_THREADS * B>(rr[1][1], vo[0], rb);
		k1_raw_issue<FMT>(rr[1][2], vo[2], rb);
	};
	issue_pair(p0);
	/* the lane's LO values, behind the first samples' loads (one round trip for both); the table carries its own
	 * wrap-around (24 loads off one address) */
	v2f w[24];
	{
		const int ph = (p.no0 + e0 + 1 + off + 80) % 80;	/* 8000 = 100 LO periods: the same in every superperiod; e0 + 1 >= -23 */
		const float2 *lo = p.lo_ext + ((size_t)s * VDL2_CS + (active ? c : 0)) * p.lo_stride + 8 + ph;
#pragma unroll
		for (int t = 0; t < 24; ++t) {
			const float2 q = lo[t];
			w[t] = (v2f){q.x, q.y};
		}
	}
	/* ROT: the lane's output is window jr = 16 g + kk of every superperiod (336 outputs: 16 periods of the 21-output schedule), so
	 * its place in the schedule period never changes and its phase index moves by rs1 from one superperiod of the family to
	 * the next (8 superperiods, 128 schedule periods); index i of the family has rk0 + i rs1 mod M */
	unsigned rk0 = 0, rs1 = 0, rk = 0, ronv = 0;
	if constexpr (ROT) {
		const unsigned *rtab = r.tab + ((size_t)s * VDL2_CS + (active ? c : 0)) * K1R_TAB;
		const int t = r.i0 + g * 16 + kk;
		rk0 = k1r_add(k1r_period(rtab, 16 * (p.per_lo + x) + t / 21, r), rtab[t % 21], r.M);
		rs1 = k1r_mod(128ull * rtab[21], r.M, r.rM);
		ronv = rtab[23];
	}
	const float fn = (float)nwin;
	const float rfn = 1.0f / fn;	/* RN(1/nf) for k1_div_exact */
	const float2 *dec = p.dec + (size_t)s * VDL2_CS * p.cap + VDL2_CARRY_FRAMES + (p.per_lo + x) * K1F_PER_OUT + g * 16;	/* workgroup-uniform */
	const unsigned dvo = (unsigned)(((size_t)(active ? c : 0) * p.cap + kk) * sizeof(float2));	/* a stream's planes span < 4 GiB (VDL2_PLANES_MAX, vdl2gpu_create) */
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");	/* from here on the only memory operations are the counted ones below */
#pragma unroll
	for (int t = 0; t < 24; ++t)
		asm volatile("" : "+v"(w[t]));	/* loaded in front of the loop, once */
	if constexpr (ROT)
		asm volatile("" : "+v"(rk0), "+v"(rs1), "+v"(ronv));	/* likewise: the loop's waits are counted */
	const bool ron = ronv != 0;
	const unsigned xa = (unsigned)(size_t)(__attribute__((address_space(3))) const float2 *)&xs[0][0][kk * 25];
	unsigned tkr = 0;	/* lane 0 of wavefront 0: the counter's answer, landing while the chunk is worked on */
	int nxt = 0x7fffffff;
	int pos = 0;	/* position in the current chunk */
	int buf = 0;	/* which copy of the slices this iteration writes and reads */
	if constexpr (ROT)
		rk = k1r_mod(rk0 + (unsigned long long)(2 * p0) * rs1, r.M, r.rM);	/* of the first superperiod of pair p0 */
	while (p0 >= 0) {
		/* pair p0: registers -> float -> LDS slices, then refill the registers with the next pair.  Every iteration
		 * issues exactly 6 loads and then 2 stores per wavefront: only the 2 stores have been issued after the loads
		 * this iteration waits for (a ticket request is issued BEFORE an iteration's loads, so they see it land). */
		/* the SIMD's arbiter serves its oldest wavefront first: left alone, the five wavefronts of a SIMD advance
		 * at very different rates.  Rotating priorities keep them together. */
		switch ((pos + (int)blockIdx.x) & 3) {
		case 0: __builtin_amdgcn_s_setprio(0); break;
		case 1: __builtin_amdgcn_s_setprio(1); break;
		case 2: __builtin_amdgcn_s_setprio(2); break;
		default: __builtin_amdgcn_s_setprio(3); break;
		}
		asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
#pragma unroll
		for (int ab = 0; ab < 2; ++ab)
#pragma unroll
			for (int u = 0; u < 3; ++u)
				asm volatile("" : "+v"(rr[ab][u]));	/* read only behind the wait */
#pragma unroll
		for (int ab = 0; ab < 2; ++ab) {
			float2 *xb = xs[buf][ab];
#pragma unroll
			for (int u = 0; u < 3; ++u)
				xb[xd[u]] = k1_raw_cvt<FMT>(rr[ab][u]);
		}
		if (pos == 0) {
			/* ask for the next ticket: older than the loads issued below, so the next iteration's wait sees it land */
			const unsigned long long m = __ballot(tid == 0);
			asm volatile(K1_MASKED_ISSUE("global_atomic_add %0, %1, %2, %4 sc0")
				     : "+v"(tkr) : "v"(0u), "v"(1u), [m] "s"(m), "s"(ctr) : "memory", "s2", "s3");
		}
		if (pos == 1) {
			asm volatile("" : "+v"(tkr));	/* it has landed: the wait above was for loads issued after the request */
			if (tid == 0)
				s_next = ((int)(tkr - tbase) + nfam) * CP;
		}
		if (pos == 2)
			nxt = __builtin_amdgcn_readfirstlane(s_next);	/* first pair of the next ticket; written one barrier ago */
		/* the next pair: in this chunk, the next ticket's first, or none (the loads then fetch this one again) */
		int p1 = pos < CP - 1 ? p0 + 1 : nxt;
		p1 = 2 * p1 < n_x ? p1 : -1;
		/* ROT: the four table entries of this pair's two rotations, older than the six sample loads below: the wait in front
		 * of the first rotation (vmcnt(6)) is for them alone.  Then the index moves on: two superperiods within a ticket,
		 * worked out anew where the next ticket begins. */
		v2f rth[2], rtl[2];
		if constexpr (ROT) {
			const unsigned rkb = k1r_add(rk, rs1, r.M);
			k1r_issue(rth[0], (rk >> 12) * 8u, r.hi);
			k1r_issue(rtl[0], (rk & 4095u) * 8u, r.lo);
			k1r_issue(rth[1], (rkb >> 12) * 8u, r.hi);
			k1r_issue(rtl[1], (rkb & 4095u) * 8u, r.lo);
			if (pos < CP - 1)
				rk = k1r_add(rkb, rs1, r.M);
			else
				rk = k1r_mod(rk0 + (unsigned long long)(2 * (p1 >= 0 ? p1 : p0)) * rs1, r.M, r.rM);
		}
		issue_pair(p1 >= 0 ? p1 : p0);
		__syncthreads();	/* the slices are written */
		const bool has_b = 2 * p0 + 1 < n_x;
		const unsigned xc = xa + (unsigned)buf * (unsigned)sizeof(xs[0]);
#pragma unroll
		for (int ab = 0; ab < 2; ++ab) {
			v2f res = {0.0f, 0.0f};
			if (ab == 0 || has_b) {
				v2f acc = {0.0f, 0.0f};
				if (K1_REAL(FMT)) {
					const v2f *xp = reinterpret_cast<const v2f *>(&xs[buf][ab][kk * 25]);
#pragma unroll
					for (int t = 0; t < 23; ++t) {
						const float x = xp[t].x;
						acc += (v2f){x, x} * w[t];
					}
					if (nwin == 24) {
						const float x = xp[23].x;
						acc += (v2f){x, x} * w[23];
					}
				} else {
					/* six blocks of 4 samples; every block is mixed while the next one's samples are on their way
					 * from LDS (reads return in order: at most 4 outstanding = the previous block is there); which
					 * slice of the pair is part of the reads' immediate offsets */
					auto mix = [&](auto par) {
						constexpr int XO = (int)sizeof(xs[0][0]) * decltype(par)::value;
						v2f x0[4], x1[4];
						asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
						k1_lds_issue4<0 + XO>(x0, xc);
						k1_lds_issue4<32 + XO>(x1, xc);
						asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
						k1_cmac4_v(acc, x0, &w[0]);
						k1_lds_issue4<64 + XO>(x0, xc);
						asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
						k1_cmac4_v(acc, x1, &w[4]);
						k1_lds_issue4<96 + XO>(x1, xc);
						asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
						k1_cmac4_v(acc, x0, &w[8]);
						k1_lds_issue4<128 + XO>(x0, xc);
						asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
						k1_cmac4_v(acc, x1, &w[12]);
						k1_lds_issue4<160 + XO>(x1, xc);
						asm volatile("s_waitcnt lgkmcnt(4)" ::: "memory");
						k1_cmac4_v(acc, x0, &w[16]);
						asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
						k1_cmac3_v(acc, x1, &w[20]);
						if (nwin == 24)
							k1_cmac1_v(acc, x1[3], w[23]);
					};
					if (ab)
						mix(std::integral_constant<int, 1>{});
					else
						mix(std::integral_constant<int, 0>{});
				}
				res = k1_div_exact(acc, fn, rfn);	/* D /= nf (d8psk.c:377) */
			}
			if constexpr (ROT) {
				if (ab == 0)
					asm volatile("s_waitcnt vmcnt(6)" ::: "memory");	/* the six sample loads were issued behind the entries */
				asm volatile("" : "+v"(rth[ab]), "+v"(rtl[ab]));	/* read only behind the wait */
				const float2 q = k1r_cmul(make_float2(res.x, res.y),
							  k1r_cmul(make_float2(rth[ab].x, rth[ab].y), make_float2(rtl[ab].x, rtl[ab].y)));
				if (ron) {
					res.x = q.x;
					res.y = q.y;
				}
			}
			/* exactly one store instruction per superperiod and wavefront: four whole lines (channels beyond nbch masked
			 * off; a wavefront without any channel, or the missing second half of the family's last pair, still issues
			 * it, with no lane enabled, so that the count above holds) */
			k1_store_masked(dec + (long long)(2 * p0 + ab) * (8 * K1F_PER_OUT), dvo, res, active && (ab == 0 || has_b));
		}
		/* no second barrier: the next iteration writes the other copy of the slices, and the one after that writes this
		 * one only behind the next iteration's barrier, which every wave reaches after its reads here */
		p0 = p1;
		pos = pos + 1 == CP ? 0 : pos + 1;
		buf ^= 1;
	}
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
