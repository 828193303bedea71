/* vdl2gpu_resolve.h -- K2s, K2b, K2c, K2f, K2d: candidate order, clusters, the real chain, commit, payload.  Part of the device side of libvdl2gpu.so; included by vdl2gpu_kernels.h only. */
#ifndef VDL2GPU_RESOLVE_H
#define VDL2GPU_RESOLVE_H

/* ====================================================================== K2s
 * Per channel: sort the candidates by time (bitonic network in LDS) for the resolver, and pick the
 * ones whose cluster is worth precomputing: the first of its (sub-phase, parity) class within a
 * burst's worth of samples.  A later candidate of the same class can only be reached if the detector
 * turns history-free in the few samples between the two; the resolver computes such a cluster itself
 * when it ever needs one (status CL_INVALID), so this is a cost decision, never a correctness one.
 */
#define K2S_NT 1024
#define K2S_MERGE 256		/* candidates a repair round merges into the sorted table instead of sorting again */
#define K2S_LOOKBACK 72		/* a triggered detector is busy for at least 9 symbols = 72 samples */
__global__ __launch_bounds__(K2S_NT)
void k2s_sort(K2Params p)
{
	__shared__ unsigned long long sbuf[VDL2_CAND_CAP];
	__shared__ WgSortShared ws;
	__shared__ int s_np;
	const int tid = threadIdx.x;
	const int c = blockIdx.x, s = (int)blockIdx.y;
	const int sc = s * VDL2_CS + c;
	if (p.force_serial)
		return;
	k2x_drain<K2S_NT>(*reinterpret_cast<K2xWork *>(ws.tmp), p, sc);	/* the common area of the scan in front (region scan; a complete scan) */
	if (p.round > 0 && p.fail[sc] >= VDL2_VERIFIED)
		return;
	int ncand = (int)p.ctl[CTL_CAND0 + sc];
	if (ncand > VDL2_CAND_CAP || p.ctl[CTL_CANDOVF0(p) + sc] != 0)
		return;		/* tables unusable: the resolver runs serially */
	const Cand *cands = p.cands + (size_t)sc * VDL2_CAND_CAP;
	int *skey = p.skey + (size_t)sc * VDL2_CAND_CAP;
	unsigned short *sidx = p.sidx + (size_t)sc * VDL2_CAND_CAP;
	unsigned short *prim = p.prim + (size_t)sc * VDL2_CAND_CAP;
	for (int i = tid; i < ncand; i += K2S_NT)
		sbuf[i] = (((unsigned long long)(unsigned)(cands[i].nrel * 4 + cands[i].r)) << 16) | (unsigned)i;
	if (tid == 0)
		s_np = 0;
	__syncthreads();
	wg_sort_u64<K2S_NT>(sbuf, ws, ncand, 18, (unsigned)(VDL2_CARRY_FRAMES + p.J));
	/* repair round: candidates are only ever appended and a cluster depends on nothing but its own
	 * candidate and the samples, so the clusters of the earlier rounds stand -- only primaries that are new
	 * (or were not primary before) go to K2b */
	const int nold = (p.round > 0) ? (int)p.ctl[CTL_NCLUST0(p) + sc] : 0;
	for (int j = tid; j < ncand; j += K2S_NT) {
		const unsigned long long v = sbuf[j];
		const int key = (int)(v >> 16), idx = (int)(v & 0xffffu);
		skey[j] = key;
		sidx[j] = (unsigned short)idx;
		const int n = key >> 2, cls = (key & 3) * 2 + (n & 1);
		bool primary = true;
		for (int i = j - 1; i >= 0; --i) {
			const int ki = (int)(sbuf[i] >> 16), ni = ki >> 2;
			if (n - ni >= K2S_LOOKBACK)
				break;
			if ((ki & 3) * 2 + (ni & 1) == cls) {
				primary = false;
				break;
			}
		}
#ifdef VDL2GPU_TESTHOOKS
		if (p.prim_drop > 0 && j % p.prim_drop == p.prim_drop - 1)
			primary = false;
#endif
		int2 *head = p.clhead + (size_t)sc * VDL2_CAND_CAP + idx;
		if (!primary)
			*head = cl_pack(0, CL_INVALID, 0, 0, 0, 0, 0);
		else if (idx >= nold || (head->y & 3) == CL_INVALID)
			prim[atomicAdd(&s_np, 1)] = (unsigned short)idx;
	}
	__syncthreads();
	if (tid == 0) {
		p.ctl[CTL_NPRIM0(p) + sc] = (unsigned)s_np;
		p.ctl[CTL_NCLUST0(p) + sc] = (unsigned)ncand;
	}
}

/* K2s for a repair round that only re-resolves (K2Params.mini_round): the table is sorted but for the handful of candidates
 * the verify pass appended -- merge them in.  Every old entry moves up by the number of new keys below it, every new one goes
 * where a binary search of the old list plus its rank among the new ones puts it (keys are unique: what the verify pass lists
 * was not in the table).  Nothing else changes: the old clusters stand, the new candidates have none (their heads say so), no
 * primaries are chosen.  A kernel of its own because of its footprint: 2 KB of LDS where k2s_sort has 84 -- one workgroup per
 * channel that wants half a CU's LDS waits for the other stage's wide kernel to drain before it gets it. */
#define K2M_NT 256	/* four wavefronts of 40 registers fit beside anything */
__global__ __launch_bounds__(K2M_NT)
void k2s_merge(K2Params p)
{
	__shared__ unsigned long long knew[K2S_MERGE];
	__shared__ K2xWork xw;
	const int tid = threadIdx.x;
	const int c = blockIdx.x, s = (int)blockIdx.y;
	const int sc = s * VDL2_CS + c;
	if (p.force_serial)
		return;
	k2x_drain<K2M_NT>(xw, p, sc);	/* the common area of the verify pass in front: what it finds there fails the channel like any other hit */
	if (p.fail[sc] >= VDL2_VERIFIED)
		return;
	const int ncand = (int)p.ctl[CTL_CAND0 + sc];
	unsigned *ovf = p.ctl + CTL_CANDOVF0(p) + sc;
	if (ncand > VDL2_CAND_CAP || *ovf != 0)
		return;		/* tables unusable: the resolver runs serially */
	const int nold = (int)p.ctl[CTL_NCLUST0(p) + sc], nnew = ncand - nold;
	if (nnew <= 0)
		return;		/* (a channel that failed for another reason than an unlisted event: the resolver will find nothing new) */
	if (nnew > K2_MERGE_LIM(p)) {	/* a handicapped test build, a pathological input: not worth a sort kernel's footprint in every push */
		if (tid == 0) {
			K2_COUNT(p, K2_DBG_ESC_MERGE);
			K2_COUNT(p, K2_DBG_ESC_MERGE_SORT);
		}
		if (tid == 0)
			atomicOr(ovf, 2u);	/* the resolver takes the channel through the serial machine (a complete round resets this); bit 1, not
						 * bit 0: the tables were not full, the host must not shorten its parts for this (k3_rebase) */
		return;
	}
	const Cand *cands = p.cands + (size_t)sc * VDL2_CAND_CAP;
	int *skey = p.skey + (size_t)sc * VDL2_CAND_CAP;
	unsigned short *sidx = p.sidx + (size_t)sc * VDL2_CAND_CAP;
	if (tid < nnew)
		knew[tid] = (((unsigned long long)(unsigned)(cands[nold + tid].nrel * 4 + cands[nold + tid].r)) << 16) | (unsigned)(nold + tid);
	__syncthreads();
	/* everything is read before anything is written: a thread's share of the old list into registers, the new keys' places by
	 * binary search of the old list */
	constexpr int PER = VDL2_CAND_CAP / K2M_NT;
	unsigned long long v[PER];
	int up[PER];
#pragma unroll
	for (int k = 0; k < PER; ++k) {
		const int j = tid + k * K2M_NT;
		v[k] = j < nold ? (((unsigned long long)(unsigned)skey[j] << 16) | sidx[j]) : ~0ull;
	}
#pragma unroll
	for (int k = 0; k < PER; ++k) {
		up[k] = 0;
		for (int i = 0; i < nnew; ++i)
			up[k] += (knew[i] < v[k]) ? 1 : 0;
	}
	int at = 0;
	unsigned long long vn = 0;
	if (tid < nnew) {
		vn = knew[tid];
		const int kn = (int)(vn >> 16);
		int a = 0, b = nold;	/* old entries below vn */
		while (a < b) {
			const int m = (a + b) >> 1;
			if (skey[m] < kn)
				a = m + 1;
			else
				b = m;
		}
		at = a;
		for (int i = 0; i < nnew; ++i)
			at += (knew[i] < vn) ? 1 : 0;
	}
	__syncthreads();
#pragma unroll
	for (int k = 0; k < PER; ++k) {
		const int j = tid + k * K2M_NT;
		if (j < nold) {
			skey[j + up[k]] = (int)(v[k] >> 16);
			sidx[j + up[k]] = (unsigned short)(v[k] & 0xffffu);
		}
	}
	if (tid < nnew) {
		skey[at] = (int)(vn >> 16);
		sidx[at] = (unsigned short)(vn & 0xffffu);
	}
	if (tid == 0) {
		p.ctl[CTL_NPRIM0(p) + sc] = 0u;
		p.ctl[CTL_NCLUST0(p) + sc] = (unsigned)ncand;
	}
}
static_assert(VDL2_CAND_CAP % K2M_NT == 0 && K2S_MERGE <= K2M_NT, "k2s_merge");

/* ====================================================================== K2b
 * One wavefront per primary trigger candidate (persistent workgroups pull tickets):
 * handle the trigger from what the candidate record says the detector saw, rebuild
 * the phase ring it returns to, run the exact machine through the 68 evaluations
 * behind the burst (and any burst that follows before the detector is history-free
 * again) and record where and how the idle search resumes.
 */
#ifndef K2B_WAVES
#define K2B_WAVES 3	/* 163 registers: with 4 (128) the compiler spilled 12-20 of them to scratch; the kernel's time does not depend on 3 / 4 / 6 wavefronts per SIMD */
#endif
#ifndef K2B_GRIDW
#define K2B_GRIDW K2B_WAVES	/* wavefronts per SIMD the cluster kernel's (persistent) grid asks for */
#endif
__global__ __launch_bounds__(K2B_NT) __attribute__((amdgpu_waves_per_eu(K2B_WAVES, 8)))
void k2b_clusters(K2Params p)
{
	__shared__ MachSharedT<K2B_NT> sh;
	__shared__ float sgrey[3 * 257];
	__shared__ unsigned s_pref[65];
	const int tid = threadIdx.x;
	const int nsc = p.nstreams * VDL2_CS;
	if (p.force_serial)
		return;
	for (int i = tid; i < 257; i += K2B_NT) {
		sgrey[i] = d_tab(c_grey1, i);
		sgrey[257 + i] = d_tab(c_grey2, i);
		sgrey[514 + i] = d_tab(c_grey3, i);
	}
	mach_init_taps(sh);
	/* blockIdx.y selects a group of up to 64 (stream, channel) slots; exclusive prefix of the
	 * group's cluster counts maps a ticket to (slot, primary candidate) */
	const int sc0 = (int)blockIdx.y * 64;
	const int nsc64 = (nsc - sc0) < 64 ? (nsc - sc0) : 64;
	if (tid == 0) {
		unsigned acc = 0;
		for (int k = 0; k < nsc64; ++k) {
			unsigned n = p.ctl[CTL_NPRIM0(p) + sc0 + k];
			n = n > VDL2_CAND_CAP ? VDL2_CAND_CAP : n;
			if (p.round > 0 && p.fail[sc0 + k] >= VDL2_VERIFIED)
				n = 0;
			s_pref[k] = acc;
			acc += n;
		}
		s_pref[nsc64] = acc;
	}
	__syncthreads();
	const unsigned total = s_pref[nsc64];
	int ord = 0;	/* (development counters: the wavefront's n-th cluster) */
	for (unsigned tk = blockIdx.x; tk < total; tk += gridDim.x) {
		int scl = 0;
		while (scl + 1 < nsc64 && s_pref[scl + 1] <= tk)
			++scl;
		const int sc = sc0 + scl;
		const int idx = (int)p.prim[(size_t)sc * VDL2_CAND_CAP + (tk - s_pref[scl])];
		const int s = sc / VDL2_CS, c = sc % VDL2_CS;
		MachCtx cx;
		mach_ctx(cx, p, s, c, true);
		const Cand cd = p.cands[(size_t)sc * VDL2_CAND_CAP + idx];
		Cluster *cl = p.clusters + (size_t)sc * VDL2_CAND_CAP + idx;
		MachState st = {cx.dec_base + cd.nrel, cd.r, VDL2_STEADY};
		cx.grey = sgrey;
		cx.desc_static = ((long long)sc * VDL2_CAND_CAP + idx) * VDL2_CL_MAXB;
		MachOut out;
		mach_out_clear(out);
		/* The candidate record holds what the detector saw when it fired -- the three fit errors and
		 * the slope (the scan computed them with the detector's own arithmetic) --, so the trigger is
		 * handled from those; what has to be rebuilt is the phase ring the detector returns to after
		 * the burst: the phases of the 68 evaluations up to and including this one. */
		const long long t0 = wall_clock64();
		const long long nstar = st.pos;
		mach_need<K2B_NT, true>(sh, cx, nstar - 152, nstar + 1);
		static_assert(K2B_NT == 64 && VDL2_NPH == 68, "ring rebuild: 64 phases here, the last 4 in mach_trigger's filter pass");
		sh.pbuf[tid] = mach_fir<K2B_NT, true>(sh, cx, nstar - 2LL * (VDL2_NPH - 1 - tid), st.r);
		if (tid == 0) {
			sh.errs[0] = 500.0f;	/* errors re-armed (d8psk.c:308) */
			sh.errs[1] = 500.0f;
			sh.frs[0] = cd.pfr;
		}
		__syncthreads();
		const long long t1 = wall_clock64();
		int rc;
		{
			const MachTrig tg = mach_trigger<K2B_NT, true>(sh, cx, nstar, cd.p2err, cd.perr, cd.err, cd.pfr, st.r);
			if (tg.defer) {
				out.ndefer++;
				rc = MR_DEFER;
			} else {
				const long long nlast = mach_commit_trigger<K2B_NT, true>(sh, cx, cx.x - cx.dec_base, nstar, tg, out);
#ifdef VDL2GPU_TESTHOOKS
				/* invariant (b) at CTL_NWIN0: the cluster's first descriptor as it lies in the pool (lane 0 wrote it) against the candidate */
				if (tid == 0 && out.nslots == 1 && !out.badslot) {
					K2_COUNT(p, K2_DBG_CHK_B_CLUSTER);
					if (p.stage[cx.desc_static].nstar != p.dec_base + cd.nrel)
						K2_COUNT(p, K2_DBG_INV_B_CLUSTER);
				}
#endif
				out.neval += 1;
				st.pos = nlast + 2;
				st.r = tg.rb;
				st.fresh = 0;
				rc = machine_run<K2B_NT, true>(sh, cx, st, true, 1, VDL2_CL_MAXB, 0, out);
			}
		}
		const long long t2 = wall_clock64();
		if (tid == 0 && p.dbg && (tk & 15u) == 0) {
			atomicAdd(p.dbg + K2_DBG_K2B_RING_TICKS, (unsigned long long)(t1 - t0));
			atomicAdd(p.dbg + K2_DBG_K2B_REST_TICKS, (unsigned long long)(t2 - t1));
			atomicAdd(p.dbg + K2_DBG_K2B_SAMPLED, 1ull);
			atomicAdd(p.dbg + K2_DBG_K2B_TRIG, (unsigned long long)out.ntrig);
			atomicAdd(p.dbg + K2_DBG_K2B_EVAL, (unsigned long long)out.neval);
			atomicMax(p.dbg + K2_DBG_K2B_MAX_TICKS, (unsigned long long)(t2 - t1));
			atomicAdd(p.dbg + K2_DBG_K2B_STEADY, (unsigned long long)(rc == MR_STEADY));
			atomicAdd(p.dbg + K2_DBG_K2B_REJ, (unsigned long long)out.nrej);
		}
		if (tid == 0 && p.dbg) {	/* is a wavefront's first cluster slower than its later ones (code fetched cold)? */
			const int o = ord < 3 ? ord : 3;
			atomicAdd(p.dbg + K2_DBG_K2B_ORD_TICKS0 + o, (unsigned long long)(t2 - t0));
			atomicAdd(p.dbg + K2_DBG_K2B_ORD_COUNT0 + o, 1ull);
		}
		++ord;
		int status;
		if (rc == MR_STEADY)
			status = CL_STEADY;
		else if (rc == MR_DEFER && out.ntrig == 0)
			status = CL_DEFER_FIRST;
		else
			status = CL_NONSTEADY;
		if (out.badslot)	/* descriptor pool full */
			status = CL_INVALID;
		if (out.badslot && tid == 0)
			K2_COUNT(p, K2_DBG_ESC_STAGE);
		if (status == CL_NONSTEADY)
			mach_store(sh, st, &cl->saved);
		if (tid == 0)	/* descriptors sit in static slots desc_static + i: the head only needs their number */
			p.clhead[(size_t)sc * VDL2_CAND_CAP + idx] =
			    cl_pack((int)(st.pos - cx.dec_base), status, st.r, out.nslots < VDL2_CL_MAXB ? out.nslots : VDL2_CL_MAXB,
				    out.ntrig, out.nrej, out.nburst);
		__syncthreads();
	}
}

/* ====================================================================== K2c
 * Resolver: one workgroup per VDL channel follows the real chain of events.  While the detector is history-free the next event is
 * simply the first candidate of the current (sub-phase, sample parity) at or after `pos`, and its consequences were precomputed by
 * K2b; otherwise the serial machine runs until the detector is history-free again.
 *   1.  the candidates as K2s sorted them, their ranks class by class (k2c_class_lists)                            (parallel)
 *   2.  for every candidate the one that follows its cluster, then four hops deep (k2c_successors, k2c_four_hops)  (parallel)
 *   3.  walk the chain through that table (k2c_walk)                                                  (one lane, LDS only)
 *   4.  list the bursts of the visited clusters, add their counters (k2c_publish)                                  (parallel)
 */

/* first sorted candidate at/after stream-relative time `want` of class (r, parity of want): a binary
 * search in that class's own list (ranks in time order, ascending), -1 if there is none.  (Scanning
 * the time-sorted list for the next entry of the class costs a candidate of a rare class a walk to the
 * end of the list, one LDS round trip per step.) */
__device__ __forceinline__ int k2c_next(const int *skey, const unsigned short *clist, const int *coff, int want, int r)
{
	const int cls = r * 2 + (want & 1);
	int lo = coff[cls], hi = coff[cls + 1];
	const int end = hi;
	while (lo < hi) {
		const int mid = (lo + hi) >> 1;
		if ((skey[clist[mid]] >> 2) < want)	/* (the class list holds ranks; their times are the sorted keys': four bytes a candidate less in LDS) */
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo < end ? (int)clist[lo] : -1;
}

/* one hop of the walk in 16 bits: rank of the successor (13 bits) | its cluster status << 13, 0xffff = none */
#define K2C_RANK 0x1fffu
#define K2C_RBITS 13
#define K2C_HOP_NONE 0xffffu
#define K2C_VIS 4096	/* entries of the visited list; more than that (it would take ten thousand bursts in a
			 * channel's push) fails the channel over to the serial redo */
/* sjump[j], for a steady cluster j: bits 0-12 = the last steady cluster within four hops of j (j itself if
 * the first hop is not steady); K2C_J_CONT: all four hops were steady, go on from there; otherwise the
 * chain ends behind it (no successor) or, K2C_J_SPECIAL, at the non-steady cluster in bits 16-28 */
#define K2C_J_CONT 0x80000000u
#define K2C_J_SPECIAL 0x40000000u
static_assert(VDL2_CAND_CAP <= 8191, "a hop holds a 13-bit rank");

/* ---- steps of following the chain that K2c, K2p, K2f and K2d share */
/* The push's mask of channels a repair round re-resolved or K2f redid serially (K2Params.fmask, a bit per channel slot below VDL2_FMASK_SLOTS).
 * If K2d ran ahead on the first pass's selection, what it made of such a channel is void (K2d's second pass tags those records REC_VOID:
 * the host and K4 drop them) and K2d decodes the repaired selection in that second pass. */
__device__ __forceinline__ void k2_fmask_set(const K2Params &p, int sc)
{
	if (p.fmask && sc < VDL2_FMASK_SLOTS)
		atomicOr(p.fmask + (sc >> 5), 1u << (sc & 31));
}

__device__ __forceinline__ bool k2_fmask_test(const K2Params &p, int sc) { return sc < VDL2_FMASK_SLOTS && (p.fmask[sc >> 5] >> (sc & 31) & 1u); }

/* thread 0 of a repair round's workgroup: channel sc is resolved again.  nwin0 (CTL_NWIN0): what that makes void of the first selection
 * before the round has listed any window -- all of it where the channel is resolved again from its input state, nothing in a local repair */
__device__ __forceinline__ void k2_begin_repair(const K2Params &p, int sc, unsigned nwin0)
{
	p.redo[sc] = 1;
	atomicAdd(&p.outc_total->repairs, 1u);	/* channel-pushes that went through a repair round */
	if (p.dbg)
		atomicAdd(p.dbg + K2_DBG_REPAIRED, 1ull);
	p.ctl[CTL_NSEL1(p) + sc] = 0;	/* (the repair rounds' own selection: see CTL_NSEL1) */
	p.ctl[CTL_NSEG0(p) + sc] = 0;
	p.ctl[CTL_NWIN0(p) + sc] = nwin0;
	k2_fmask_set(p, sc);
}

/* is stream-relative time t inside one of the nwin windows a local repair listed (K2Params.win) */
__device__ __forceinline__ bool k2_in_windows(const K2Params &p, const int2 *win, unsigned nwin, long long t)
{
	bool in = false;
	for (unsigned w = 0; w < nwin && w < (unsigned)K2_WIN_LIM(p); ++w)
		in = in || (t >= win[w].x && t < win[w].y);
	return in;
}

/* the chain idles in class (r, parity of lo) over stream-relative [lo, hi) and the probe did not scan that class: entry q of the
 * channel's list of stretches the verify pass must confirm empty.  false: the list is full and the caller fails the channel.
 * (K2c's two lists; k2p_patch, whose every lane counts the entries and lane 0 stores them, has the same lines written out: as a
 * call of this the kernel spills three scalar registers fewer, and its resource line is held where it was measured.) */
__device__ __forceinline__ bool k2_emit_seg(const K2Params &p, Seg *segs, unsigned q, int lo, int hi, int r)
{
	if (q >= (unsigned)K2_SEG_LIM(p)) {
		K2_COUNT(p, K2_DBG_ESC_SEG);
		return false;
	}
	segs[q] = Seg{lo, hi, r, 0};
	return true;
}

/* the ns > 0 bursts of a cluster K2b made go to the end of a selection list of length *nsel (K2c publishing: an LDS copy of it): static
 * descriptor slots, slot0 = (channel * VDL2_CAND_CAP + candidate index) * VDL2_CL_MAXB onwards; what the list does not hold is counted as dropped */
template <class T> __device__ __forceinline__ void k2_select_slots(const K2Params &p, unsigned *sel, T *nsel, unsigned slot0, int ns)
{
	const unsigned q = (unsigned)atomicAdd(nsel, (T)ns);
	for (int i = 0; i < ns; ++i) {
		if (q + i < VDL2_SEL_CAP)
			sel[q + i] = slot0 + i;
		else
			atomicAdd(&p.outc->dropped, 1u);
	}
}

/* the class (r, parity of STREAM time pos: a push's time base may be odd) is one the probe did not scan everywhere */
__device__ __forceinline__ bool k2_unprobed(const K2Params &p, int r, long long pos) { return r != p.probe_r || (int)(pos & 1) != p.probe_par; }

/* The resolver's tables in LDS: 23 bytes per candidate, the tables hold 6144.  (Sorted rank -> candidate index is read from device
 * memory where it is needed -- publishing: a lane each --, and the rank of the candidate that follows a cluster is the first hop of
 * swalk[].)  The arrays are __shared__ variables of k2c_resolve, each one of its own, and this struct refers to them: as members of
 * one LDS struct the compiler aligns them to their element and unrolls the loops over them less (fewer registers, other
 * instruction counts than the kernel has been measured with: DESIGN.md 8). */
struct K2cShared {
	int (&skey)[VDL2_CAND_CAP];		/* sorted keys: nrel*4 + r */
	uint8_t (&sstat)[VDL2_CAND_CAP];	/* cl_stat4() of every cluster's head */
	unsigned short (&svis)[K2C_VIS];	/* what the real chain visited: rank | 0x8000 = that cluster; rank = the steady hops of swalk[rank] */
	unsigned (&sjump)[VDL2_CAND_CAP];	/* the walk's view of swalk[]: see K2C_J_* */
	int (&sx)[VDL2_CAND_CAP];		/* where the idle search resumes behind every candidate's cluster (cl_pack().x), by sorted rank; the rest
						 * of the head is read from device memory where it is needed (publishing: every lane its own) */
	int (&walk)[4];				/* lane 0's walk to everybody: see k2c_walk; publishing: list positions, visited entries */
	int (&cnt)[4];				/* what the visited clusters counted: triggers, rejects, bursts */
	unsigned short (&clist)[VDL2_CAND_CAP];	/* ranks of the candidates, class by class, time order within */
	unsigned long long (&swalk)[VDL2_CAND_CAP];	/* the next four hops from a steady cluster: what the walk reads */
	int (&coff)[9];				/* where each class (r * 2 + time parity) starts in clist */
	int (&wcnt)[K2_NT / 64][8];
};

/* 1b. the class lists, a counting sort that keeps the time order: every thread counts the classes in
 *     its own contiguous stretch of the sorted list, an exclusive scan over (class, thread) turns the
 *     counts into positions, and the thread places its stretch */
__device__ __forceinline__ void k2c_class_lists(const K2cShared &ks, int tid, int ncand)
{
	const int per = (ncand + K2_NT - 1) / K2_NT;
	const int j0 = tid * per < ncand ? tid * per : ncand, j1 = j0 + per < ncand ? j0 + per : ncand;
	int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	for (int j = j0; j < j1; ++j) {
		const int k = ks.skey[j], cls = (k & 3) * 2 + ((k >> 2) & 1);
#pragma unroll
		for (int q = 0; q < 8; ++q)
			cnt[q] += (cls == q);
	}
	const int wave = tid >> 6, lane = tid & 63;
	int excl[8];
#pragma unroll
	for (int q = 0; q < 8; ++q) {
		int v = cnt[q];
		for (int d = 1; d < 64; d <<= 1) {
			const int o = __shfl_up(v, d, 64);
			if (lane >= d)
				v += o;
		}
		excl[q] = v - cnt[q];
		if (lane == 63)
			ks.wcnt[wave][q] = v;
	}
	__syncthreads();
	if (tid == 0) {
		int acc = 0;
		for (int q = 0; q < 8; ++q) {
			ks.coff[q] = acc;
			for (int w = 0; w < K2_NT / 64; ++w) {
				const int v = ks.wcnt[w][q];
				ks.wcnt[w][q] = acc;	/* where wave w's share of class q starts */
				acc += v;
			}
		}
		ks.coff[8] = acc;
	}
	__syncthreads();
#pragma unroll
	for (int q = 0; q < 8; ++q)
		excl[q] += ks.wcnt[wave][q];
	for (int j = j0; j < j1; ++j) {
		const int k = ks.skey[j], cls = (k & 3) * 2 + ((k >> 2) & 1);
		int at = 0;
#pragma unroll
		for (int q = 0; q < 8; ++q)
			if (cls == q)
				at = excl[q]++;
		ks.clist[at] = (unsigned short)j;
	}
	__syncthreads();
}

/* 2. successor table.  (Interleaving several searches per thread to overlap their LDS round trips
 *    was slower: this kernel, with two serial machines inlined, has no registers to spare.) */
__device__ __forceinline__ void k2c_successors(const K2cShared &ks, int tid, int ncand)
{
	unsigned short *const sw16 = reinterpret_cast<unsigned short *>(ks.swalk);	/* (hop i of rank j: sw16[4 j + i]) */
	for (int j = tid; j < ncand; j += K2_NT) {
		int nx = -1;
		if (stat4_status(ks.sstat[j]) == CL_STEADY)
			nx = k2c_next(ks.skey, ks.clist, ks.coff, ks.sx[j], stat4_r(ks.sstat[j]));	/* sx[j] lies behind the candidate's own time */
		/* the first hop: rank of the candidate that follows the cluster | that one's status (the other three: 2b) */
		sw16[4 * j] = (nx < 0) ? (unsigned short)K2C_HOP_NONE : (unsigned short)((unsigned)nx | ((unsigned)stat4_status(ks.sstat[nx]) << K2C_RBITS));
	}
	__syncthreads();
}

/* 2b. four hops per table entry: the walk is one lane chasing pointers through LDS, a round
 *     trip per read, so it reads as rarely as possible */
__device__ __forceinline__ void k2c_four_hops(const K2cShared &ks, int tid, int ncand)
{
	unsigned short *const sw16 = reinterpret_cast<unsigned short *>(ks.swalk);	/* (hop i of rank j: sw16[4 j + i]) */
	for (int j = tid; j < ncand; j += K2_NT) {
		unsigned jv = 0;
		int at = j;
		bool open = (stat4_status(ks.sstat[j]) == CL_STEADY);
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			unsigned hop = K2C_HOP_NONE;
			if (open) {
				hop = sw16[4 * at];	/* (first hops only are read here, and nobody writes them in this step) */
				if (hop != K2C_HOP_NONE) {
					open = ((hop >> K2C_RBITS) == CL_STEADY);
					if (open)
						at = (int)(hop & K2C_RANK);
				} else
					open = false;
			}
			if (i > 0)
				sw16[4 * j + i] = (unsigned short)hop;
			if (!open && !(jv & K2C_J_SPECIAL) && hop != K2C_HOP_NONE)
				jv |= K2C_J_SPECIAL | ((hop & K2C_RANK) << 16);
		}
		ks.sjump[j] = jv | (unsigned)at | (open ? K2C_J_CONT : 0u);
	}
	__syncthreads();
}

/* 3. history-free at (st.pos, st.r): lane 0 walks the successor table until something special happens and leaves in ks.walk[]
 *    [0] the candidate (rank) the chain has arrived at, -1: no more candidates; [1] the last steady cluster it went through, -1: none;
 *    [2] 1 = the cluster at [0] is not a steady one.  nvis: slots of svis[] in use (lane 0's copy counts). */
__device__ __forceinline__ void k2c_walk(const K2cShared &ks, const K2Params &p, int sc, const MachCtx &cx, const MachState &st, bool lazy, int seg_from, int &nvis)
{
	int cur = k2c_next(ks.skey, ks.clist, ks.coff, (int)(st.pos - cx.dec_base), st.r);
	int last = -1, why = 0;	/* why: 0 = no more candidates, 1 = special cluster at cur */
	if (lazy && k2_unprobed(p, st.r, st.pos)) {
		/* the chain idles from here to the next candidate in a class the probe did not
		 * scan: K2a-verify must confirm there really is nothing in between */
		const int g_hi = (cur >= 0) ? (ks.skey[cur] >> 2) : (int)(cx.avail_end - cx.dec_base);
		if (g_hi > seg_from && !k2_emit_seg(p, p.segs + (size_t)sc * VDL2_SEG_CAP, atomicAdd(p.ctl + CTL_NSEG0(p) + sc, 1u), (int)(st.pos - cx.dec_base), g_hi, st.r))
			atomicMin(p.fail + sc, 0);
	}
	if (cur >= 0 && stat4_status(ks.sstat[cur]) != CL_STEADY)
		why = 1;
	else if (cur >= 0) {
		/* A lone lane chasing pointers: a wavefront on its own issues an instruction every ~5
		 * cycles, so the loop is four instructions and one LDS round trip per four clusters;
		 * what was visited is worked out from the list afterwards, by everybody. */
		if (nvis < K2_VIS_LIM(p))
			ks.svis[nvis] = (unsigned short)(cur | 0x8000);
		++nvis;
		last = cur;
		unsigned v;
		for (;;) {
			v = ks.sjump[last];
			if (nvis < K2_VIS_LIM(p))
				ks.svis[nvis] = (unsigned short)last;
			++nvis;
			if (!(v & K2C_J_CONT))
				break;
			last = (int)(v & K2C_RANK);
		}
		last = (int)(v & K2C_RANK);
		if (v & K2C_J_SPECIAL) {
			cur = (int)((v >> 16) & K2C_RANK);
			why = 1;
		} else
			cur = -1;
		if (nvis > K2_VIS_LIM(p)) {
			K2_COUNT(p, K2_DBG_ESC_VIS);
			atomicMin(p.fail + sc, 0);
		}
	}
	ks.walk[0] = cur;
	ks.walk[1] = last;
	ks.walk[2] = why;
}

/* 4. publish the visited clusters: list positions come from LDS counters seeded with what the
 *    serial stretches and the walk already listed; the global counters are written once.  Behind it ks.cnt[0..2] hold what the
 *    clusters counted (triggers, rejects, bursts) and ks.walk[3] the entries of the visited list. */
__device__ __forceinline__ void k2c_publish(const K2cShared &ks, const K2Params &p, int sc, int tid, const MachCtx &cx, bool lazy, int seg_from, int nvis,
					    bool tables_ok, int nslog)
{
	unsigned short *const sw16 = reinterpret_cast<unsigned short *>(ks.swalk);	/* (hop i of rank j: sw16[4 j + i]) */
	const bool first_pass = p.round == 0;
	const int t_end = (int)(cx.avail_end - cx.dec_base);
	uint8_t *const onchain = p.onchain + (size_t)sc * VDL2_CAND_CAP;
	Seg *segs = p.segs + (size_t)sc * VDL2_SEG_CAP;
	unsigned *nseg = p.ctl + CTL_NSEG0(p) + sc;
	if (tid < 4)
		ks.cnt[tid] = 0;
	if (tid == 0) {
		ks.walk[0] = (int)*cx.nsel;
		ks.walk[1] = (int)*nseg;
		ks.walk[3] = nvis < K2_VIS_LIM(p) ? nvis : K2_VIS_LIM(p);
	}
	__syncthreads();
	int a = 0, b = 0, d = 0;
	const int nv4 = ks.walk[3] * 4;
	for (int t = tid; t < nv4; t += K2_NT) {
		const unsigned ve = ks.svis[t >> 2];
		int j = -1;
		if (ve & 0x8000u)
			j = (t & 3) == 0 ? (int)(ve & K2C_RANK) : -1;
		else {
			const unsigned hop = (unsigned)(ks.swalk[ve] >> (16 * (t & 3))) & 0xffffu;
			if (hop != K2C_HOP_NONE && (hop >> K2C_RBITS) == CL_STEADY)
				j = (int)(hop & K2C_RANK);
		}
		if (j >= 0) {
			const unsigned gidx = p.sidx[(size_t)sc * VDL2_CAND_CAP + j];	/* (from device memory: a lane each, all in flight together) */
			const int2 hd = p.clhead[(size_t)sc * VDL2_CAND_CAP + gidx];
			if (first_pass)
				onchain[gidx] = 1;	/* invariant (a) at CTL_NWIN0: exactly the clusters selected and counted here (and the k2c_resolve loop's) */
			const unsigned hop0 = sw16[4 * j];
			const int next_t = (hop0 == K2C_HOP_NONE) ? t_end : (ks.skey[hop0 & K2C_RANK] >> 2);	/* the successor's trigger, or the end of the data */
			const int ns = cl_nslots(hd);
			const unsigned slot0 = (unsigned)(((size_t)sc * VDL2_CAND_CAP + gidx) * VDL2_CL_MAXB);
			if (ns)
				k2_select_slots(p, cx.sel, &ks.walk[0], slot0, ns);
			a += cl_ntrig(hd);
			b += cl_nrej(hd);
			d += cl_nburst(hd);
			/* after a steady cluster the chain idles in class (r_s, parity of n_s) until
			 * the successor's trigger (or the end of the data) */
			if (lazy && stat4_status(ks.sstat[j]) == CL_STEADY && k2_unprobed(p, cl_r(hd), cx.dec_base + hd.x) && next_t > seg_from &&
			    !k2_emit_seg(p, segs, (unsigned)atomicAdd(&ks.walk[1], 1), hd.x, next_t, cl_r(hd)))
				atomicMin(p.fail + sc, 0);
		}
	}
	if (a)
		atomicAdd(&ks.cnt[0], a);
	if (b)
		atomicAdd(&ks.cnt[1], b);
	if (d)
		atomicAdd(&ks.cnt[2], d);
	__syncthreads();
	if (tid == 0) {
		*cx.nsel = (unsigned)ks.walk[0];
		*nseg = (unsigned)ks.walk[1];
		/* the output records of the selected bursts, reserved in one piece: K2d's workgroups (one per burst) then need no
		 * atomic of their own -- a thousand of them asking one device-scope counter for a slot at the same moment took 80 us,
		 * more than decoding the bursts (the same effect as in k4_frames) */
		/* Only the FIRST pass reserves here: every record it reserves is written (K2d's first pass decodes every channel's first
		 * selection, void or not).  A repair round's selection may be superseded by the next round's or by K2f's serial redo --
		 * records reserved for it would stay unwritten: whatever an earlier push left in the ring there would be handed out
		 * as bursts [found by scripts/soak.py's dropped-region-scan modes: two rounds, or a round and a redo].  The repaired
		 * selection's records are reserved by K2f, when it is final. */
		if (ks.walk[0] > 0 && p.sel_reserved && p.round == 0)
			p.ctl[CTL_SELBASE0(p) + sc] = atomicAdd(&p.outc->records, (unsigned)ks.walk[0]);
		if (first_pass)
			p.ctl[CTL_NSLOG0(p) + sc] = (unsigned)(tables_ok ? nslog : K2_SLOG_LIM(p) + 1);	/* (no tables: nothing a local repair could stand on) */
		if (first_pass && tables_ok && nslog > K2_SLOG_LIM(p))
			K2_COUNT(p, K2_DBG_ESC_SLOG);
	}
	__syncthreads();
}

__global__ __launch_bounds__(K2_NT)
void k2c_resolve(K2Params p)
{
	__shared__ MachSharedT<K2_NT> sh;
	__shared__ int skey[VDL2_CAND_CAP], sx[VDL2_CAND_CAP], s_walk[4], s_cnt[4], coff[9], s_wcnt[K2_NT / 64][8];
	__shared__ unsigned sjump[VDL2_CAND_CAP];
	__shared__ unsigned long long swalk[VDL2_CAND_CAP];
	__shared__ unsigned short svis[K2C_VIS], clist[VDL2_CAND_CAP];
	__shared__ uint8_t sstat[VDL2_CAND_CAP];
	const K2cShared ks = {skey, sstat, svis, sjump, sx, s_walk, s_cnt, clist, swalk, coff, s_wcnt};
#ifndef K2C_PRIO
#define K2C_PRIO 3
#endif
	__builtin_amdgcn_s_setprio(K2C_PRIO);	/* one workgroup per channel beside the channeliser's thousands of waves */
	const int tid = threadIdx.x;
	const int c = blockIdx.x, s = (int)blockIdx.y;
	const int sc = s * VDL2_CS + c;
	int seg_from = -0x7fffffff;	/* repair round: stretches that end at or before the earliest event the verify pass found lie on the unchanged
					 * part of the chain and have been verified -- only what lies behind is listed again */
	if (p.round > 0) {
		const int fail_in = p.fail[sc];
		if (fail_in >= VDL2_VERIFIED)
			return;		/* verified in the first pass: nothing to repair */
		seg_from = fail_in;
		__syncthreads();
		if (tid == 0) {
			p.fail[sc] = 0x7f7f7f7f;	/* the repair pass is verified afresh */
			k2_begin_repair(p, sc, VDL2_WIN_ALL);	/* resolved again from the input state: nothing of the first selection stands */
		}
		__syncthreads();
	}
	const ChanState *cs = p.cs + sc;	/* input state: left untouched until K2f commits */
	ChanState *cs_out = p.cs_out + sc;
	MachCtx cx;
	mach_ctx(cx, p, s, c, true);	/* bursts of serial stretches become descriptors too */
	cx.sel = (p.round > 0 ? p.sel_list2 : p.sel_list) + (size_t)sc * VDL2_SEL_CAP;
	cx.nsel = p.ctl + (p.round > 0 ? CTL_NSEL1(p) : CTL_NSEL0(p)) + sc;
	MachState st = mach_state(cs);
	const bool lazy = !p.full_scan && !p.full_round;	/* (a full round's tables hold every class: nothing is left to verify) */
	mach_init_taps(sh);
	mach_load(sh, cs);
	MachOut out;
	mach_out_clear(out);
	unsigned long long n_slow = 0;
	int ncand = (int)p.ctl[CTL_CAND0 + sc];
	const bool tables_ok = !p.force_serial && ncand <= VDL2_CAND_CAP && p.ctl[CTL_CANDOVF0(p) + sc] == 0;
	if (!tables_ok)
		ncand = 0;
	/* What a local repair (k2p_patch) needs of this pass: which candidates the chain met in the history-free state (a repaired
	 * stretch that arrives at one of them has rejoined this chain), and what the serial stretches counted (no cluster head has it). */
	uint8_t *const onchain = p.onchain + (size_t)sc * VDL2_CAND_CAP;
	K2Slog *const slog = p.slog + (size_t)sc * VDL2_SLOG_CAP;
	int nslog = 0;
	const bool first_pass = p.round == 0;
	if (first_pass)
		for (int i = tid; i < (ncand + 3) / 4; i += K2_NT)
			reinterpret_cast<uint32_t *>(onchain)[i] = 0u;
	const long long pos_in = st.pos;
	const long long tk0 = wall_clock64();
	/* 1. the candidates as K2s sorted them by time, and of each one's cluster what the walk reads.  (Written here, on the arrays themselves:
	 *    as a function on `ks` the compiler picks other induction variables for this loop and the kernel has one LDS store more.) */
	const int2 *head = p.clhead + (size_t)sc * VDL2_CAND_CAP;
	for (int i = tid; i < ncand; i += K2_NT) {
		const int idx = p.sidx[(size_t)sc * VDL2_CAND_CAP + i];
		skey[i] = p.skey[(size_t)sc * VDL2_CAND_CAP + i];
		const int2 hd = head[idx];
		sx[i] = hd.x;
		sstat[i] = cl_stat4(hd);
	}
	__syncthreads();
	k2c_class_lists(ks, tid, ncand);
	const long long tk1 = wall_clock64();
	k2c_successors(ks, tid, ncand);
	k2c_four_hops(ks, tid, ncand);
	const long long tk2 = wall_clock64();
	bool steady_end = false;
	int nvis = 0;	/* slots of svis[] in use (thread 0's copy counts) */
	bool replay = false;	/* a cluster K2b did not make (CL_INVALID) is replayed here, from its candidate's instant */
	for (;;) {
		if (!tables_ok || st.fresh < VDL2_STEADY || replay) {
			/* history-dependent stretch (or no tables): serial machine.  (ONE call site: inlined into the kernel,
			 * its context stays in registers; with two the compiler made it a function and passed MachCtx /
			 * MachState / MachOut through 264 bytes of scratch per lane.)  A replay runs until the detector is
			 * history-free again behind at least one more trigger than the push has counted so far (a plain 1
			 * returned at once, without progress, when an earlier trigger had been counted). */
			const long long p0 = st.pos;
			const int c_trig = out.ntrig, c_rej = out.nrej, c_burst = out.nburst;
			const int rc = machine_run<K2_NT, false>(sh, cx, st, tables_ok, replay ? out.ntrig + 1 : 0, 1 << 30, replay ? 1 : 0, out);
			if (!replay)
				n_slow += (unsigned long long)(st.pos - p0);
			if (first_pass && tables_ok && (out.ntrig != c_trig || out.nrej != c_rej || out.nburst != c_burst)) {
				if (tid == 0 && nslog < K2_SLOG_LIM(p))
					slog[nslog] = K2Slog{(int)(p0 - cx.dec_base), out.ntrig - c_trig, out.nrej - c_rej, out.nburst - c_burst};
				++nslog;
			}
			replay = false;
			if (rc != MR_STEADY)
				break;
			continue;
		}
		if (tid == 0)	/* history-free */
			k2c_walk(ks, p, sc, cx, st, lazy, seg_from, nvis);
		__syncthreads();
		const int cur = ks.walk[0], last = ks.walk[1], why = ks.walk[2];
		__syncthreads();
		if (last >= 0) {
			st.pos = cx.dec_base + ks.sx[last];
			st.r = stat4_r(ks.sstat[last]);
		}
		if (!why) {
			mach_idle_to_end(cx, st);
			steady_end = true;
			break;
		}
		const long long ncand_t = cx.dec_base + (ks.skey[cur] >> 2);
		const Cluster *cl = p.clusters + (size_t)sc * VDL2_CAND_CAP + p.sidx[(size_t)sc * VDL2_CAND_CAP + cur];
		const int status = stat4_status(ks.sstat[cur]);
		if (first_pass && tid == 0)	/* (the chain met this candidate history-free too: whatever its cluster is, what follows is determined) */
			onchain[p.sidx[(size_t)sc * VDL2_CAND_CAP + cur]] = 1;
		if (status == CL_DEFER_FIRST) {
			st.pos = ncand_t;
			out.ndefer++;
			steady_end = true;
			break;
		}
		if (status == CL_INVALID) {
			/* no cluster for this candidate (not a primary, or the staging pool was full): replay the stretch at the top of the loop */
			st.pos = ncand_t;
			mach_materialize<K2_NT, false>(sh, cx, st.pos, st.r);
			replay = true;
			if (tid == 0 && p.dbg)
				atomicAdd(p.dbg + K2_DBG_K2C_REPLAYS, 1ull);	/* replays of clusters K2b did not make */
			continue;
		}
		/* CL_NONSTEADY: its bursts count, then continue from the explicit state it stopped in */
		if (tid == 0) {
			if (nvis < K2_VIS_LIM(p))
				ks.svis[nvis] = (unsigned short)(cur | 0x8000);
			else {
				K2_COUNT(p, K2_DBG_ESC_VIS);
				atomicMin(p.fail + sc, 0);
			}
			++nvis;
		}
		if (tid == 0 && p.dbg)
			atomicAdd(p.dbg + K2_DBG_K2C_NONSTEADY, 1ull);	/* non-steady clusters continued serially */
		mach_resume(sh, st, &cl->saved);
	}
	__syncthreads();
	/* A burst of a serial stretch or a replay that found the descriptor pool or the selection list full is in the counters but has no
	 * descriptor K2d could decode: the pass cannot stand -- the channel fails (as in k2b_clusters and k2p_patch) and K2f, which writes its
	 * records itself and needs no descriptor, redoes it.  Counted, never silent. */
	if (out.badslot && tid == 0) {
		K2_COUNT(p, K2_DBG_ESC_STAGE);
		atomicMin(p.fail + sc, 0);
	}
	const long long tk3 = wall_clock64();
	k2c_publish(ks, p, sc, tid, cx, lazy, seg_from, nvis, tables_ok, nslog);
	if (steady_end) {
		mach_materialize<K2_NT, false>(sh, cx, st.pos, st.r);
		st.fresh = VDL2_STEADY;
	}
	__syncthreads();
	mach_store(sh, st, cs_out);
	if (tid == 0) {
		cs_out->n_eval = cs->n_eval + (unsigned long long)((st.pos - pos_in) / 2);	/* evaluation instants covered */
		cs_out->n_trig = cs->n_trig + (unsigned long long)(out.ntrig + ks.cnt[0]);
		cs_out->n_reject = cs->n_reject + (unsigned long long)(out.nrej + ks.cnt[1]);
		cs_out->n_burst = cs->n_burst + (unsigned long long)(out.nburst + ks.cnt[2]);
		cs_out->n_defer = cs->n_defer + (unsigned long long)out.ndefer;
		cs_out->n_slow = cs->n_slow + n_slow;
		cs_out->n_cand = cs->n_cand + (unsigned long long)ncand;
		cs_out->n_redo = cs->n_redo;
		if (p.dbg) {
			const long long tk4 = wall_clock64();
			atomicAdd(p.dbg + K2_DBG_K2C_LOAD_TICKS, (unsigned long long)(tk1 - tk0));
			atomicAdd(p.dbg + K2_DBG_K2C_TABLES_TICKS, (unsigned long long)(tk2 - tk1));
			atomicAdd(p.dbg + K2_DBG_K2C_WALK_TICKS, (unsigned long long)(tk3 - tk2));
			atomicAdd(p.dbg + K2_DBG_K2C_PUBLISH_TICKS, (unsigned long long)(tk4 - tk3));
			atomicAdd(p.dbg + K2_DBG_K2C_CALLS, 1ull);
			atomicAdd(p.dbg + K2_DBG_K2C_CANDS, (unsigned long long)ncand);
			atomicAdd(p.dbg + K2_DBG_K2C_VISITED, (unsigned long long)ks.walk[3]);	/* visited-list entries */
			atomicAdd(p.dbg + K2_DBG_K2C_SERIAL_SAMPLES, n_slow);
		}
	}
}

/* ====================================================================== K2p
 * Local repair (the first repair round).  The verify pass found detector events the tables lacked -- a noise trigger that exists
 * in one timing class only, once per hundred channel-seconds of ordinary traffic: most pushes have one somewhere -- and listed them
 * as candidates without clusters.  Until round 5 the round re-resolved the failing channel from the START of the push (k2s_merge,
 * k2c_resolve with a CU's whole LDS, a verify pass over everything behind the event, every payload decoded again: 0.3 ms on the
 * tail of every push, and the chain resolver -> verify -> round -> commit -> next push's resolver was the period).  But the chain
 * is a deterministic function of where the detector stands: the event lies in a stretch the old chain IDLED through history-free
 * (that is what the verify pass scans), so up to the event the old chain stands; from the event on the new chain is followed --
 * the event replayed by the serial machine, then cluster by cluster through the tables -- until it arrives, history-free, at a
 * candidate the OLD chain also met history-free (K2Params.onchain): from there on the two are the same chain again.  A burst or
 * two as a rule (the class a burst leaves the detector in depends on the burst, hardly on the class it was met in).
 *   What changes is confined to the WINDOW [event, rejoin): the old chain's bursts triggered inside it are void (CTL_NWIN0 /
 *   K2Params.win: K2d's second pass tags their records), the new chain's bursts there are the repair's selection (sel_list2), the
 *   stretches the new chain idles through inside it are what the round's verify pass scans, the counters move by the difference.
 *   A new chain that does not rejoin before the data end leaves the channel state itself (the window runs to the end).
 * One workgroup per channel, tables read from device memory where they lie (a hop is three or four dependent reads; the windows
 * are a few hops): 8 KB of LDS where the resolver wants 157 -- a workgroup that wants a CU's whole LDS waits for a wide kernel
 * of another push to END.  What this kernel cannot do locally -- tables unusable, more new candidates than K2S_MERGE, more windows
 * than VDL2_WIN_CAP, a first pass with more serial stretches than its log holds -- it leaves failed: a further round resolves the
 * channel from its input state as before (k2s_merge + k2c_resolve), or K2f redoes it serially.
 * Match: d8psk.c:292-313 (what a trigger changes), 97-107 (a rejected header), 317-319 (the sub-phase sticks). */
#define K2P_NT K2_NT
#ifdef K2P_TRACE
#define K2P_TR(...) do { if (tid == 0 && sc == K2P_TRACE) printf(__VA_ARGS__); } while (0)
#else
#define K2P_TR(...) do { } while (0)
#endif
struct K2pShared {
	MachSharedT<K2P_NT> m;
	unsigned long long knew[K2S_MERGE];	/* the new candidates by time: (nrel * 4 + r) << 16 | index */
	int2 win[VDL2_WIN_CAP];
	union {
		K2xWork xw;			/* (while the verify pass's common area is drained) */
		int red[3][K2P_NT / 64];
	} u;
};

/* first rank of the sorted table whose key is >= key (wave-parallel 64-ary search: three rounds for 6144 entries) */
__device__ __forceinline__ int k2p_lower_bound(const int *skey, int n, int key)
{
	const int lane = threadIdx.x & 63;
	int lo = 0, hi = n;
	while (hi > lo) {
		const int step = (hi - lo + 63) / 64;
		const int j = lo + lane * step;
		const bool ge = j >= hi || skey[j] >= key;
		const unsigned long long m = __ballot(ge);
		const int f = m ? __builtin_ctzll(m) : 64;
		if (f == 0) {
			hi = lo;
			break;
		}
		const int nhi = lo + f * step < hi ? lo + f * step : hi;
		lo = lo + (f - 1) * step + 1;
		hi = nhi;
	}
	return lo;
}

/* first entry >= from of a list of n keys (key_at(j) = nrel * 4 + r, ascending) with time >= want in class cls (sub-phase * 2 + parity
 * of the time); n if none.  The sorted table in device memory, or the new candidates in LDS */
template <class KeyAt> __device__ __forceinline__ int k2p_next(KeyAt key_at, int from, int n, int want, int cls)
{
	const int lane = threadIdx.x & 63;
	for (int b = from; b < n; b += 64) {
		const int j = b + lane;
		const int k = j < n ? key_at(j) : 0;
		const int t = k >> 2;
		const bool hit = j < n && t >= want && ((k & 3) * 2 + (t & 1)) == cls;
		const unsigned long long m = __ballot(hit);
		if (m)
			return b + __builtin_ctzll(m);
	}
	return n;
}

/* the new candidates (nold .. nold + nnew - 1 of the table) by time into knew[]: every one finds its rank by counting (there are a handful) */
__device__ __forceinline__ void k2p_rank_new(unsigned long long *knew, const Cand *cands, int nold, int nnew, int tid)
{
	for (int i = tid; i < nnew; i += K2P_NT) {
		const unsigned long long v = (((unsigned long long)(unsigned)(cands[nold + i].nrel * 4 + cands[nold + i].r)) << 16) | (unsigned)(nold + i);
		int at = 0;
		for (int j = 0; j < nnew; ++j) {
			const unsigned long long w = (((unsigned long long)(unsigned)(cands[nold + j].nrel * 4 + cands[nold + j].r)) << 16) | (unsigned)(nold + j);
			at += (w < v) ? 1 : 0;
		}
		knew[at] = v;
	}
}

/* what the OLD chain counted inside the nwin windows of ps.win[]: the clusters it met there (their heads: invariant (a) at CTL_NWIN0), the
 * serial stretches it began there (K2Params.slog).  Every thread returns the workgroup's sums: x triggers, y rejects, z bursts */
__device__ __forceinline__ int3 k2p_old_counts(K2pShared &ps, const K2Params &p, int sc, int tid, int nwin, int nold, unsigned nslog_in)
{
	const int *skey = p.skey + (size_t)sc * VDL2_CAND_CAP;
	const unsigned short *sidx = p.sidx + (size_t)sc * VDL2_CAND_CAP;
	const int2 *heads = p.clhead + (size_t)sc * VDL2_CAND_CAP;
	const uint8_t *onchain = p.onchain + (size_t)sc * VDL2_CAND_CAP;
	int sub_trig = 0, sub_rej = 0, sub_burst = 0;
	for (int w = 0; w < nwin; ++w) {
		const int2 wn = ps.win[w];
		const int r_lo = k2p_lower_bound(skey, nold, wn.x * 4);
		const int r_hi = wn.y == 0x7fffffff ? nold : k2p_lower_bound(skey, nold, wn.y * 4);
		for (int j = r_lo + tid; j < r_hi; j += K2P_NT) {
			const int idx = sidx[j];
			if (onchain[idx]) {
				const int2 hd = heads[idx];
				sub_trig += cl_ntrig(hd);
				sub_rej += cl_nrej(hd);
				sub_burst += cl_nburst(hd);
			}
		}
		if (tid < (int)nslog_in) {
			const K2Slog g = p.slog[(size_t)sc * VDL2_SLOG_CAP + tid];
			if (g.t >= wn.x && g.t < wn.y) {
				sub_trig += g.ntrig;
				sub_rej += g.nrej;
				sub_burst += g.nburst;
			}
		}
	}
	for (int d = 32; d > 0; d >>= 1) {
		sub_trig += __shfl_xor(sub_trig, d, 64);
		sub_rej += __shfl_xor(sub_rej, d, 64);
		sub_burst += __shfl_xor(sub_burst, d, 64);
	}
	if ((tid & 63) == 0) {
		ps.u.red[0][tid >> 6] = sub_trig;
		ps.u.red[1][tid >> 6] = sub_rej;
		ps.u.red[2][tid >> 6] = sub_burst;
	}
	__syncthreads();
	int3 sub = make_int3(0, 0, 0);
	for (int w = 0; w < K2P_NT / 64; ++w) {
		sub.x += ps.u.red[0][w];
		sub.y += ps.u.red[1][w];
		sub.z += ps.u.red[2][w];
	}
	return sub;
}

#ifdef VDL2GPU_TESTHOOKS
/* test build, invariant (a) at CTL_NWIN0, when a window [x, y) is closed: lane 0 walks the channel's first selection; a burst of a cluster
 * K2b made (a static descriptor slot) that was triggered inside the window must belong to a candidate marked in onchain[] */
__device__ __forceinline__ void k2p_check_onchain(const K2Params &p, int sc, int x, int y)
{
	if (threadIdx.x != 0 || !p.dbg)
		return;
	const unsigned dyn_base = (unsigned)p.nstreams * VDL2_CS * VDL2_CAND_CAP * VDL2_CL_MAXB;
	const unsigned *sel0 = p.sel_list + (size_t)sc * VDL2_SEL_CAP;
	unsigned n0 = p.ctl[CTL_NSEL0(p) + sc];
	n0 = n0 > VDL2_SEL_CAP ? VDL2_SEL_CAP : n0;
	for (unsigned i = 0; i < n0; ++i) {
		const unsigned slot = sel0[i];
		if (slot >= dyn_base)
			continue;	/* (a serial stretch's burst: no cluster) */
		const long long t = p.stage[slot].nstar - p.dec_base;
		if (t >= x && t < y) {
			K2_COUNT(p, K2_DBG_CHK_A);
			if (!p.onchain[slot / VDL2_CL_MAXB])
				K2_COUNT(p, K2_DBG_INV_A);
		}
	}
}
#endif

__global__ __launch_bounds__(K2P_NT)
void k2p_patch(K2Params p)
{
	__shared__ K2pShared ps;
	MachSharedT<K2P_NT> &sh = ps.m;
	const int tid = threadIdx.x;
	const int c = blockIdx.x, s = (int)blockIdx.y;
	const int sc = s * VDL2_CS + c;
	if (p.force_serial)
		return;
	k2x_drain<K2P_NT>(ps.u.xw, p, sc);	/* the common area of the verify pass in front: what it finds there fails the channel like any other hit */
	const int fail_in = p.fail[sc];
	if (fail_in >= VDL2_VERIFIED)
		return;		/* verified in the first pass: nothing to repair */
	__syncthreads();
	const int ncand = (int)p.ctl[CTL_CAND0 + sc];
	const unsigned ovf_in = p.ctl[CTL_CANDOVF0(p) + sc];
	const int nold = (int)p.ctl[CTL_NCLUST0(p) + sc], nnew = ncand - nold;
	const unsigned nslog_in = p.ctl[CTL_NSLOG0(p) + sc];
	if (tid == 0)
		k2_begin_repair(p, sc, 0);	/* (the windows are listed at the end) */
	/* what cannot be repaired locally stays failed (fail[] keeps its value): the next round, or K2f, takes the channel from its input state */
	/* fail_in <= 0 is not an event's instant: the verify pass could not vouch for the channel (items refused by a full list, more stretches than
	 * the lists hold): stretches it was to look at have not been looked at, and a local repair verifies only what IT changes
	 * [found by scripts/soak.py on handles whose item lists are small: seeds 6064, 6068, 6077] */
	K2P_TR("k2p sc %d: fail_in %d ncand %d nold %d nslog %u ovf %u dec_base %lld\n", sc, fail_in, ncand, nold, nslog_in, ovf_in, (long long)p.dec_base);
	if (tid == 0 && ncand <= VDL2_CAND_CAP && ovf_in == 0) {	/* (with usable tables: what else refuses the repair) */
		if (nnew > K2_MERGE_LIM(p))
			K2_COUNT(p, K2_DBG_ESC_MERGE);
		if (nslog_in > (unsigned)K2_SLOG_LIM(p))
			K2_COUNT(p, K2_DBG_ESC_SLOG);
	}
	if (ncand > VDL2_CAND_CAP || ovf_in != 0 || nnew <= 0 || nnew > K2_MERGE_LIM(p) || nslog_in > (unsigned)K2_SLOG_LIM(p) || fail_in <= 0)
		return;
	__syncthreads();
	if (tid == 0)
		p.fail[sc] = 0x7f7f7f7f;	/* the repair is verified afresh */
	const ChanState *cs = p.cs + sc;	/* input state: left untouched until K2f commits */
	ChanState *cs_out = p.cs_out + sc;	/* the first pass's result: what this kernel amends */
	const Cand *cands = p.cands + (size_t)sc * VDL2_CAND_CAP;
	const int *skey = p.skey + (size_t)sc * VDL2_CAND_CAP;
	const unsigned short *sidx = p.sidx + (size_t)sc * VDL2_CAND_CAP;
	const int2 *heads = p.clhead + (size_t)sc * VDL2_CAND_CAP;
	const uint8_t *onchain = p.onchain + (size_t)sc * VDL2_CAND_CAP;
	const Cluster *clusters = p.clusters + (size_t)sc * VDL2_CAND_CAP;
	unsigned *sel = p.sel_list2 + (size_t)sc * VDL2_SEL_CAP;
	unsigned *nsel = p.ctl + CTL_NSEL1(p) + sc;
	Seg *segs = p.segs + (size_t)sc * VDL2_SEG_CAP;
	k2p_rank_new(ps.knew, cands, nold, nnew, tid);
	MachCtx cx;
	mach_ctx(cx, p, s, c, true);	/* bursts of serial stretches become descriptors */
	cx.sel = sel;
	cx.nsel = nsel;
	const int t_end = (int)(cx.avail_end - cx.dec_base);
	mach_init_taps(sh);	/* (barriers inside: knew[] is in place behind it) */
	MachOut out;
	mach_out_clear(out);
	MachState st = {0, 0, VDL2_STEADY};
	int add_trig = 0, add_rej = 0, add_burst = 0, add_defer = 0;	/* what the table clusters on the new chain count */
	int nwin = 0, nsegs = 0;
	int rk = 0;		/* rank of the old candidate the walk is looking at */
	int ev = 0;		/* next new candidate to look at */
	int t_cur = -0x7fffffff;	/* events before this lie inside a window already handled */
	bool to_end = false, steady_end = false, failed = false;
	/* mode of the one serial-machine call site below (two sites and the compiler makes it a function: see k2c_resolve) */
	enum { GO_WALK, GO_REPLAY, GO_SERIAL } go = GO_WALK;
	bool in_window = false;
	int win_lo = 0;
	for (;;) {
		if (!in_window) {
			/* the next event on the chain as it stands: the earliest new candidate behind the windows handled so far (it lies in
			 * a stretch the old chain idles through in its class: the verify pass found it there) */
			while (ev < nnew && (int)(ps.knew[ev] >> 18) < t_cur)
				++ev;
			if (ev >= nnew)
				break;
			const int key = (int)(ps.knew[ev] >> 16);
			++ev;
			win_lo = key >> 2;
			K2P_TR("  event %d r %d (t_cur %d)\n", key >> 2, key & 3, t_cur);
			in_window = true;
			st.pos = cx.dec_base + win_lo;
			st.r = key & 3;
			st.fresh = VDL2_STEADY;
			go = GO_REPLAY;
		}
		if (go != GO_WALK) {
			if (go == GO_REPLAY)
				mach_materialize<K2P_NT, false>(sh, cx, st.pos, st.r);
			const bool replay = go == GO_REPLAY;
			const int rc = machine_run<K2P_NT, false>(sh, cx, st, true, replay ? out.ntrig + 1 : 0, 1 << 30, replay ? 1 : 0, out);
			go = GO_WALK;
			K2P_TR("  machine rc %d -> pos %lld r %d fresh %d ntrig %d nburst %d ndefer %d\n", rc, (long long)(st.pos - cx.dec_base), st.r, st.fresh, out.ntrig, out.nburst, out.ndefer);
			if (rc != MR_STEADY) {	/* the data end (or a deferred burst) inside a history-dependent stretch: the channel state is the machine's */
				to_end = true;
				break;
			}
		}
		/* history-free at (st.pos, st.r): the next event is the first candidate of that class at or behind st.pos, old or new */
		const int want = (int)(st.pos - cx.dec_base), cls = st.r * 2 + (want & 1);
		/* (the search starts at the first entry at or behind `want` whatever its class: the hit of one class says nothing about where the
		 * candidates of the class the chain is in after the NEXT burst lie -- round 6's first version went on from the hit and, once a class
		 * had no further candidate, found none of any class: scripts/soak.py seed 6068) */
		rk = k2p_next([&](int j) { return skey[j]; }, k2p_lower_bound(skey, nold, want * 4), nold, want, cls);
		const int jn = k2p_next([&](int j) { return (int)(ps.knew[j] >> 16); }, 0, nnew, want, cls);
		const int t_old = rk < nold ? (skey[rk] >> 2) : 0x7fffffff;
		const int t_new = jn < nnew ? (int)(ps.knew[jn] >> 18) : 0x7fffffff;
		const int t_next = t_old < t_new ? t_old : t_new;
		K2P_TR("  walk at %d r %d cls %d: t_old %d (rk %d) t_new %d\n", want, st.r, cls, t_old, rk, t_new);
		if (k2_unprobed(p, st.r, st.pos)) {
			/* the new chain idles from here to that candidate in a class the probe did not scan: the round's verify pass looks */
			const int g_hi = t_next < t_end ? t_next : t_end;
			if (g_hi > want) {
				if (nsegs < K2_SEG_LIM(p)) {
					if (tid == 0)
						segs[nsegs] = Seg{want, g_hi, st.r, 0};
				} else {
					if (tid == 0)
						K2_COUNT(p, K2_DBG_ESC_SEG);
					failed = true;
				}
				++nsegs;
			}
		}
		if (t_next == 0x7fffffff) {
			mach_idle_to_end(cx, st);
			steady_end = true;
			to_end = true;
			break;
		}
		if (t_new < t_old) {	/* another new candidate: no cluster, replayed like the event */
			st.pos = cx.dec_base + t_new;
			go = GO_REPLAY;
			continue;
		}
		const int idx = sidx[rk];
		K2P_TR("  cand idx %d onchain %d\n", idx, (int)onchain[idx]);
		if (onchain[idx]) {
			/* the old chain met this candidate history-free as well: the same chain from here on */
			if (nwin < K2_WIN_LIM(p)) {
				if (tid == 0)
					ps.win[nwin] = make_int2(win_lo, t_old);
			} else {
				if (tid == 0)
					K2_COUNT(p, K2_DBG_ESC_WIN);
				failed = true;
			}
#ifdef VDL2GPU_TESTHOOKS
			k2p_check_onchain(p, sc, win_lo, t_old);
#endif
			++nwin;
			t_cur = t_old;
			in_window = false;
			continue;
		}
		const int2 hd = heads[idx];
		const int status = cl_status(hd);
		K2P_TR("  old cand idx %d status %d x %d\n", idx, status, hd.x);
		if (status == CL_INVALID) {
			st.pos = cx.dec_base + t_old;
			go = GO_REPLAY;
			continue;
		}
		if (status == CL_DEFER_FIRST) {	/* the burst is not completely inside the data held: the chain ends in front of its trigger */
			st.pos = cx.dec_base + t_old;
			add_defer++;
			steady_end = true;
			to_end = true;
			break;
		}
		/* a cluster K2b made: its bursts are on the new chain */
		const int ns = cl_nslots(hd);
		const unsigned slot0 = (unsigned)(((size_t)sc * VDL2_CAND_CAP + idx) * VDL2_CL_MAXB);
		if (tid == 0 && ns)
			k2_select_slots(p, sel, nsel, slot0, ns);	/* (the serial machine appends through the same counter) */
		add_trig += cl_ntrig(hd);
		add_rej += cl_nrej(hd);
		add_burst += cl_nburst(hd);
		if (status == CL_STEADY) {
			st.pos = cx.dec_base + hd.x;
			st.r = cl_r(hd);
			continue;
		}
		/* CL_NONSTEADY */
		__syncthreads();
		mach_resume(sh, st, &clusters[idx].saved);
		go = GO_SERIAL;
	}
	__syncthreads();
	K2P_TR(" end: to_end %d steady_end %d failed %d nwin %d nsegs %d pos %lld r %d\n", (int)to_end, (int)steady_end, (int)failed, nwin, nsegs, (long long)(st.pos - cx.dec_base), st.r);
	if (to_end) {	/* the last window runs to the end of the data */
		if (nwin < K2_WIN_LIM(p)) {
			if (tid == 0)
				ps.win[nwin] = make_int2(win_lo, 0x7fffffff);
		} else {
			if (tid == 0)
				K2_COUNT(p, K2_DBG_ESC_WIN);
			failed = true;
		}
#ifdef VDL2GPU_TESTHOOKS
		k2p_check_onchain(p, sc, win_lo, 0x7fffffff);
#endif
		++nwin;
	}
	if (out.badslot && tid == 0)
		K2_COUNT(p, K2_DBG_ESC_STAGE);
	if (out.badslot)
		failed = true;
	if (failed) {	/* more windows or stretches than the lists hold: not repaired */
		if (tid == 0)
			K2_COUNT(p, K2_DBG_ESC_PATCH_ABANDON);
		if (tid == 0) {
			atomicMin(p.fail + sc, 0);
			p.ctl[CTL_NSEL1(p) + sc] = 0;
			p.ctl[CTL_NSEG0(p) + sc] = 0;
		}
		return;
	}
	__syncthreads();
	const int3 sub = k2p_old_counts(ps, p, sc, tid, nwin, nold, nslog_in);
	for (int w = tid; w < nwin; w += K2P_NT)
		p.win[(size_t)sc * VDL2_WIN_CAP + w] = ps.win[w];
	/* old counters of the push as the first pass left them in cs_out (read before anything is stored) */
	const unsigned long long o_trig = cs_out->n_trig, o_rej = cs_out->n_reject, o_burst = cs_out->n_burst, o_cand = cs_out->n_cand;
	__syncthreads();
	if (to_end) {
		if (steady_end) {
			mach_materialize<K2P_NT, false>(sh, cx, st.pos, st.r);
			st.fresh = VDL2_STEADY;
		}
		__syncthreads();
		mach_store(sh, st, cs_out);
	}
	if (tid == 0) {
		p.ctl[CTL_NSEG0(p) + sc] = (unsigned)nsegs;
		p.ctl[CTL_NWIN0(p) + sc] = (unsigned)nwin;
		cs_out->n_trig = o_trig - (unsigned long long)sub.x + (unsigned long long)(add_trig + out.ntrig);
		cs_out->n_reject = o_rej - (unsigned long long)sub.y + (unsigned long long)(add_rej + out.nrej);
		cs_out->n_burst = o_burst - (unsigned long long)sub.z + (unsigned long long)(add_burst + out.nburst);
		cs_out->n_cand = o_cand + (unsigned long long)nnew;
		if (to_end) {
			cs_out->n_eval = cs->n_eval + (unsigned long long)((st.pos - cs->pos) / 2);
			cs_out->n_defer = cs->n_defer + (unsigned long long)(out.ndefer + add_defer);
		}
	}
}

/* ====================================================================== K2f
 * Commit.  If K2a-verify found nothing the resolver's result becomes the channel state.  If it
 * found a detector hit the tables did not contain, the channel's push is redone from its input
 * state by the serial machine alone (always exact; it writes its bursts itself) and the
 * resolver's selection for that channel is dropped.
 */
/* (k2f_commit_fb, below, is this kernel's text once more with the feedback rows: a change here is a change there) */
__global__ __launch_bounds__(K2_NT)
void k2f_commit(K2Params p)
{
	__shared__ MachSharedT<K2_NT> sh;
	__shared__ K2xWork xw;
	const int tid = threadIdx.x;
	const int c = blockIdx.x, s = (int)blockIdx.y;
	const int sc = s * VDL2_CS + c;
	ChanState *cs = p.cs + sc;
	k2x_drain<K2_NT>(xw, p, sc);	/* the common area of the last verify pass */
	if (p.fail[sc] >= VDL2_VERIFIED) {
		const uint32_t *src = reinterpret_cast<const uint32_t *>(p.cs_out + sc);
		uint32_t *dst = reinterpret_cast<uint32_t *>(cs);
		for (int i = tid; i < (int)(sizeof(ChanState) / 4); i += K2_NT)
			dst[i] = src[i];
		/* a channel the repair rounds re-resolved: its selection is final now -- the records K2d's second pass fills */
		if (tid == 0 && p.sel_reserved && k2_fmask_test(p, sc)) {
			const unsigned n = p.ctl[CTL_NSEL1(p) + sc];
			if (n > 0)
				p.ctl[CTL_SELBASE1(p) + sc] = atomicAdd(&p.outc->records, n > VDL2_SEL_CAP ? VDL2_SEL_CAP : n);
		}
		return;
	}
	MachCtx cx;
	mach_ctx(cx, p, s, c, false);
	MachState st = mach_state(cs);
	const long long p0 = st.pos;
	mach_init_taps(sh);
	mach_load(sh, cs);
	MachOut out;
	mach_out_clear(out);
	machine_run<K2_NT, false>(sh, cx, st, false, 0, 1 << 30, 0, out);
	__syncthreads();
	mach_store(sh, st, cs);
	if (tid == 0) {
		cs->n_eval += (unsigned long long)out.neval;
		cs->n_trig += (unsigned long long)out.ntrig;
		cs->n_reject += (unsigned long long)out.nrej;
		cs->n_burst += (unsigned long long)out.nburst;
		cs->n_defer += (unsigned long long)out.ndefer;
		cs->n_slow += (unsigned long long)(st.pos - p0);
		cs->n_redo += 1;
		atomicAdd(&p.outc_total->redo, 1u);
		p.ctl[CTL_NSEL1(p) + sc] = 0;	/* K2d: nothing of the resolver's for this channel (it is masked: K2d reads the repair rounds' selection) ... */
		p.ctl[CTL_NWIN0(p) + sc] = VDL2_WIN_ALL;
		p.redo[sc] = 1;			/* (... also where the mask does not reach: K2d's one pass behind the commit asks this word) */
		k2_fmask_set(p, sc);		/* ... and if K2d ran ahead of the verify pass, the host drops what it made of it */
	}
}

/* VDL2GPU_F_FEEDBACK: k2f_commit again, statement for statement, with the one difference that the serial machine also writes every
 * record's decision-feedback rows, fb[slot] (machine_run<.., true>, burst_payload_feedback).  A kernel of its own text, not a body the
 * two share: called through a shared function k2f_commit compiles to other registers (226 VGPRs and 264 scalar spills for 234 and
 * 258), and what a handle without the flag runs stays what it was.  tests/test_gpu_feedback.py holds the two against each other:
 * the records and every other column of a redone channel are those of a handle without the flag. */
__global__ __launch_bounds__(K2_NT)
void k2f_commit_fb(K2Params p, vdl2gpu_fb_t *fb)
{
	__shared__ MachSharedT<K2_NT> sh;
	__shared__ K2xWork xw;
	const int tid = threadIdx.x;
	const int c = blockIdx.x, s = (int)blockIdx.y;
	const int sc = s * VDL2_CS + c;
	ChanState *cs = p.cs + sc;
	k2x_drain<K2_NT>(xw, p, sc);
	if (p.fail[sc] >= VDL2_VERIFIED) {
		const uint32_t *src = reinterpret_cast<const uint32_t *>(p.cs_out + sc);
		uint32_t *dst = reinterpret_cast<uint32_t *>(cs);
		for (int i = tid; i < (int)(sizeof(ChanState) / 4); i += K2_NT)
			dst[i] = src[i];
		if (tid == 0 && p.sel_reserved && k2_fmask_test(p, sc)) {
			const unsigned n = p.ctl[CTL_NSEL1(p) + sc];
			if (n > 0)
				p.ctl[CTL_SELBASE1(p) + sc] = atomicAdd(&p.outc->records, n > VDL2_SEL_CAP ? VDL2_SEL_CAP : n);
		}
		return;
	}
	MachCtx cx;
	mach_ctx(cx, p, s, c, false);
	MachState st = mach_state(cs);
	const long long p0 = st.pos;
	mach_init_taps(sh);
	mach_load(sh, cs);
	MachOut out;
	mach_out_clear(out);
	machine_run<K2_NT, false, true>(sh, cx, st, false, 0, 1 << 30, 0, out, fb);
	__syncthreads();
	mach_store(sh, st, cs);
	if (tid == 0) {
		cs->n_eval += (unsigned long long)out.neval;
		cs->n_trig += (unsigned long long)out.ntrig;
		cs->n_reject += (unsigned long long)out.nrej;
		cs->n_burst += (unsigned long long)out.nburst;
		cs->n_defer += (unsigned long long)out.ndefer;
		cs->n_slow += (unsigned long long)(st.pos - p0);
		cs->n_redo += 1;
		atomicAdd(&p.outc_total->redo, 1u);
		p.ctl[CTL_NSEL1(p) + sc] = 0;
		p.ctl[CTL_NWIN0(p) + sc] = VDL2_WIN_ALL;
		p.redo[sc] = 1;
		k2_fmask_set(p, sc);
	}
}

/* ====================================================================== K2d
 * Payload decode of the bursts that lie on the real chain: one workgroup per
 * selected burst descriptor, one lane per byte.
 */
#define K2D_NT 256
#ifndef K2D_WAVES
#define K2D_WAVES 5	/* 91 registers, no spill (round 4: 119 / four wavefronts -- with the table paths a run-time choice the kernel carried the
			 * code and the scalar registers of the paths it never takes: burst_payload<NT, TAB>) */
#endif
/* LEV (VDL2GPU_F_LEVELS): behind every burst its first wavefront measures the levels (burst_payload_levels) -- a kernel of its own,
 * k2d_payload_lev, with the registers it needs (four wavefronts): k2d_payload sits at the edge of its five and spilled with the pass
 * inlined; it carries none of it */
/* SOFT (VDL2GPU_F_SOFT_RS): behind every burst all its lanes write the reliability map from the phases still in sph
 * (burst_payload_soft) -- k2d_payload_soft, and k2d_payload_lev_soft with both flags */
/* CAR (VDL2GPU_F_CARRIER): behind every burst one lane per symbol adds up the slices' distance from their sectors' centres, again
 * from the phases in sph (burst_payload_carrier) -- four kernels more, k2d_payload*_car, so that the four above keep their code */
/* FB (VDL2GPU_F_FEEDBACK): behind every burst its symbols are sliced a second time with the residuals of the last three fed back
 * (burst_payload_feedback: the indices go where the phases were, one byte a symbol, so it comes last) -- eight kernels more,
 * k2d_payload*_fb, so that the eight above keep their code.  The rows' ring (fb, one vdl2gpu_fb_t per record slot of p.recs) is a
 * second kernel argument, not a member of K2Params: the parameter block of every kernel that never reads them stays what it was */
template <bool LEV, bool SOFT, bool CAR = false, bool FB = false> __device__ __forceinline__ void k2d_run(const K2Params &p, vdl2gpu_fb_t *fb = nullptr)
{
	__shared__ unsigned s_slot;
	__shared__ int s_car[2];	/* (CAR only: the burst's two sums) */
	__shared__ int s_fb[1];		/* (FB only: the burst's sum of residuals) */
	__shared__ float sph[VDL2_MAXSYM];
	__shared__ float s_tabs[72 + VDL2_ATAN_ROWS * VDL2_ATAN_STRIDE + 3 * 257];	/* mflt[], atanf range table, Grey1/2/3 (see burst_payload) */
	const int sc = (int)blockIdx.y;	/* stream * VDL2_CS + channel slot, like everywhere else: the grid spans all VDL2_CS slots of every stream */
	if ((sc % VDL2_CS) >= p.nbch)
		return;
	/* Which selection.  The first resolver pass's (sel_list) stands but for what the repair rounds made void of it (CTL_NWIN0: the
	 * bursts triggered inside the windows of a local repair, or all of it), the rounds' own (sel_list2) comes on top.
	 *   SEL_FIRST: the first selection of every channel, beside the verify pass (nothing is known of any repair yet; records tagged REC_FIRST);
	 *   SEL_REPAIRED: second pass, behind the commit: only the channels a round touched (masked) -- the first pass's records that have
	 *               become void are tagged REC_VOID (the host and K4 drop those), the rounds' selection is decoded (records tagged REC_FINAL);
	 *   SEL_FINAL: the one pass behind the commit of handles that cannot run the decode ahead (more than VDL2_FMASK_SLOTS channel slots: the
	 *               mask does not cover them; complete scans): what stands of the first selection, then the rounds' selection. */
	const bool touched = p.sel_mode == SEL_FINAL ? p.redo[sc] != 0 : k2_fmask_test(p, sc);
	if (p.sel_mode == SEL_REPAIRED && !touched)
		return;
	const unsigned nwin = (p.sel_mode != SEL_FIRST && touched) ? p.ctl[CTL_NWIN0(p) + sc] : 0u;
	const int2 *win = p.win + (size_t)sc * VDL2_WIN_CAP;
	unsigned n0 = p.ctl[CTL_NSEL0(p) + sc], n1 = (p.sel_mode != SEL_FIRST && touched) ? p.ctl[CTL_NSEL1(p) + sc] : 0u;
	n0 = n0 > VDL2_SEL_CAP ? VDL2_SEL_CAP : n0;
	n1 = n1 > VDL2_SEL_CAP ? VDL2_SEL_CAP : n1;
	const unsigned *sel0 = p.sel_list + (size_t)sc * VDL2_SEL_CAP, *sel1 = p.sel_list2 + (size_t)sc * VDL2_SEL_CAP;
	if (p.sel_mode == SEL_REPAIRED && nwin != 0 && p.sel_reserved) {
		/* the first pass's records of this channel lie in one piece from CTL_SELBASE0 on: tag what has become void */
		const unsigned base0 = p.ctl[CTL_SELBASE0(p) + sc];
		for (unsigned i = blockIdx.x * K2D_NT + threadIdx.x; i < n0; i += gridDim.x * K2D_NT) {
			if (base0 + i >= p.rec_cap)
				break;
			vdl2gpu_burst_t *rec = p.recs + base0 + i;
#ifdef VDL2GPU_TESTHOOKS
			/* record i of the piece was made from entry i of the first selection (where windows are asked: a complete round re-makes the descriptors) */
			if (nwin != VDL2_WIN_ALL) {
				K2_COUNT(p, K2_DBG_CHK_B_RECORD);
				if (p.stage[sel0[i]].nstar != rec->trig_dec)
					K2_COUNT(p, K2_DBG_INV_B_RECORD);
			}
#endif
			if (nwin == VDL2_WIN_ALL || k2_in_windows(p, win, nwin, rec->trig_dec - p.dec_base))	/* invariant (b) at CTL_NWIN0 */
				rec->trig_sample = REC_VOID;
		}
	}
	/* the bursts this launch decodes for the channel: entries [0, na) of the first selection, then [0, n1) of the rounds' */
	const unsigned na = p.sel_mode == SEL_REPAIRED ? 0u : ((p.sel_mode == SEL_FINAL && nwin == VDL2_WIN_ALL) ? 0u : n0);
	const unsigned n = na + n1;
	if (blockIdx.x >= n)
		return;
	for (int i = threadIdx.x; i < 72; i += K2D_NT)
		s_tabs[i] = (i < 65) ? d_tab(c_mflt, i) : 0.0f;
	if (threadIdx.x < VDL2_ATAN_ROWS * VDL2_ATAN_STRIDE)
		s_tabs[72 + threadIdx.x] = vdl2_atan_tab_entry(threadIdx.x);
	for (int i = threadIdx.x; i < 257; i += K2D_NT) {
		float *g = s_tabs + 72 + VDL2_ATAN_ROWS * VDL2_ATAN_STRIDE;
		g[i] = d_tab(c_grey1, i);
		g[257 + i] = d_tab(c_grey2, i);
		g[514 + i] = d_tab(c_grey3, i);
	}
	__syncthreads();
	/* reserved by K2c (first selection) and K2f (the rounds' selection, when it is final): K2d fills them without atomics */
	const unsigned base0 = p.ctl[CTL_SELBASE0(p) + sc], base1 = p.ctl[CTL_SELBASE1(p) + sc];
	for (unsigned i = blockIdx.x; i < n; i += gridDim.x) {
		const bool second = i >= na;
		const BurstDesc d = p.stage[second ? sel1[i - na] : sel0[i]];
		/* (block-uniform) a burst of the first selection inside a repaired window: not on the chain any more */
		if (!second && p.sel_mode == SEL_FINAL && nwin != 0 && k2_in_windows(p, win, nwin, d.nstar - p.dec_base))
			continue;
#ifdef VDL2GPU_TESTHOOKS
		{	/* invariant (b) at CTL_NWIN0: a cluster's first descriptor (static slot, burst 0) against its candidate */
			const unsigned dslot = second ? sel1[i - na] : sel0[i];
			if (threadIdx.x == 0 && dslot < (unsigned)p.nstreams * VDL2_CS * VDL2_CAND_CAP * VDL2_CL_MAXB && dslot % VDL2_CL_MAXB == 0) {
				K2_COUNT(p, K2_DBG_CHK_B_DECODE);
				if (d.nstar != p.dec_base + p.cands[dslot / VDL2_CL_MAXB].nrel)
					K2_COUNT(p, K2_DBG_INV_B_DECODE);
			}
		}
#endif
		unsigned slot;
		if (p.sel_reserved)
			slot = (second ? base1 : base0) + (second ? i - na : i);
		else {
			__syncthreads();
			if (threadIdx.x == 0)
				s_slot = atomicAdd(&p.outc->records, 1u);
			__syncthreads();
			slot = s_slot;
		}
		if (slot >= p.rec_cap) {	/* ring full: counted, never silent */
			if (threadIdx.x == 0)
				atomicAdd(&p.outc->dropped, 1u);
			slot = 0xffffffffu;
		}
		if (slot != 0xffffffffu) {
			const int s = d.sc / VDL2_CS;
			const float2 *x0 = p.dec + (size_t)d.sc * p.cap - p.dec_base;
			burst_payload<K2D_NT, true>(p.recs + slot, x0, p.pn, d.nstar, d.clk0, d.df, d.nbrow, d.nlbyte, s, p.cfg[d.sc], sph, p.sel_mode == SEL_FIRST ? REC_FIRST : REC_FINAL, d.sc, s_tabs, p.pn8);
			if (LEV && threadIdx.x < 64)
				burst_payload_levels(p.levels + slot, x0, d.nstar, d.clk0, d.nbrow, d.nlbyte, s_tabs, p.dec_base);
			if (SOFT) {
				__syncthreads();
				burst_payload_soft<K2D_NT>(p.soft + slot, x0, d.nstar, d.clk0, d.df, d.nbrow, d.nlbyte, sph, s_tabs, s_tabs + 72 + VDL2_ATAN_ROWS * VDL2_ATAN_STRIDE);
			}
			if (CAR)
				burst_payload_carrier<K2D_NT>(p.carrier + slot, x0, d.nstar, d.clk0, d.df, d.nbrow, d.nlbyte, sph, s_tabs, s_car);
			if (FB) {
				/* burst_payload_feedback adds S up while it fills its first chunk from sph: sph has to take the longest burst in one */
				static_assert(11 + 8 * ((VDL2_MAXSYM - 3) / 8) > (25 + 8 * VDL2GPU_MAXROWS * VDL2GPU_ROWLEN - 1) / 3, "one chunk of indices in sph");
				__syncthreads();	/* (everybody is done with the phases) */
				burst_payload_feedback<K2D_NT>(fb + slot, x0, p.pn, p.pn8, d.nstar, d.clk0, d.df, d.nbrow, d.nlbyte, sph, s_tabs,
							       s_tabs + 72 + VDL2_ATAN_ROWS * VDL2_ATAN_STRIDE, reinterpret_cast<uint8_t *>(sph), VDL2_MAXSYM, s_fb);
			}
		}
		__syncthreads();
	}
}

/* The sixteen payload kernels, one line each: name, the least wavefronts per SIMD the compiler is held to, LEV, SOFT, CAR, FB.  The
 * kernels are defined from this list right below and launch_payload (vdl2gpu.hip) builds its tables from it, each kernel at the index
 * its own flag columns give: the order of the lines means nothing.  Without FB a kernel takes (K2Params), with it (K2Params, the rows'
 * ring). */
#define K2D_PAYLOAD_KERNELS(X) \
	X(k2d_payload, K2D_WAVES, 0, 0, 0, 0) \
	X(k2d_payload_lev, 4, 1, 0, 0, 0) \
	X(k2d_payload_soft, 4, 0, 1, 0, 0) \
	X(k2d_payload_lev_soft, 4, 1, 1, 0, 0) \
	X(k2d_payload_car, 4, 0, 0, 1, 0) \
	X(k2d_payload_lev_car, 4, 1, 0, 1, 0) \
	X(k2d_payload_soft_car, 4, 0, 1, 1, 0) \
	X(k2d_payload_lev_soft_car, 4, 1, 1, 1, 0) \
	X(k2d_payload_fb, 4, 0, 0, 0, 1) \
	X(k2d_payload_lev_fb, 4, 1, 0, 0, 1) \
	X(k2d_payload_soft_fb, 4, 0, 1, 0, 1) \
	X(k2d_payload_lev_soft_fb, 4, 1, 1, 0, 1) \
	X(k2d_payload_car_fb, 4, 0, 0, 1, 1) \
	X(k2d_payload_lev_car_fb, 4, 1, 0, 1, 1) \
	X(k2d_payload_soft_car_fb, 4, 0, 1, 1, 1) \
	X(k2d_payload_lev_soft_car_fb, 4, 1, 1, 1, 1)
#define K2D_INDEX(LEV, SOFT, CAR, FB) ((LEV) | (SOFT) << 1 | (CAR) << 2 | (FB) << 3)
#define K2D_BIT(name, waves, LEV, SOFT, CAR, FB) | 1u << K2D_INDEX(LEV, SOFT, CAR, FB)
static_assert((0u K2D_PAYLOAD_KERNELS(K2D_BIT)) == 0xffffu, "one payload kernel for every set of passes");
#undef K2D_BIT
#define K2D_ARGS_0 K2Params p
#define K2D_ARGS_1 K2Params p, vdl2gpu_fb_t *fb
#define K2D_PASS_0 p
#define K2D_PASS_1 p, fb
#define K2D_DEFINE(name, waves, LEV, SOFT, CAR, FB) \
	__global__ __launch_bounds__(K2D_NT) __attribute__((amdgpu_waves_per_eu(waves, 8))) void name(K2D_ARGS_##FB) \
	{ \
		k2d_run<LEV, SOFT, CAR, FB>(K2D_PASS_##FB); \
	}
K2D_PAYLOAD_KERNELS(K2D_DEFINE)
#undef K2D_DEFINE

#endif
