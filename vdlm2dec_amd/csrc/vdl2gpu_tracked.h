/* vdl2gpu_tracked.h -- VDL2GPU_F_TRACKED (include/vdl2gpu.h, vdl2gpu_trk_t): what vdl2gpu.hip needs of vdl2gpu_tracked.hip -- the
 * parameter block of the kernel that slices a burst's payload with a tracked sampling instant, the prototypes of that kernel and of
 * the column's export, and the block path's kernels with the second attempt (k4_frames_body with TRK).  The kernels live in a
 * translation unit of their own for the reason those of vdl2gpu_symclk.hip do: the kernels of vdl2gpu.hip are compiled without them
 * and keep their registers, and the record of them (kernel_resources.txt) keeps its set of names.  (Behind vdl2gpu_blocks.h: K4Params) */
#ifndef VDL2GPU_TRACKED_H
#define VDL2GPU_TRACKED_H

#define KTR_NT VDL2GPU_TRK_SEG	/* lanes of a workgroup: one per symbol of a segment */
static_assert(VDL2GPU_TRK_SEGS == ((25 + 8 * VDL2GPU_MAXROWS * VDL2GPU_ROWLEN - 1) / 3 - 7 + VDL2GPU_TRK_SEG - 1) / VDL2GPU_TRK_SEG,
	      "VDL2GPU_TRK_SEGS segments of VDL2GPU_TRK_SEG symbols cover the payload symbols of the longest burst, and no more");
static_assert(sizeof(vdl2gpu_trk_t) == 2048 && offsetof(vdl2gpu_trk_t, d_first) == 2040 && offsetof(vdl2gpu_trk_t, nseg) == 2044,
	      "vdl2gpu_trk_t as include/vdl2gpu.h states it");

/* Record-driven like k_symclk_sums: a record of the push's ring carries all the kernel needs (end_dec, nbrow, nlbyte, df, stream, chn,
 * Fr, and on the device the tag in trig_sample and -- from K2d, not from the serial machine -- the channel slot in end_sample). */
struct KTrackedParams {
	const float2 *dec;		/* the push's plane set: plane of channel slot sc at dec + sc * cap, frame 0 = stream time dec_base */
	int cap;			/* frames a plane has room for: the planes' stride */
	long long dec_base;
	const ChanCfg *cfg;		/* [nstreams * VDL2_CS] */
	int nbch, nstreams;
	int frames;			/* frames of a plane that hold the push's samples, at most cap: nothing outside [0, frames) is read */
	const vdl2gpu_burst_t *recs;	/* the push's output ring ... */
	const unsigned *count;		/* ... and how many records it holds */
	unsigned rec_cap;
	vdl2gpu_trk_t *out;		/* one entry per record slot of `recs` */
	const uint8_t *pn8;		/* the scrambler sequence by payload byte (K2Params.pn8) */
};

/* grid (x): workgroup x does the records x, x + gridDim.x, ...: all segments of a record in order, then its bytes */
__global__ void k_tracked_rows(KTrackedParams p);
/* the column, device ring -> slab, behind k_export_records with its count / cap (like k_export_feedback) */
__global__ void k_export_tracked(const unsigned *count, unsigned cap, const vdl2gpu_trk_t *src, vdl2gpu_trk_t *dst);
/* the block kernel with the second attempt for a handle's or a call's combination of report, feedback rows and mode (VDL2GPU_BLK_*) */
typedef void (*K4Kernel)(K4Params);
K4Kernel k4_frames_trk_kernel(bool rep, bool fb, uint32_t mode);

#endif
