/* vdl2gpu_symclk.h -- VDL2GPU_F_SYMCLK (include/vdl2gpu.h, vdl2gpu_symclk_t): what vdl2gpu.hip needs of vdl2gpu_symclk.hip -- the
 * parameter block of its two kernels, their prototypes, and the sub-phase-0 taps as the host holds them.  The kernels live in a
 * translation unit of their own for the reason those of vdl2gpu_allframes.hip do: the kernels of vdl2gpu.hip are compiled without
 * them and keep their registers, and the record of them (kernel_resources.txt) keeps its set of names. */
#ifndef VDL2GPU_SYMCLK_H
#define VDL2GPU_SYMCLK_H

#define KSC_NT VDL2GPU_SYMCLK_SEG	/* lanes of a workgroup: one per symbol of a segment */
#define KSC_TAPS 17			/* mflt[4 j], j = 0 .. 16: sub-phase 0 */
static_assert(VDL2GPU_SYMCLK_SEGS == ((25 + 8 * VDL2GPU_MAXROWS * VDL2GPU_ROWLEN + 2) / 3 + VDL2GPU_SYMCLK_SEG - 1) / VDL2GPU_SYMCLK_SEG,
	      "VDL2GPU_SYMCLK_SEGS segments of VDL2GPU_SYMCLK_SEG symbols cover the longest burst (burst_geom with VDL2GPU_MAXROWS rows), and no more");
static_assert(sizeof(vdl2gpu_symclk_t) == 744 && offsetof(vdl2gpu_symclk_t, e) == 40 && offsetof(vdl2gpu_symclk_t, toa_sample) == 16,
	      "vdl2gpu_symclk_t as include/vdl2gpu.h states it");

/* The kernels are record-driven: a record of the push's ring carries all they need (end_dec, nbrow, nlbyte, stream, chn, Fr, and
 * on the device the tag in trig_sample and -- from K2d, not from the serial machine -- the channel slot in end_sample), so one code
 * path serves K2d, the serial machine, repair rounds and deferred bursts alike. */
struct KSymclkParams {
	const float2 *dec;		/* the push's plane set: plane of channel slot sc at dec + sc * cap, frame 0 = stream time dec_base */
	long long cap;
	long long dec_base;
	long long frames;		/* frames of a plane that hold the push's samples: VDL2_CARRY_FRAMES + J; nothing outside [0, frames) is read */
	const ChanCfg *cfg;		/* [nstreams * VDL2_CS] */
	int nbch, nstreams;
	const vdl2gpu_burst_t *recs;	/* the push's output ring ... */
	const unsigned *count;		/* ... and how many records it holds */
	unsigned rec_cap;
	vdl2gpu_symclk_t *out;		/* one record per record slot of `recs` */
	float taps[KSC_TAPS];
};

/* grid (VDL2GPU_SYMCLK_SEGS, y): workgroup (s, y) does segment s of the records y, y + gridDim.y, ... */
__global__ void k_symclk_sums(KSymclkParams p);
/* the column, device ring -> slab, behind k_export_records with its count / cap (like k_export_feedback) */
__global__ void k_export_symclk(const unsigned *count, unsigned cap, const vdl2gpu_symclk_t *src, vdl2gpu_symclk_t *dst);
/* mflt[4 j] for j = 0 .. 16 as floats, from the host's copy of the table (no device call) */
void symclk_taps(float *taps17);

#endif
