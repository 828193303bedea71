/*
 * vdl2gpu_allframes.hip -- the block path's kernels for VDL2GPU_F_ALL_FRAMES (include/vdl2gpu.h): k4_frames_body of vdl2gpu_blocks.h
 * with ALL, once for each of REP x FB.  Every segment between two flags of a burst is a candidate frame, not only what follows the
 * first flag.
 *
 * A translation unit of its own, compiled by its own hipcc -c and linked into libvdl2gpu.so: the kernels of vdl2gpu.hip are then
 * compiled without these four beside them and keep the registers they had, and the record of them (kernel_resources.txt) keeps its
 * set of names; these four are recorded in kernel_resources_allframes.txt.  Nothing but the four kernels is defined here: the types
 * without the constant tables, the block path's device functions without its kernels.  vdl2gpu.hip launches them through the
 * prototypes at the end of vdl2gpu_blocks.h.
 */
#define VDL2GPU_TYPES_NO_TABLES
#define VDL2GPU_BLOCKS_DEVICE_ONLY
#include "vdl2gpu_types.h"
#include "vdl2gpu_geom.h"
#include "vdl2gpu_blocks.h"

/* (k4_frames runs five waves to a SIMD, at 96 registers; left alone the compiler takes 104 here, and four) */
__global__ __launch_bounds__(K4_NT) __attribute__((amdgpu_waves_per_eu(5)))
void k4_frames_all(K4Params p)
{
	k4_frames_body<false, false, true>(p);
}

__global__ __launch_bounds__(K4_NT)
void k4_frames_all_rep(K4Params p)
{
	k4_frames_body<true, false, true>(p);
}

__global__ __launch_bounds__(K4_NT)
void k4_frames_all_fb(K4Params p)
{
	k4_frames_body<false, true, true>(p);
}

__global__ __launch_bounds__(K4_NT)
void k4_frames_all_rep_fb(K4Params p)
{
	k4_frames_body<true, true, true>(p);
}
