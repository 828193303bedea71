/*
 * vdl2gpu_rawflags.hip -- the block path's kernels for VDL2GPU_F_RAW_FLAGS (include/vdl2gpu.h): k4_frames_body of vdl2gpu_blocks.h
 * with ALL and RAW, once for each of REP x FB.  Every segment between two flags of a burst is a candidate frame, and a flag is six
 * adjacent ones of the stuffed bit stream: a stuffed data byte 0x7e is data.
 *
 * A translation unit of its own for the reason vdl2gpu_allframes.hip is one: the kernels of vdl2gpu.hip and of vdl2gpu_allframes.hip
 * are compiled without these four beside them and keep their registers, and the records of them keep their sets of names; these four
 * are recorded in kernel_resources_rawflags.txt.  Nothing but the four kernels is defined here.  vdl2gpu.hip launches them through
 * the prototypes at the end of vdl2gpu_blocks.h.
 */
#define VDL2GPU_TYPES_NO_TABLES
#define VDL2GPU_BLOCKS_DEVICE_ONLY
#include "vdl2gpu_types.h"
#include "vdl2gpu_geom.h"
#include "vdl2gpu_blocks.h"

/* (five waves to a SIMD, like k4_frames and k4_frames_all) */
__global__ __launch_bounds__(K4_NT) __attribute__((amdgpu_waves_per_eu(5)))
void k4_frames_raw(K4Params p)
{
	k4_frames_body<false, false, true, true>(p);
}

__global__ __launch_bounds__(K4_NT)
void k4_frames_raw_rep(K4Params p)
{
	k4_frames_body<true, false, true, true>(p);
}

__global__ __launch_bounds__(K4_NT)
void k4_frames_raw_fb(K4Params p)
{
	k4_frames_body<false, true, true, true>(p);
}

__global__ __launch_bounds__(K4_NT)
void k4_frames_raw_rep_fb(K4Params p)
{
	k4_frames_body<true, true, true, true>(p);
}
