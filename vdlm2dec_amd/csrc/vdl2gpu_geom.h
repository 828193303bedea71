/* vdl2gpu_geom.h -- the byte schedule of a burst.  Part of the device side of libvdl2gpu.so; included by vdl2gpu_machine.h (the
 * demodulator) and by vdl2gpu_allframes.hip (the block path's kernels that live in a translation unit of their own). */
#ifndef VDL2GPU_GEOM_H
#define VDL2GPU_GEOM_H

/* receiver's byte schedule for a burst of nbrow rows / nlbyte bytes in the last row
 * (d8psk.c:117-206): ND data bytes then NF FEC bytes, column-major over the rows,
 * short last row */
struct BurstGeom {
	int nd_rows, nd_last, nf_rows, nf_last, ND, NF, nsym;
};

__device__ __forceinline__ BurstGeom burst_geom(int nbrow, int nlbyte)
{
	BurstGeom g;
	g.nd_rows = nbrow;
	g.nd_last = nlbyte ? nlbyte : 249;	/* nlbyte==0: the zero-fill loop is skipped */
	g.ND = (nbrow - 1) * 249 + g.nd_last;
	if (nlbyte <= 2) {			/* FEC shortening of the last row, d8psk.c:153-161 */
		g.nf_rows = nbrow - 1;
		g.nf_last = 6;
	} else {
		g.nf_rows = nbrow;
		g.nf_last = (nlbyte <= 30) ? 2 : (nlbyte <= 67 ? 4 : 6);
	}
	g.NF = (g.nf_rows > 0) ? (g.nf_rows - 1) * 6 + g.nf_last : 0;
	g.nsym = (25 + 8 * (g.ND + g.NF) + 2) / 3;
	return g;
}

#endif
