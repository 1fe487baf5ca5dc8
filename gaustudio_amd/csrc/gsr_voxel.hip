// gsr_voxel.hip -- triangle mesh voxelization and closest-point colouring on the device: the hot path of the reference's
// VoxelInitializer (gaustudio/pipelines/initializers/mesh.py:252-442), which goes through Open3D's
// VoxelGrid.create_from_triangle_mesh_within_bounds (every voxel against every triangle on one CPU core) and a per-point
// Python loop for the colours.
//
// Contract (every operation in order: tests/mesh_voxel_model.py):
//   * everything is float64 and written out operation by operation (the library is built with -ffp-contract=off): the set of
//     occupied voxels does not depend on a float32 rounding of a separating-axis test;
//   * overlap = Akenine-Moller's triangle / box test with its exact comparisons, box centre (min_bound + h) + i voxel_size,
//     h = voxel_size / 2; touching counts; a zero-area triangle voxelizes as the segment or point it is;
//   * occupied voxels in ascending linear index (i0 n1 + i1) n2 + i2, their triangles ascending within a voxel;
//   * closest = Ericson's closest point on a triangle (region tests in his order) from the returned voxel centre
//     ((i + 0.5) voxel_size) + min_bound to the triangles listed in the 27 voxels around it; smallest d2 wins, exact ties go to
//     the lower triangle, a d2 that is not finite never wins (no winner: triangle -1, weights 0, colour 0.5).
//
// MI355X design:
//   * plan: one lane per triangle -> index-space box (widened by one voxel), number of (i0, i1) columns; exclusive scan;
//   * count / emit: one lane per (triangle, column) work item, found by binary search in the scan.  The triangle's plane
//     narrows the column to a conservative i2 range (a filter only: the overlap test decides), so no lane walks a large
//     triangle's whole box -- a lane's worst case is one column of at most 1024 voxels.  Count, scan, emit in item order;
//   * sort: the stable LSD radix sort of gsr_sort.h by voxel index, only the digits n0 n1 n2 needs; head flags, scan, compact;
//   * closest: one wave per occupied voxel; lanes 0..26 find the neighbours by binary search in voxel_index, the 64 lanes
//     stride over the concatenated candidate lists, a lexicographic (d2, triangle) butterfly picks the winner.
// All arithmetic is scalar-per-lane float64 on the vector ALU (no matrix cores, no packed math).  Plain HIP C++.  No float atomics:
// the only atomics are integer vector atomics (status word, 64-bit totals, occupancy bits, the sort's LDS histogram).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsrast.h"
#include "gsr_sort.h"

namespace {

struct VGrid { double vs, h, mb[3]; int n[3]; };

bool make_grid(double voxel_size, const double* min_bound, int n0, int n1, int n2, VGrid* G)
{
	if (!min_bound || !(voxel_size > 0.0) || !isfinite(voxel_size)) return false;
	const int n[3] = {n0, n1, n2};
	for (int d = 0; d < 3; d++) {
		if (n[d] < 2 || n[d] > GSR_VOXEL_MAX_RES || !isfinite(min_bound[d])) return false;
		G->n[d] = n[d];
		G->mb[d] = min_bound[d];
	}
	G->vs = voxel_size;
	G->h = voxel_size / 2;
	return true;
}

__device__ __forceinline__ double box_centre(const VGrid& G, int d, int i) { return (G.mb[d] + G.h) + (double)i * G.vs; }

// ------------------------------------------------------------------------------------------------------ overlap
__device__ __forceinline__ bool sep(double pa, double pb, double rad) { return fmin(pa, pb) > rad || fmax(pa, pb) < -rad; }

// tribox3: true = the box (centre c, half edge h) and the triangle overlap
__device__ bool tribox(const double c[3], double h, const double t0[3], const double t1[3], const double t2[3])
{
	double v0[3], v1[3], v2[3], e0[3], e1[3], e2[3];
	for (int k = 0; k < 3; k++) { v0[k] = t0[k] - c[k]; v1[k] = t1[k] - c[k]; v2[k] = t2[k] - c[k]; }
	for (int k = 0; k < 3; k++) { e0[k] = v1[k] - v0[k]; e1[k] = v2[k] - v1[k]; e2[k] = v0[k] - v2[k]; }
	double a, b, rad;
#define VOX_XT(e, va, vb) a = e[2]; b = e[1]; rad = fabs(a) * h + fabs(b) * h; \
	if (sep(a * va[1] - b * va[2], a * vb[1] - b * vb[2], rad)) return false;
#define VOX_YT(e, va, vb) a = e[2]; b = e[0]; rad = fabs(a) * h + fabs(b) * h; \
	if (sep(-a * va[0] + b * va[2], -a * vb[0] + b * vb[2], rad)) return false;
#define VOX_ZT(e, va, vb) a = e[1]; b = e[0]; rad = fabs(a) * h + fabs(b) * h; \
	if (sep(a * va[0] - b * va[1], a * vb[0] - b * vb[1], rad)) return false;
	VOX_XT(e0, v0, v2) VOX_YT(e0, v0, v2) VOX_ZT(e0, v1, v2)
	VOX_XT(e1, v0, v2) VOX_YT(e1, v0, v2) VOX_ZT(e1, v0, v1)
	VOX_XT(e2, v0, v1) VOX_YT(e2, v0, v1) VOX_ZT(e2, v1, v2)
#undef VOX_XT
#undef VOX_YT
#undef VOX_ZT
	for (int k = 0; k < 3; k++) {
		const double mn = fmin(fmin(v0[k], v1[k]), v2[k]), mx = fmax(fmax(v0[k], v1[k]), v2[k]);
		if (mn > h || mx < -h) return false;
	}
	const double n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
	double vmin[3], vmax[3];
	for (int k = 0; k < 3; k++) {
		if (n[k] > 0.0) { vmin[k] = -h - v0[k]; vmax[k] = h - v0[k]; }
		else            { vmin[k] = h - v0[k]; vmax[k] = -h - v0[k]; }
	}
	if (n[0] * vmin[0] + n[1] * vmin[1] + n[2] * vmin[2] > 0.0) return false;
	return n[0] * vmax[0] + n[1] * vmax[1] + n[2] * vmax[2] >= 0.0;
}

// ------------------------------------------------------------------------------------------------------ plan
__global__ void __launch_bounds__(256) vox_check_vertices(const double* __restrict__ v, long long n3, int* status)
{
	const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
	if (i < n3 && !isfinite(v[i])) atomicOr(status, 1);
}

// per triangle: box[6] = lo0, lo1, lo2, hi0, hi1, hi2 (inclusive; lo > hi = none) and the number of (i0, i1) columns
__global__ void __launch_bounds__(256) vox_plan(const double* __restrict__ verts, int nv, const int* __restrict__ faces, int nf,
                                                VGrid G, int* __restrict__ box, int* __restrict__ ncol,
                                                unsigned long long* total, int* status)
{
	__shared__ unsigned long long s_total;
	if (threadIdx.x == 0) s_total = 0;
	__syncthreads();
	const int t = blockIdx.x * 256 + threadIdx.x;
	if (t < nf) {
		const int f0 = faces[3 * (size_t)t], f1 = faces[3 * (size_t)t + 1], f2 = faces[3 * (size_t)t + 2];
		int cols = 0;
		if (f0 < 0 || f0 >= nv || f1 < 0 || f1 >= nv || f2 < 0 || f2 >= nv) {
			atomicOr(status, 2);
			for (int k = 0; k < 6; k++) box[6 * (size_t)t + k] = k < 3 ? 1 : 0;
		} else {
			int lo[3], hi[3];
			for (int d = 0; d < 3; d++) {
				const double x0 = verts[3 * (size_t)f0 + d], x1 = verts[3 * (size_t)f1 + d], x2 = verts[3 * (size_t)f2 + d];
				const double mn = fmin(fmin(x0, x1), x2), mx = fmax(fmax(x0, x1), x2);
				const double flo = floor((mn - G.mb[d]) / G.vs) - 1.0, fhi = floor((mx - G.mb[d]) / G.vs) + 1.0;
				lo[d] = (int)fmin(fmax(flo, 0.0), (double)G.n[d]);
				hi[d] = (int)fmin(fmax(fhi, -1.0), (double)(G.n[d] - 1));
			}
			if (lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2]) cols = (hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1);
			for (int d = 0; d < 3; d++) { box[6 * (size_t)t + d] = lo[d]; box[6 * (size_t)t + 3 + d] = hi[d]; }
		}
		ncol[t] = cols;
		if (cols) atomicAdd(&s_total, (unsigned long long)cols);
	}
	__syncthreads();
	if (threadIdx.x == 0 && s_total) atomicAdd(total, s_total);
}

// ------------------------------------------------------------------------------------------------------ count / emit
// the i2 range [klo, khi] within [lo2, hi2] that the triangle's plane can reach in column (i0, i1), one voxel wider either
// side; the whole range when the normal's component along the column is too small for the bound to hold
__device__ void plane_range(const VGrid& G, const double t0[3], const double t1[3], const double t2[3], int i0, int i1, int lo2,
                            int hi2, int* klo, int* khi)
{
	*klo = lo2; *khi = hi2;
	double e0[3], e1[3];
	for (int k = 0; k < 3; k++) { e0[k] = t1[k] - t0[k]; e1[k] = t2[k] - t1[k]; }
	const double n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
	double L = 0.0, M = 0.0;
	for (int k = 0; k < 3; k++) {
		L = fmax(L, fmax(fabs(e0[k]), fabs(e1[k])));
		M = fmax(M, fmax(fmax(fabs(t0[k]), fabs(t1[k])), fabs(t2[k])));
	}
	const double nerr = (0x1p-40 * L) * (M + L);   // far above the rounding error of a normal component
	if (!(fabs(n[2]) * G.vs > (32.0 * L) * nerr)) return;
	const double dx = box_centre(G, 0, i0) - t0[0], dy = box_centre(G, 1, i1) - t0[1];
	const double s = n[0] * dx + n[1] * dy;
	const double zc = t0[2] - s / n[2];
	const double r = ((fabs(n[0]) + fabs(n[1])) * G.h) / fabs(n[2]);
	const double flo = floor(((zc - r) - G.mb[2]) / G.vs) - 1.0, fhi = floor(((zc + r) - G.mb[2]) / G.vs) + 1.0;
	*klo = (int)fmin(fmax(flo, (double)lo2), (double)(hi2 + 1));
	*khi = (int)fmin(fmax(fhi, (double)(lo2 - 1)), (double)hi2);
}

// EMIT = false: count[w] = hits of work item w; EMIT = true: the hits go to keys / tris from start[w] on
template <bool EMIT>
__global__ void __launch_bounds__(256) vox_items(const double* __restrict__ verts, const int* __restrict__ faces, int nf, VGrid G,
                                                 const int* __restrict__ box, const int* __restrict__ col_start, int num_items,
                                                 int* __restrict__ count, const int* __restrict__ start, int* __restrict__ keys,
                                                 int* __restrict__ tris, unsigned long long* total)
{
	__shared__ unsigned long long s_total;
	if (!EMIT) {
		if (threadIdx.x == 0) s_total = 0;
		__syncthreads();
	}
	const int w = blockIdx.x * 256 + threadIdx.x;
	if (w < num_items) {
		int a = 0, b = nf;          // the last triangle t with col_start[t] <= w (triangles without columns share a start)
		while (b - a > 1) {
			const int m = (a + b) >> 1;
			if (col_start[m] <= w) a = m; else b = m;
		}
		const int t = a;
		const int* bx = box + 6 * (size_t)t;
		const int lo0 = bx[0], lo1 = bx[1], lo2 = bx[2], hi1 = bx[4], hi2 = bx[5];
		const int c = w - col_start[t], w1 = hi1 - lo1 + 1;
		const int i0 = lo0 + c / w1, i1 = lo1 + c % w1;
		double t0[3], t1[3], t2[3];
		const int f0 = faces[3 * (size_t)t], f1 = faces[3 * (size_t)t + 1], f2 = faces[3 * (size_t)t + 2];
		for (int k = 0; k < 3; k++) {
			t0[k] = verts[3 * (size_t)f0 + k]; t1[k] = verts[3 * (size_t)f1 + k]; t2[k] = verts[3 * (size_t)f2 + k];
		}
		int klo, khi;
		plane_range(G, t0, t1, t2, i0, i1, lo2, hi2, &klo, &khi);
		double cc[3] = {box_centre(G, 0, i0), box_centre(G, 1, i1), 0.0};
		int hits = 0;
		size_t out = EMIT ? (size_t)start[w] : 0;
		for (int i2 = klo; i2 <= khi; i2++) {
			cc[2] = box_centre(G, 2, i2);
			if (tribox(cc, G.h, t0, t1, t2)) {
				if (EMIT) {
					keys[out] = (i0 * G.n[1] + i1) * G.n[2] + i2;
					tris[out] = t;
					out++;
				}
				hits++;
			}
		}
		if (!EMIT) {
			count[w] = hits;
			if (hits) atomicAdd(&s_total, (unsigned long long)hits);
		}
	}
	if (!EMIT) {
		__syncthreads();
		if (threadIdx.x == 0 && s_total) atomicAdd(total, s_total);
	}
}

// ------------------------------------------------------------------------------------------------------ sort / compact
__global__ void __launch_bounds__(256) vox_heads(const int* __restrict__ keys, int n, int* __restrict__ head)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

__global__ void __launch_bounds__(256) vox_compact(const int* __restrict__ keys, const int* __restrict__ tris, int n,
                                                   const int* __restrict__ head, const int* __restrict__ rank, int n1, int n2,
                                                   uint32_t* __restrict__ voxel_index, int* __restrict__ pair_start,
                                                   int* __restrict__ pair_tri, int* __restrict__ grid_index,
                                                   uint32_t* __restrict__ occupancy)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	pair_tri[i] = tris[i];
	if (head[i]) {
		const int r = rank[i], key = keys[i];
		voxel_index[r] = (uint32_t)key;
		pair_start[r] = i;
		if (grid_index) {
			grid_index[3 * (size_t)r] = key / (n1 * n2);
			grid_index[3 * (size_t)r + 1] = (key / n2) % n1;
			grid_index[3 * (size_t)r + 2] = key % n2;
		}
		if (occupancy) atomicOr(&occupancy[key >> 5], 1u << (key & 31));
	}
	if (i == n - 1) pair_start[rank[n]] = n;
}

// ------------------------------------------------------------------------------------------------------ closest
__device__ __forceinline__ double dot3(const double x[3], const double y[3]) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }

// Ericson, Real-Time Collision Detection 5.1.5: barycentric (v, w) of the closest point, and the squared distance to it
__device__ double closest_point(const double p[3], const double a[3], const double b[3], const double c[3], double* v_out,
                                double* w_out)
{
	double ab[3], ac[3], ap[3], bp[3], cp[3], q[3];
	for (int k = 0; k < 3; k++) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = p[k] - a[k]; }
	const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
	double v, w;
	bool done = false;
	if (d1 <= 0.0 && d2 <= 0.0) { v = 0.0; w = 0.0; for (int k = 0; k < 3; k++) q[k] = a[k]; done = true; }
	double d3 = 0, d4 = 0, d5 = 0, d6 = 0, vc = 0, vb = 0;
	if (!done) {
		for (int k = 0; k < 3; k++) bp[k] = p[k] - b[k];
		d3 = dot3(ab, bp); d4 = dot3(ac, bp);
		if (d3 >= 0.0 && d4 <= d3) { v = 1.0; w = 0.0; for (int k = 0; k < 3; k++) q[k] = b[k]; done = true; }
	}
	if (!done) {
		vc = d1 * d4 - d3 * d2;
		if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
			v = d1 / (d1 - d3); w = 0.0;
			for (int k = 0; k < 3; k++) q[k] = a[k] + v * ab[k];
			done = true;
		}
	}
	if (!done) {
		for (int k = 0; k < 3; k++) cp[k] = p[k] - c[k];
		d5 = dot3(ab, cp); d6 = dot3(ac, cp);
		if (d6 >= 0.0 && d5 <= d6) { v = 0.0; w = 1.0; for (int k = 0; k < 3; k++) q[k] = c[k]; done = true; }
	}
	if (!done) {
		vb = d5 * d2 - d1 * d6;
		if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
			w = d2 / (d2 - d6); v = 0.0;
			for (int k = 0; k < 3; k++) q[k] = a[k] + w * ac[k];
			done = true;
		}
	}
	if (!done) {
		const double va = d3 * d6 - d5 * d4;
		if (va <= 0.0 && (d4 - d3) >= 0.0 && (d5 - d6) >= 0.0) {
			w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); v = 1.0 - w;
			for (int k = 0; k < 3; k++) q[k] = b[k] + w * (c[k] - b[k]);
		} else {
			const double denom = 1.0 / ((va + vb) + vc);
			v = vb * denom; w = vc * denom;
			for (int k = 0; k < 3; k++) q[k] = (a[k] + ab[k] * v) + ac[k] * w;
		}
	}
	const double dx = p[0] - q[0], dy = p[1] - q[1], dz = p[2] - q[2];
	*v_out = v; *w_out = w;
	return dx * dx + dy * dy + dz * dz;
}

// one wave per occupied voxel, four per block
__global__ void __launch_bounds__(256) vox_closest(const double* __restrict__ verts, int nv, const int* __restrict__ faces, int nf,
                                                   const float* __restrict__ colors, VGrid G,
                                                   const uint32_t* __restrict__ voxel_index, const int* __restrict__ pair_start,
                                                   const int* __restrict__ pair_tri, int nvox, int* __restrict__ closest_tri,
                                                   double* __restrict__ closest_uvw, float* __restrict__ color)
{
	__shared__ int s_start[4][27];
	__shared__ int s_pref[4][28];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int q = blockIdx.x * 4 + wave;
	const bool active = q < nvox;
	int g[3] = {0, 0, 0};
	if (active) {
		const int key = (int)voxel_index[q];
		g[0] = key / (G.n[1] * G.n[2]); g[1] = (key / G.n[2]) % G.n[1]; g[2] = key % G.n[2];
	}
	if (lane < 27) {
		int st = 0, cnt = 0;
		const int o[3] = {g[0] + lane / 9 - 1, g[1] + (lane / 3) % 3 - 1, g[2] + lane % 3 - 1};
		if (active && o[0] >= 0 && o[0] < G.n[0] && o[1] >= 0 && o[1] < G.n[1] && o[2] >= 0 && o[2] < G.n[2]) {
			const uint32_t want = (uint32_t)((o[0] * G.n[1] + o[1]) * G.n[2] + o[2]);
			int a = 0, b = nvox;          // first slot with voxel_index >= want
			while (a < b) {
				const int m = (a + b) >> 1;
				if (voxel_index[m] < want) a = m + 1; else b = m;
			}
			if (a < nvox && voxel_index[a] == want) { st = pair_start[a]; cnt = pair_start[a + 1] - st; }
		}
		s_start[wave][lane] = st;
		s_pref[wave][lane] = cnt < 0 ? 0 : cnt;
	}
	__syncthreads();
	if (lane == 0) {
		int run = 0;
		for (int k = 0; k < 27; k++) { const int cnt = s_pref[wave][k]; s_pref[wave][k] = run; run += cnt; }
		s_pref[wave][27] = run;
	}
	__syncthreads();
	const double p[3] = {((double)g[0] + 0.5) * G.vs + G.mb[0], ((double)g[1] + 0.5) * G.vs + G.mb[1],
	                     ((double)g[2] + 0.5) * G.vs + G.mb[2]};
	double bd = INFINITY, bv = 0.0, bw = 0.0;
	int bt = INT_MAX;
	const int total = active ? s_pref[wave][27] : 0;
	for (int j = lane; j < total; j += 64) {
		int k = 0;
		while (k < 26 && s_pref[wave][k + 1] <= j) k++;
		const int t = pair_tri[s_start[wave][k] + (j - s_pref[wave][k])];
		if (t < 0 || t >= nf) continue;
		const int f0 = faces[3 * (size_t)t], f1 = faces[3 * (size_t)t + 1], f2 = faces[3 * (size_t)t + 2];
		if (f0 < 0 || f0 >= nv || f1 < 0 || f1 >= nv || f2 < 0 || f2 >= nv) continue;
		double a[3], b[3], c[3], v, w;
		for (int d = 0; d < 3; d++) { a[d] = verts[3 * (size_t)f0 + d]; b[d] = verts[3 * (size_t)f1 + d]; c[d] = verts[3 * (size_t)f2 + d]; }
		const double dd = closest_point(p, a, b, c, &v, &w);
		if (isfinite(dd) && (dd < bd || (dd == bd && t < bt))) { bd = dd; bt = t; bv = v; bw = w; }
	}
	for (int off = 32; off > 0; off >>= 1) {
		const double od = __shfl_xor(bd, off), ov = __shfl_xor(bv, off), ow = __shfl_xor(bw, off);
		const int ot = __shfl_xor(bt, off);
		if (od < bd || (od == bd && ot < bt)) { bd = od; bt = ot; bv = ov; bw = ow; }
	}
	if (active && lane == 0) {
		const bool found = bt != INT_MAX;
		const double u = (1.0 - bv) - bw;
		closest_tri[q] = found ? bt : -1;
		closest_uvw[3 * (size_t)q] = found ? u : 0.0;
		closest_uvw[3 * (size_t)q + 1] = found ? bv : 0.0;
		closest_uvw[3 * (size_t)q + 2] = found ? bw : 0.0;
		if (color) {
			for (int ch = 0; ch < 3; ch++) {
				float out = 0.5f;
				if (found) {
					const double c0 = (double)colors[3 * (size_t)faces[3 * (size_t)bt] + ch];
					const double c1 = (double)colors[3 * (size_t)faces[3 * (size_t)bt + 1] + ch];
					const double c2 = (double)colors[3 * (size_t)faces[3 * (size_t)bt + 2] + ch];
					out = (float)((c0 * u + c1 * bv) + c2 * bw);
				}
				color[3 * (size_t)q + ch] = out;
			}
		}
	}
}

}  // namespace

extern "C" {

int gsr_voxel_plan(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const double* vertices, int num_vertices, const int* faces,
                   int num_faces, double voxel_size, const double* min_bound, int n0, int n1, int n2, int* tri_box, int* col_start,
                   int* num_items, void* stream)
{
	VGrid G;
	if (!make_grid(voxel_size, min_bound, n0, n1, n2, &G) || num_vertices < 0 || num_faces < 0 || num_faces > (1 << 28) ||
	    num_vertices > (1 << 28) || !num_items || !col_start || (num_faces > 0 && (!vertices || !faces || !tri_box || num_vertices < 1)))
		return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const int nf = num_faces;
	int *ncol, *part, *status, *box;
	unsigned long long* total;
	auto carve = [&](Arena& ws) {
		ncol = ws.take<int>(nf); part = ws.take<int>(scan_part_len(nf));
		total = ws.take<unsigned long long>(1); status = ws.take<int>(1);
		box = ws.take<int>((size_t)nf * 6);   // the caller's arrays are written only once the mesh has been found valid
	};
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;
	GSR_TRY(hipMemsetAsync(total, 0, 8, s));
	GSR_TRY(hipMemsetAsync(status, 0, 4, s));
	if (nf > 0) {
		hipLaunchKernelGGL(vox_check_vertices, dim3(blocks(3LL * num_vertices)), dim3(256), 0, s, vertices, 3LL * num_vertices, status);
		hipLaunchKernelGGL(vox_plan, dim3(blocks(nf)), dim3(256), 0, s, vertices, num_vertices, faces, nf, G, box, ncol, total, status);
	}
	int bad = 0;
	unsigned long long tot = 0;
	GSR_TRY(hipMemcpyAsync(&bad, status, sizeof(int), hipMemcpyDeviceToHost, s));
	GSR_TRY(hipMemcpyAsync(&tot, total, sizeof(tot), hipMemcpyDeviceToHost, s));
	GSR_TRY(hipStreamSynchronize(s));
	if (bad || tot > (unsigned long long)GSR_VOXEL_MAX_ITEMS) return GSR_ERR_ARG;
	if (nf > 0) GSR_TRY(hipMemcpyAsync(tri_box, box, (size_t)nf * 6 * sizeof(int), hipMemcpyDeviceToDevice, s));
	const int rc = exclusive_scan(ncol, nf, col_start, part, s);
	if (rc) return rc;
	*num_items = (int)tot;
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_voxel_count(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const double* vertices, const int* faces, int num_faces,
                    double voxel_size, const double* min_bound, int n0, int n1, int n2, const int* tri_box, const int* col_start,
                    int num_items, int* item_start, int* num_pairs, void* stream)
{
	VGrid G;
	if (!make_grid(voxel_size, min_bound, n0, n1, n2, &G) || num_faces < 0 || num_items < 0 || num_items > GSR_VOXEL_MAX_ITEMS ||
	    !item_start || !num_pairs || (num_items > 0 && (!vertices || !faces || !tri_box || !col_start || num_faces < 1)))
		return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	int *count, *part;
	unsigned long long* total;
	auto carve = [&](Arena& ws) {
		count = ws.take<int>(num_items); part = ws.take<int>(scan_part_len(num_items));
		total = ws.take<unsigned long long>(1);
	};
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;
	GSR_TRY(hipMemsetAsync(total, 0, 8, s));
	if (num_items > 0)
		hipLaunchKernelGGL(vox_items<false>, dim3(blocks(num_items)), dim3(256), 0, s, vertices, faces, num_faces, G, tri_box, col_start,
		                   num_items, count, (const int*)nullptr, (int*)nullptr, (int*)nullptr, total);
	const int rc = exclusive_scan(count, num_items, item_start, part, s);
	if (rc) return rc;
	unsigned long long tot = 0;
	GSR_TRY(hipMemcpyAsync(&tot, total, sizeof(tot), hipMemcpyDeviceToHost, s));
	GSR_TRY(hipStreamSynchronize(s));
	if (tot > (unsigned long long)GSR_VOXEL_MAX_ITEMS) return GSR_ERR_ARG;
	*num_pairs = (int)tot;
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_voxel_emit(const double* vertices, const int* faces, int num_faces, double voxel_size, const double* min_bound, int n0, int n1,
                   int n2, const int* tri_box, const int* col_start, int num_items, const int* item_start, uint32_t* pair_voxel,
                   int* pair_tri, void* stream)
{
	VGrid G;
	if (!make_grid(voxel_size, min_bound, n0, n1, n2, &G) || num_faces < 0 || num_items < 0 || num_items > GSR_VOXEL_MAX_ITEMS ||
	    (num_items > 0 && (!vertices || !faces || !tri_box || !col_start || !item_start || !pair_voxel || !pair_tri || num_faces < 1)))
		return GSR_ERR_ARG;
	if (num_items > 0)
		hipLaunchKernelGGL(vox_items<true>, dim3(blocks(num_items)), dim3(256), 0, (hipStream_t)stream, vertices, faces, num_faces, G,
		                   tri_box, col_start, num_items, (int*)nullptr, item_start, reinterpret_cast<int*>(pair_voxel), pair_tri,
		                   (unsigned long long*)nullptr);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_voxel_sort(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const uint32_t* pair_voxel, const int* pair_tri_in, int num_pairs,
                   int n0, int n1, int n2, uint32_t* voxel_index, int* pair_start, int* pair_tri, int* grid_index, uint32_t* occupancy,
                   int* num_voxels, void* stream)
{
	const double zero[3] = {0, 0, 0};
	VGrid G;
	if (!make_grid(1.0, zero, n0, n1, n2, &G) || num_pairs < 0 || num_pairs > GSR_VOXEL_MAX_ITEMS || !num_voxels || !pair_start ||
	    (num_pairs > 0 && (!pair_voxel || !pair_tri_in || !voxel_index || !pair_tri)))
		return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const int n = num_pairs;
	const long long nn = (long long)n0 * n1 * n2;
	if (occupancy) GSR_TRY(hipMemsetAsync(occupancy, 0, (size_t)((nn + 31) / 32) * 4, s));
	if (n == 0) {
		GSR_TRY(hipMemsetAsync(pair_start, 0, sizeof(int), s));
		*num_voxels = 0;
		return GSR_OK;
	}
	int *k0, *v0, *head, *rank;
	SortBufs<int> sb;   // sb.part serves the scan of the head flags too
	auto carve = [&](Arena& ws) {
		k0 = ws.take<int>(n); v0 = ws.take<int>(n); sb = sort_take<int>(ws, n, n);
		head = ws.take<int>(n); rank = ws.take<int>((size_t)n + 1);
	};
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;
	GSR_TRY(hipMemcpyAsync(k0, pair_voxel, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
	GSR_TRY(hipMemcpyAsync(v0, pair_tri_in, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
	int rc = radix_sort(k0, v0, n, bits_for(nn), sb, s);
	if (rc) return rc;
	hipLaunchKernelGGL(vox_heads, dim3(blocks(n)), dim3(256), 0, s, k0, n, head);
	rc = exclusive_scan(head, n, rank, sb.part, s);
	if (rc) return rc;
	hipLaunchKernelGGL(vox_compact, dim3(blocks(n)), dim3(256), 0, s, k0, v0, n, head, rank, n1, n2, voxel_index, pair_start, pair_tri,
	                   grid_index, occupancy);
	GSR_TRY(hipMemcpyAsync(num_voxels, rank + n, sizeof(int), hipMemcpyDeviceToHost, s));
	GSR_TRY(hipStreamSynchronize(s));
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_voxel_closest(const double* vertices, int num_vertices, const int* faces, int num_faces, const float* vertex_colors,
                      double voxel_size, const double* min_bound, int n0, int n1, int n2, const uint32_t* voxel_index,
                      const int* pair_start, const int* pair_tri, int num_voxels, int* closest_tri, double* closest_uvw, float* color,
                      void* stream)
{
	VGrid G;
	if (!make_grid(voxel_size, min_bound, n0, n1, n2, &G) || num_vertices < 0 || num_faces < 0 || num_voxels < 0 ||
	    (color && !vertex_colors) ||
	    (num_voxels > 0 && (!vertices || !faces || !voxel_index || !pair_start || !pair_tri || !closest_tri || !closest_uvw)))
		return GSR_ERR_ARG;
	if (num_voxels > 0)
		hipLaunchKernelGGL(vox_closest, dim3((unsigned)((num_voxels + 3) / 4)), dim3(256), 0, (hipStream_t)stream, vertices, num_vertices,
		                   faces, num_faces, vertex_colors, G, voxel_index, pair_start, pair_tri, num_voxels, closest_tri, closest_uvw,
		                   color);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

}  // extern "C"
