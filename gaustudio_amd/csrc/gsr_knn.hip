// gsr_knn.hip -- exact k-nearest neighbours, normal fusion and point-cloud outlier removal on the GPU: the part of
// gs-extract-pcd that follows the render loop (gaustudio/scripts/extract_pcd.py:45-51 clean_point_cloud, :108-183
// normal_fusion), which the reference runs on the CPU (scipy cKDTree + a Python loop per point; Open3D).
//
// MI355X design:
//   * kNN: a hashed sparse grid (64-bit cell keys, open addressing, table of 2^ceil(log2 2N) slots), so points on a
//     surface, tight clusters, duplicates and far outliers cost O(N) memory whatever the bounding box.  The cell size is
//     chosen by measuring the occupied-cell count (a few insert passes, one host read each) until a cell holds ~k/2
//     points on average.  Points are placed cell-contiguously by a count -> atomic offset -> scatter pass; the order
//     inside a cell and of the cells does not matter, because every result is ordered by (fp64 squared distance, index).
//   * One wave per query, one lane per result slot (k <= 64): the wave visits the cells of the shells r = 0..2 around the
//     query cell, 64 candidates at a time, and stops when the k-th distance is below the distance to the scanned cube.
//     A query that is not settled after shell 2 (sparse regions, far outliers, N close to k) scans the list of occupied
//     cells, pruned by the distance to each cell's box.
//   * Fusion: records {id, normal, weight} are grouped by id with a stable LSD radix sort (8-bit counting-sort passes),
//     so each id's records are reduced in record order (view order, then pixel order), one lane per id, in fp64: no
//     float atomics, bit-identical output from run to run.
//   * Cleaning: fixed-shape fp64 block reductions for the mean and the standard deviation of the mean kNN distance.
//   * 3-NN mean distance (simple-knn's distCUDA2): the same grid at ~4 points per cell, one LANE per point in
//     cell order, three fp64 distances in registers, shells 0..2; what is not settled then goes through the wave-per-query kNN.
// All memory is caller-owned or obtained through the gsr_alloc_fn callback; the entry points are stateless.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/gsrast.h"
#include "gsr_sort.h"

namespace {

constexpr uint64_t EMPTY = ~0ull;
constexpr int CELL_BITS = 21;
constexpr int CELL_MAX = (1 << CELL_BITS) - 1;
constexpr int SHELL_MAX = 2;            // shells scanned around the query cell before the full cell scan
constexpr int NO_INDEX = 0x7fffffff;
constexpr int DIST3_CELL_TARGET = 4;    // points per occupied cell for dist3_query (DESIGN.md s19 has the measurements)

struct Grid {
	double ox, oy, oz;   // origin (bounding-box minimum)
	double h, inv_h;     // cell size
	double margin;       // slack for the rounding of the cell assignment (1e-6 cells)
	uint64_t mask;       // table size - 1
};

__host__ __device__ __forceinline__ uint64_t cell_key(int x, int y, int z)
{
	return ((uint64_t)x << 42) | ((uint64_t)y << 21) | (uint64_t)z;
}
__device__ __forceinline__ uint64_t mix64(uint64_t x)
{
	x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
	x ^= x >> 27; x *= 0x94d049bb133111ebull;
	x ^= x >> 31;
	return x;
}
__device__ __forceinline__ int cell_of(float p, double o, double inv_h)
{
	const double c = floor(((double)p - o) * inv_h);
	return (int)fmin(fmax(c, 0.0), (double)CELL_MAX);
}
// the query's cell, not clamped to the grid (a query may lie outside it); kept within int range
__device__ __forceinline__ int qcell_of(float p, double o, double inv_h)
{
	const double c = floor(((double)p - o) * inv_h);
	return (int)fmin(fmax(c, -(double)(1 << 24)), (double)(1 << 24));
}
__device__ __forceinline__ int find_slot(const unsigned long long* keys, uint64_t mask, uint64_t key)
{
	uint64_t slot = mix64(key) & mask;
	for (uint64_t probe = 0; probe <= mask; probe++) {
		const unsigned long long k = keys[slot];
		if (k == key) return (int)slot;
		if (k == EMPTY) return -1;
		slot = (slot + 1) & mask;
	}
	return -1;
}
__device__ __forceinline__ int ordered(float f)
{
	const int i = __float_as_int(f);
	return i >= 0 ? i : i ^ 0x7fffffff;
}
__host__ __forceinline__ float unordered(int i)
{
	const int b = i >= 0 ? i : i ^ 0x7fffffff;
	float f;
	memcpy(&f, &b, 4);
	return f;
}

// ------------------------------------------------------------------------------------------------------ grid build
// bbox[0..2] = ordered min, [3..5] = ordered max, [6] = 1 if a coordinate is not finite
__global__ void __launch_bounds__(256) bbox_kernel(const float* __restrict__ pts, int n, int* __restrict__ bbox)
{
	__shared__ int red[6][256];
	int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, mx[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
	int bad = 0;
	for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
		for (int a = 0; a < 3; a++) {
			const float v = pts[3 * (size_t)i + a];
			if (!isfinite(v)) { bad = 1; continue; }
			mn[a] = min(mn[a], ordered(v));
			mx[a] = max(mx[a], ordered(v));
		}
	}
	for (int a = 0; a < 3; a++) { red[a][threadIdx.x] = mn[a]; red[3 + a][threadIdx.x] = mx[a]; }
	__syncthreads();
	for (int s = 128; s > 0; s >>= 1) {
		if ((int)threadIdx.x < s)
			for (int a = 0; a < 3; a++) {
				red[a][threadIdx.x] = min(red[a][threadIdx.x], red[a][threadIdx.x + s]);
				red[3 + a][threadIdx.x] = max(red[3 + a][threadIdx.x], red[3 + a][threadIdx.x + s]);
			}
		__syncthreads();
	}
	if (threadIdx.x < 3) atomicMin(&bbox[threadIdx.x], red[threadIdx.x][0]);
	else if (threadIdx.x < 6) atomicMax(&bbox[threadIdx.x], red[threadIdx.x][0]);
	if (bad) atomicOr(&bbox[6], 1);
}

// inserts every point's cell; cnt[slot] = points in the cell, counters[0] = occupied cells
__global__ void __launch_bounds__(256) grid_insert(const float* __restrict__ pts, int n, Grid g, unsigned long long* keys,
                                                   int* __restrict__ pslot, int* cnt, int* counters)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int cx = cell_of(pts[3 * (size_t)i], g.ox, g.inv_h), cy = cell_of(pts[3 * (size_t)i + 1], g.oy, g.inv_h),
	          cz = cell_of(pts[3 * (size_t)i + 2], g.oz, g.inv_h);
	const uint64_t key = cell_key(cx, cy, cz);
	uint64_t slot = mix64(key) & g.mask;
	for (;;) {   // the table has >= 2 n slots: an empty slot is always found
		unsigned long long k = keys[slot];
		if (k == EMPTY) {
			k = atomicCAS(&keys[slot], (unsigned long long)EMPTY, (unsigned long long)key);
			if (k == EMPTY) { atomicAdd(&counters[0], 1); break; }
		}
		if (k == key) break;
		slot = (slot + 1) & g.mask;
	}
	pslot[i] = (int)slot;
	atomicAdd(&cnt[slot], 1);
}

// start[slot] = first position of the cell's points; cells[] = the occupied slots (any order)
__global__ void __launch_bounds__(256) grid_offsets(const unsigned long long* __restrict__ keys, const int* __restrict__ cnt,
                                                    uint64_t size, int* __restrict__ start, int* __restrict__ cells, int* counters)
{
	const uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (s >= size || keys[s] == EMPTY) return;
	start[s] = atomicAdd(&counters[1], cnt[s]);
	cells[atomicAdd(&counters[2], 1)] = (int)s;
}

__global__ void __launch_bounds__(256) grid_scatter(const float* __restrict__ pts, int n, const int* __restrict__ pslot,
                                                    const int* __restrict__ start, int* fill, float4* __restrict__ spts)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int s = pslot[i];
	const int pos = start[s] + atomicAdd(&fill[s], 1);
	spts[pos] = make_float4(pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], __int_as_float(i));
}

// ------------------------------------------------------------------------------------------------------ kNN query
__device__ __forceinline__ bool lex_less(double a, int ia, double b, int ib) { return a < b || (a == b && ia < ib); }

struct WaveTopK {
	double bd;   // this lane's slot (lane < k): ascending (bd, bi); empty = (+inf, NO_INDEX)
	int bi;
	double td;   // the k-th slot, wave-uniform
	int ti;
};

// offers one candidate per lane (valid lanes only) to the wave's sorted list; every lane must call it
__device__ __forceinline__ void offer(WaveTopK& t, int k, int lane, bool valid, double cd, int ci)
{
	uint64_t m = __ballot(valid && lex_less(cd, ci, t.td, t.ti));
	while (m) {
		const int src = __ffsll((unsigned long long)m) - 1;
		m &= m - 1;
		const double xd = __shfl(cd, src);
		const int xi = __shfl(ci, src);
		if (!lex_less(xd, xi, t.td, t.ti)) continue;   // the k-th slot moved below it (uniform)
		const uint64_t gm = __ballot(lane < k && lex_less(xd, xi, t.bd, t.bi));
		const int pos = __ffsll((unsigned long long)gm) - 1;
		const double ud = __shfl_up(t.bd, 1);
		const int ui = __shfl_up(t.bi, 1);
		if (lane > pos && lane < k) { t.bd = ud; t.bi = ui; }
		if (lane == pos) { t.bd = xd; t.bi = xi; }
		t.td = __shfl(t.bd, k - 1);
		t.ti = __shfl(t.bi, k - 1);
	}
}

// each lane names one cell (start cs, count cc; cc = 0 for none): the wave walks their points 64 at a time
__device__ __forceinline__ void scan_cells(WaveTopK& t, int k, int lane, int cs, int cc, const float4* __restrict__ spts,
                                           float qx, float qy, float qz)
{
	int incl = cc;
	for (int o = 1; o < 64; o <<= 1) {
		const int y = __shfl_up(incl, o);
		if (lane >= o) incl += y;
	}
	const int total = __shfl(incl, 63);
	for (int base = 0; base < total; base += 64) {
		const int e = base + lane;
		int lo = 0;   // owner lane of candidate e = number of lanes whose inclusive count is <= e
		for (int step = 32; step > 0; step >>= 1) {
			const int v = __shfl(incl, lo + step - 1);
			if (v <= e) lo += step;
		}
		const int o_start = __shfl(cs, lo), o_incl = __shfl(incl, lo), o_cnt = __shfl(cc, lo);
		const bool valid = e < total;
		double d2 = 0.0;
		int ci = NO_INDEX;
		if (valid) {
			const float4 p = spts[o_start + (e - (o_incl - o_cnt))];
			const double dx = (double)p.x - (double)qx, dy = (double)p.y - (double)qy, dz = (double)p.z - (double)qz;
			d2 = dx * dx + dy * dy + dz * dz;
			ci = __float_as_int(p.w);
		}
		offer(t, k, lane, valid, d2, ci);
	}
}

// one wave per query; writes dist2[q*k + j], idx[q*k + j] for j < k in ascending (dist2, index) order
__global__ void __launch_bounds__(256) knn_query(Grid g, const unsigned long long* __restrict__ keys, const int* __restrict__ start,
                                                 const int* __restrict__ cnt, const int* __restrict__ cells, int ncells,
                                                 const float4* __restrict__ spts, const float* __restrict__ queries, int nq, int k,
                                                 double* __restrict__ dist2, int64_t* __restrict__ idx, int* __restrict__ qbad)
{
	const int lane = threadIdx.x & 63;
	const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (q >= nq) return;   // wave-uniform
	const float qx = queries[3 * (size_t)q], qy = queries[3 * (size_t)q + 1], qz = queries[3 * (size_t)q + 2];
	if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) {   // wave-uniform: no distance to order by; the host reports it
		if (lane == 0) atomicOr(qbad, 1);
		return;
	}
	const int cx = qcell_of(qx, g.ox, g.inv_h), cy = qcell_of(qy, g.oy, g.inv_h), cz = qcell_of(qz, g.oz, g.inv_h);
	WaveTopK t{HUGE_VAL, NO_INDEX, HUGE_VAL, NO_INDEX};
	bool done = false;
	for (int r = 0; r <= SHELL_MAX && !done; r++) {
		const int side = 2 * r + 1, ncube = side * side * side;
		for (int b = 0; b < ncube; b += 64) {
			const int e = b + lane;
			int cs = 0, cc = 0;
			if (e < ncube) {
				const int ox = e % side - r, oy = (e / side) % side - r, oz = e / (side * side) - r;
				const int x = cx + ox, y = cy + oy, z = cz + oz;
				const bool shell = max(abs(ox), max(abs(oy), abs(oz))) == r;
				if (shell && x >= 0 && y >= 0 && z >= 0 && x <= CELL_MAX && y <= CELL_MAX && z <= CELL_MAX) {
					const int s = find_slot(keys, g.mask, cell_key(x, y, z));
					if (s >= 0) { cs = start[s]; cc = cnt[s]; }
				}
			}
			scan_cells(t, k, lane, cs, cc, spts, qx, qy, qz);
		}
		if (t.ti != NO_INDEX) {   // full: every unseen point lies outside the scanned cube, at least `bound` away
			const double lx = (double)qx - (g.ox + (cx - r) * g.h), hx = g.ox + (cx + r + 1) * g.h - (double)qx;
			const double ly = (double)qy - (g.oy + (cy - r) * g.h), hy = g.oy + (cy + r + 1) * g.h - (double)qy;
			const double lz = (double)qz - (g.oz + (cz - r) * g.h), hz = g.oz + (cz + r + 1) * g.h - (double)qz;
			const double bound = fmin(fmin(fmin(lx, hx), fmin(ly, hy)), fmin(lz, hz)) - g.margin;
			done = bound > 0.0 && t.td < bound * bound;
		}
	}
	if (!done) {   // the full scan over the occupied cells outside the cube already scanned
		for (int b = 0; b < ncells; b += 64) {
			const int e = b + lane;
			int cs = 0, cc = 0;
			if (e < ncells) {
				const int s = cells[e];
				const uint64_t key = keys[s];
				const int x = (int)(key >> 42), y = (int)((key >> 21) & CELL_MAX), z = (int)(key & CELL_MAX);
				const bool scanned = max(abs(x - cx), max(abs(y - cy), abs(z - cz))) <= SHELL_MAX;
				double dx = fmax(fmax(g.ox + x * g.h - g.margin - (double)qx, (double)qx - (g.ox + (x + 1) * g.h + g.margin)), 0.0);
				double dy = fmax(fmax(g.oy + y * g.h - g.margin - (double)qy, (double)qy - (g.oy + (y + 1) * g.h + g.margin)), 0.0);
				double dz = fmax(fmax(g.oz + z * g.h - g.margin - (double)qz, (double)qz - (g.oz + (z + 1) * g.h + g.margin)), 0.0);
				const bool far = t.ti != NO_INDEX && dx * dx + dy * dy + dz * dz > t.td;
				if (!scanned && !far) { cs = start[s]; cc = cnt[s]; }
			}
			scan_cells(t, k, lane, cs, cc, spts, qx, qy, qz);
		}
	}
	if (lane < k) {
		dist2[(size_t)q * k + lane] = t.bd;
		idx[(size_t)q * k + lane] = t.bi == NO_INDEX ? -1 : t.bi;
	}
}

// ------------------------------------------------------------------------------------------------------ 3-NN mean distance
// simple-knn's distCUDA2 / calculate_dist2_python (gaustudio/models/vanilla_sg.py:9-14): the mean of the squared distances to
// the three nearest OTHER points.  One lane per sorted position of spts, so the 64 lanes of a wave lie in the same few cells
// and walk nearly the same cell lists (their loads hit the same lines).  Only the three smallest VALUES are kept (six VGPRs,
// a min / max insertion network, no index): ties need no order, and the order the atomics gave the points inside a cell
// does not reach the result.  No LDS; every loop is bounded by a cell count or the table mask.
struct Best3 {
	double d1, d2, d3;   // ascending; +inf = empty
};
__device__ __forceinline__ void insert3(Best3& b, double d)
{
	const double t = fmax(b.d1, d);
	b.d1 = fmin(b.d1, d);
	const double u = fmax(b.d2, t);
	b.d2 = fmin(b.d2, t);
	b.d3 = fmin(b.d3, u);
}

// the cells at Chebyshev distance R of (cx, cy, cz)
template <int R>
__device__ __forceinline__ void scan_shell3(Best3& b, const Grid& g, const unsigned long long* __restrict__ keys,
                                            const int* __restrict__ start, const int* __restrict__ cnt,
                                            const float4* __restrict__ spts, int cx, int cy, int cz, double qx, double qy, double qz,
                                            int self)
{
	constexpr int side = 2 * R + 1, ncube = side * side * side;
#pragma unroll 1
	for (int e = 0; e < ncube; e++) {
		const int ox = e % side - R, oy = (e / side) % side - R, oz = e / (side * side) - R;
		if (max(abs(ox), max(abs(oy), abs(oz))) != R) continue;
		const int x = cx + ox, y = cy + oy, z = cz + oz;
		if (x < 0 || y < 0 || z < 0 || x > CELL_MAX || y > CELL_MAX || z > CELL_MAX) continue;
		const int s = find_slot(keys, g.mask, cell_key(x, y, z));
		if (s < 0) continue;
		const int c0 = start[s], c1 = c0 + cnt[s];
		for (int j = c0; j < c1; j++) {
			const float4 p = spts[j];
			if (__float_as_int(p.w) == self) continue;
			const double dx = (double)p.x - qx, dy = (double)p.y - qy, dz = (double)p.z - qz;
			insert3(b, dx * dx + dy * dy + dz * dz);
		}
	}
}

// knn_query's settle test: every unseen point lies outside the cube of shells 0..r, at least `bound` away
__device__ __forceinline__ bool settled3(const Best3& b, const Grid& g, int cx, int cy, int cz, int r, double qx, double qy, double qz)
{
	if (b.d3 == HUGE_VAL) return false;
	const double lx = qx - (g.ox + (cx - r) * g.h), hx = g.ox + (cx + r + 1) * g.h - qx;
	const double ly = qy - (g.oy + (cy - r) * g.h), hy = g.oy + (cy + r + 1) * g.h - qy;
	const double lz = qz - (g.oz + (cz - r) * g.h), hz = g.oz + (cz + r + 1) * g.h - qz;
	const double bound = fmin(fmin(fmin(lx, hx), fmin(ly, hy)), fmin(lz, hz)) - g.margin;
	return bound > 0.0 && b.d3 < bound * bound;
}

// stat[0] = lanes that needed shell 2, stat[1] = lanes left unsettled: their original indices go to leftover[] (any order)
__global__ void __launch_bounds__(256) dist3_query(Grid g, const unsigned long long* __restrict__ keys, const int* __restrict__ start,
                                                   const int* __restrict__ cnt, const float4* __restrict__ spts, int n,
                                                   float* __restrict__ out, int* __restrict__ leftover, int* stat)
{
	const int pos = blockIdx.x * 256 + threadIdx.x;
	if (pos >= n) return;
	const float4 q = spts[pos];
	const int self = __float_as_int(q.w);
	const double qx = q.x, qy = q.y, qz = q.z;
	const int cx = cell_of(q.x, g.ox, g.inv_h), cy = cell_of(q.y, g.oy, g.inv_h), cz = cell_of(q.z, g.oz, g.inv_h);
	Best3 b{HUGE_VAL, HUGE_VAL, HUGE_VAL};
	scan_shell3<0>(b, g, keys, start, cnt, spts, cx, cy, cz, qx, qy, qz, self);
	scan_shell3<1>(b, g, keys, start, cnt, spts, cx, cy, cz, qx, qy, qz, self);
	bool done = settled3(b, g, cx, cy, cz, 1, qx, qy, qz);
	const uint64_t m = __ballot(!done);   // one atomic per wave for the count
	if (!done && (int)(threadIdx.x & 63) == __ffsll((unsigned long long)m) - 1) atomicAdd(&stat[0], __popcll(m));
	if (!done) {
		scan_shell3<2>(b, g, keys, start, cnt, spts, cx, cy, cz, qx, qy, qz, self);
		done = settled3(b, g, cx, cy, cz, 2, qx, qy, qz);
	}
	if (done) out[self] = (float)(((b.d1 + b.d2) + b.d3) / 3.0);
	else leftover[atomicAdd(&stat[1], 1)] = self;
}

// the leftovers' kNN rows (k = 4, entry 0 is the point itself or a duplicate of it: distance 0, the minimum) into out
__global__ void __launch_bounds__(256) dist3_fold(const double* __restrict__ d2, const int* __restrict__ leftover, int m,
                                                  float* __restrict__ out)
{
	const int j = blockIdx.x * 256 + threadIdx.x;
	if (j >= m) return;
	const double* d = d2 + 4 * (size_t)j;
	out[leftover[j]] = (float)(((d[1] + d[2]) + d[3]) / 3.0);
}

// ------------------------------------------------------------------------------------------------------ host helpers
uint64_t table_size(int n)
{
	uint64_t s = 64;
	while (s < 2 * (uint64_t)n) s <<= 1;
	return s;
}

// the hashed grid over `pts`: its buffers (grid_take) and what grid_build finds
struct GridBufs {
	Grid g;
	unsigned long long* keys;
	int *cnt, *start, *fill, *pslot, *cells;
	float4* spts;
	int* counters;   // [0..2] the build's, [3] a query that is not finite, [4..6] dist3_query's, [8..14] the bounding box
	int occupied, ncells;
};
void grid_take(Arena& ws, int n, GridBufs& gb)
{
	const uint64_t T = table_size(n);
	gb.keys = ws.take<unsigned long long>(T);
	gb.cnt = ws.take<int>(T);
	gb.start = ws.take<int>(T);
	gb.fill = ws.take<int>(T);
	gb.pslot = ws.take<int>(n);
	gb.cells = ws.take<int>(n);
	gb.spts = ws.take<float4>(n);
	gb.counters = ws.take<int>(16);
}

// builds the grid with ~m_target points per occupied cell (and no more than CELL_MAX cells along an axis)
int grid_build(GridBufs& gb, const float* pts, int n, double m_target, hipStream_t s)
{
	const uint64_t T = table_size(n);
	unsigned long long* keys = gb.keys;
	int *cnt = gb.cnt, *start = gb.start, *fill = gb.fill, *pslot = gb.pslot, *cells = gb.cells, *counters = gb.counters;

	int bbox_init[7] = {0x7fffffff, 0x7fffffff, 0x7fffffff, (int)0x80000000, (int)0x80000000, (int)0x80000000, 0};
	GSR_TRY(hipMemcpyAsync(counters + 8, bbox_init, sizeof(bbox_init), hipMemcpyHostToDevice, s));
	const int nb = (n + 255) / 256;
	hipLaunchKernelGGL(bbox_kernel, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, s, pts, n, counters + 8);
	GSR_TRY(hipGetLastError());
	int bbox[7];
	GSR_TRY(hipMemcpyAsync(bbox, counters + 8, sizeof(bbox), hipMemcpyDeviceToHost, s));
	GSR_TRY(hipStreamSynchronize(s));
	if (bbox[6]) return GSR_ERR_NONFINITE;
	double lo[3], ext = 0.0;
	for (int a = 0; a < 3; a++) {
		lo[a] = unordered(bbox[a]);
		ext = fmax(ext, (double)unordered(bbox[3 + a]) - lo[a]);
	}
	const double h_min = ext / (CELL_MAX - 1);
	double h = ext > 0.0 ? fmax(ext / cbrt(fmax((double)n / m_target, 1.0)), h_min) : 1.0;
	Grid g{lo[0], lo[1], lo[2], h, 1.0 / h, 1e-6 * h, T - 1};
	int occupied = 0;
	for (int it = 0;; it++) {
		g.h = h; g.inv_h = 1.0 / h; g.margin = 1e-6 * h;
		GSR_TRY(hipMemsetAsync(keys, 0xff, T * 8, s));
		GSR_TRY(hipMemsetAsync(cnt, 0, T * 4, s));
		GSR_TRY(hipMemsetAsync(counters, 0, 8 * sizeof(int), s));
		hipLaunchKernelGGL(grid_insert, dim3(nb), dim3(256), 0, s, pts, n, g, keys, pslot, cnt, counters);
		GSR_TRY(hipGetLastError());
		GSR_TRY(hipMemcpyAsync(&occupied, counters, sizeof(int), hipMemcpyDeviceToHost, s));
		GSR_TRY(hipStreamSynchronize(s));
		const double ratio = m_target / ((double)n / (double)(occupied > 0 ? occupied : 1));
		if (it >= 7 || ext == 0.0 || (ratio >= 0.5 && ratio <= 2.0) || (ratio < 1.0 && h <= h_min)) break;
		h = fmax(h * fmin(fmax(pow(ratio, 1.0 / 2.5), 1.0 / 16.0), 16.0), h_min);
	}
	GSR_TRY(hipMemsetAsync(fill, 0, T * 4, s));
	hipLaunchKernelGGL(grid_offsets, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, keys, cnt, T, start, cells, counters);
	hipLaunchKernelGGL(grid_scatter, dim3(nb), dim3(256), 0, s, pts, n, pslot, start, fill, gb.spts);
	int ncells = 0;
	GSR_TRY(hipMemcpyAsync(&ncells, counters + 2, sizeof(int), hipMemcpyDeviceToHost, s));
	GSR_TRY(hipStreamSynchronize(s));
	gb.g = g; gb.occupied = occupied; gb.ncells = ncells;
	return GSR_OK;
}

// answers the queries from a built grid, one wave per query
int knn_answer(const GridBufs& gb, const float* queries, int nq, int k, double* dist2, int64_t* idx, bool check_queries, hipStream_t s)
{
	if (nq > 0)   // counters[3] (zeroed with the grid's counters): set by a query that is not finite
		hipLaunchKernelGGL(knn_query, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, s, gb.g, gb.keys, gb.start, gb.cnt, gb.cells, gb.ncells,
		                   gb.spts, queries, nq, k, dist2, idx, gb.counters + 3);
	GSR_TRY(hipGetLastError());
	if (nq > 0 && check_queries) {
		int qbad = 0;
		GSR_TRY(hipMemcpyAsync(&qbad, gb.counters + 3, sizeof(int), hipMemcpyDeviceToHost, s));
		GSR_TRY(hipStreamSynchronize(s));
		if (qbad) return GSR_ERR_NONFINITE_QUERY;
	}
	return GSR_OK;
}

// builds the grid over `pts` in gb's buffers (grid_take(.., n, ..)) and answers the queries
int knn_run(GridBufs& gb, const float* pts, int n, const float* queries, int nq, int k, double* dist2, int64_t* idx,
            hipStream_t s)
{
	const int rc = grid_build(gb, pts, n, fmin(fmax(k * 0.5, 8.0), 32.0), s);   // ~k/2 points per occupied cell
	if (rc) return rc;
	return knn_answer(gb, queries, nq, k, dist2, idx, queries != pts, s);   // the points themselves were checked with the bounding box
}

// ------------------------------------------------------------------------------------------------------ fusion
// record = 5 words {id (int), n.x, n.y, n.z, w}
__global__ void __launch_bounds__(256) fusion_records(const float* __restrict__ xyz, int P, const int* __restrict__ ids,
                                                      const float* __restrict__ normals, const float* __restrict__ conf, int n,
                                                      float tx, float ty, float tz, int* __restrict__ rec, int* status)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int id = ids[i];
	const float nx = normals[3 * (size_t)i], ny = normals[3 * (size_t)i + 1], nz = normals[3 * (size_t)i + 2];
	double w = 0.0;
	if (id < 0 || id >= P) {
		atomicOr(status, 1);
	} else {   // extract_pcd.py:118-126: w = conf * |dot(v / |v|, n)| / (|v| + 1e-6), v = t - xyz[id]
		const double vx = (double)tx - (double)xyz[3 * (size_t)id], vy = (double)ty - (double)xyz[3 * (size_t)id + 1],
		             vz = (double)tz - (double)xyz[3 * (size_t)id + 2];
		const double d = sqrt(vx * vx + vy * vy + vz * vz);
		const double vw = fabs((vx / d) * nx + (vy / d) * ny + (vz / d) * nz);
		w = (double)conf[i] * vw * (1.0 / (d + 1e-6));
	}
	int* r = rec + 5 * (size_t)i;
	r[0] = id;
	r[1] = __float_as_int(nx);
	r[2] = __float_as_int(ny);
	r[3] = __float_as_int(nz);
	r[4] = __float_as_int((float)w);
}

__global__ void __launch_bounds__(256) sort_init(const int* __restrict__ rec, int n, int* __restrict__ keys, int* __restrict__ vals)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	keys[i] = rec[5 * (size_t)i];
	vals[i] = i;
}

__global__ void __launch_bounds__(256) unique_flags(const int* __restrict__ keys, int n, int* __restrict__ flags)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) flags[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}
__global__ void __launch_bounds__(256) unique_emit(const int* __restrict__ keys, int n, const int* __restrict__ flags,
                                                   const int* __restrict__ uidx, int* __restrict__ seg, int* __restrict__ unique_ids)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	if (flags[i]) { seg[uidx[i]] = i; unique_ids[uidx[i]] = keys[i]; }
	if (i == n - 1) seg[uidx[n]] = n;
}

// one lane per fused id: the two passes of extract_pcd.py:130-168 over its records in record order, fp64
__global__ void __launch_bounds__(256) fusion_reduce(const int* __restrict__ rec, const int* __restrict__ order,
                                                     const int* __restrict__ seg, int U, float consistency, float* __restrict__ mean)
{
	const int u = blockIdx.x * 256 + threadIdx.x;
	if (u >= U) return;
	const int b = seg[u], e = seg[u + 1];
	double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
	for (int j = b; j < e; j++) {
		const int* r = rec + 5 * (size_t)order[j];
		const double w = __int_as_float(r[4]);
		sx += (double)__int_as_float(r[1]) * w;
		sy += (double)__int_as_float(r[2]) * w;
		sz += (double)__int_as_float(r[3]) * w;
		sw += w;
	}
	double mx = sx / sw, my = sy / sw, mz = sz / sw;
	double nrm = fmax(sqrt(mx * mx + my * my + mz * mz), 1e-12);
	mx /= nrm; my /= nrm; mz /= nrm;
	const double c = (double)consistency;
	sx = sy = sz = sw = 0.0;
	for (int j = b; j < e; j++) {
		const int* r = rec + 5 * (size_t)order[j];
		const double nx = __int_as_float(r[1]), ny = __int_as_float(r[2]), nz = __int_as_float(r[3]);
		const double dx = nx - mx, dy = ny - my, dz = nz - mz;
		if (!(sqrt(dx * dx + dy * dy + dz * dz) < c)) continue;
		const double w = __int_as_float(r[4]);
		sx += nx * w;
		sy += ny * w;
		sz += nz * w;
		sw += w;
	}
	mx = sx / sw; my = sy / sw; mz = sz / sw;   // no consistent record: 0/0 = NaN, kept
	nrm = fmax(sqrt(mx * mx + my * my + mz * mz), 1e-12);
	mean[3 * (size_t)u] = (float)(mx / nrm);
	mean[3 * (size_t)u + 1] = (float)(my / nrm);
	mean[3 * (size_t)u + 2] = (float)(mz / nrm);
}

__global__ void __launch_bounds__(256) gather_points(const float* __restrict__ xyz, const int* __restrict__ ids, int U,
                                                     float* __restrict__ q)
{
	const int u = blockIdx.x * 256 + threadIdx.x;
	if (u >= U) return;
	const size_t id = (size_t)ids[u];
	q[3 * (size_t)u] = xyz[3 * id];
	q[3 * (size_t)u + 1] = xyz[3 * id + 1];
	q[3 * (size_t)u + 2] = xyz[3 * id + 2];
}

// extract_pcd.py:173-179: s = sum_j mean[idx_j] * exp(-d_j / sigma) in fp64, cast to fp32, F.normalize (eps 1e-12)
__global__ void __launch_bounds__(256) fusion_smooth(const float* __restrict__ mean, const double* __restrict__ d2,
                                                     const int64_t* __restrict__ nbr, int U, int k, double sigma,
                                                     float* __restrict__ out)
{
	const int u = blockIdx.x * 256 + threadIdx.x;
	if (u >= U) return;
	double sx = 0.0, sy = 0.0, sz = 0.0;
	for (int j = 0; j < k; j++) {
		const size_t v = (size_t)nbr[(size_t)u * k + j];
		const double w = exp(-sqrt(d2[(size_t)u * k + j]) / sigma);
		sx += (double)mean[3 * v] * w;
		sy += (double)mean[3 * v + 1] * w;
		sz += (double)mean[3 * v + 2] * w;
	}
	const float fx = (float)sx, fy = (float)sy, fz = (float)sz;
	const float nrm = fmaxf(sqrtf(fx * fx + fy * fy + fz * fz), 1e-12f);
	out[3 * (size_t)u] = fx / nrm;
	out[3 * (size_t)u + 1] = fy / nrm;
	out[3 * (size_t)u + 2] = fz / nrm;
}

// ------------------------------------------------------------------------------------------------------ cleaning
__global__ void __launch_bounds__(256) mean_knn_dist(const double* __restrict__ d2, int n, int k, double* __restrict__ a)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	double s = 0.0;
	for (int j = 0; j < k; j++) s += sqrt(d2[(size_t)i * k + j]);
	a[i] = s / k;
}

// per 256-element tile: sum over a_i > 0 of (a_i - centre)^pow (pow 1 or 2) and the count, fixed tree shape
__global__ void __launch_bounds__(256) stat_partials(const double* __restrict__ a, int n, const double* centre, int pw,
                                                     double* __restrict__ psum, int* __restrict__ pcnt)
{
	__shared__ double rs[256];
	__shared__ int rc[256];
	const int i = blockIdx.x * 256 + threadIdx.x;
	const double c = pw == 2 ? centre[0] : 0.0;
	double v = 0.0;
	int m = 0;
	if (i < n && a[i] > 0.0) {
		v = pw == 2 ? (a[i] - c) * (a[i] - c) : a[i];
		m = 1;
	}
	rs[threadIdx.x] = v;
	rc[threadIdx.x] = m;
	__syncthreads();
	for (int w = 128; w > 0; w >>= 1) {
		if ((int)threadIdx.x < w) { rs[threadIdx.x] += rs[threadIdx.x + w]; rc[threadIdx.x] += rc[threadIdx.x + w]; }
		__syncthreads();
	}
	if (threadIdx.x == 0) { psum[blockIdx.x] = rs[0]; pcnt[blockIdx.x] = rc[0]; }
}
// stats[0] = mean, stats[1] = threshold mean + ratio * std (Bessel); pw 1 writes stats[0], pw 2 stats[1]
__global__ void __launch_bounds__(256) stat_final(const double* __restrict__ psum, const int* __restrict__ pcnt, int np, int pw,
                                                  double ratio, double* stats)
{
	__shared__ double rs[256];
	__shared__ long long rc[256];
	double v = 0.0;
	long long m = 0;
	for (int j = threadIdx.x; j < np; j += 256) { v += psum[j]; m += pcnt[j]; }
	rs[threadIdx.x] = v;
	rc[threadIdx.x] = m;
	__syncthreads();
	for (int w = 128; w > 0; w >>= 1) {
		if ((int)threadIdx.x < w) { rs[threadIdx.x] += rs[threadIdx.x + w]; rc[threadIdx.x] += rc[threadIdx.x + w]; }
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		if (pw == 1) stats[0] = rs[0] / (double)rc[0];
		else stats[1] = stats[0] + ratio * sqrt(rs[0] / (double)(rc[0] - 1));
	}
}
__global__ void __launch_bounds__(256) stat_mask(const double* __restrict__ a, int n, const double* __restrict__ stats,
                                                 unsigned char* __restrict__ keep)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) keep[i] = (a[i] > 0.0 && a[i] < stats[1]) ? 1 : 0;
}

// extract_pcd.py:30-43: neighbour 0 is taken to be the point itself; mean of acos(|dot|) over the others, fp64
__global__ void __launch_bounds__(256) normal_mask(const double* __restrict__ normals, const int64_t* __restrict__ nbr, int n, int k,
                                                   double threshold, unsigned char* __restrict__ keep)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const double nx = normals[3 * (size_t)i], ny = normals[3 * (size_t)i + 1], nz = normals[3 * (size_t)i + 2];
	double s = 0.0;
	for (int j = 1; j < k; j++) {
		const size_t v = (size_t)nbr[(size_t)i * k + j];
		const double d = normals[3 * v] * nx + normals[3 * v + 1] * ny + normals[3 * v + 2] * nz;
		s += acos(fabs(d));
	}
	const double m = s / (double)(k - 1);   // k == 1: 0/0 = NaN, dropped (np.mean of nothing)
	keep[i] = m < threshold ? 1 : 0;
}

}  // namespace

extern "C" {

int gsr_knn(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* points, int num_points, const float* queries,
            int num_queries, int k, double* dist2, int64_t* indices, void* stream)
{
	if (!queries) { queries = points; num_queries = num_points; }
	if (!points || num_points <= 0 || num_queries < 0 || k < 1 || k > GSR_KNN_MAX_K || k > num_points) return GSR_ERR_ARG;
	if (num_queries > 0 && (!dist2 || !indices)) return GSR_ERR_ARG;
	GridBufs gb;
	if (!ws_carve(workspace_alloc, workspace_ctx, [&](Arena& ws) { grid_take(ws, num_points, gb); })) return GSR_ERR_ALLOC;
	return knn_run(gb, points, num_points, queries, num_queries, k, dist2, indices, (hipStream_t)stream);
}

int gsr_mean_dist3_ex(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* points, int num_points, float* out_dist2,
                      int cell_target, int stats[3], float stage_ms[3], void* stream)
{
	if (!points || num_points < 4 || !out_dist2 || cell_target < 0 || cell_target > 64) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const int n = num_points;
	GridBufs gb;
	int* leftover;
	auto carve = [&](Arena& ws) { grid_take(ws, n, gb); leftover = ws.take<int>(n); };
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;
	hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
	if (stage_ms)
		for (int j = 0; j < 4; j++) GSR_TRY(hipEventCreate(&ev[j]));
	struct EventGuard {
		hipEvent_t* e;
		~EventGuard() { for (int j = 0; j < 4; j++) if (e[j]) (void)hipEventDestroy(e[j]); }
	} guard{ev};
	if (stage_ms) GSR_TRY(hipEventRecord(ev[0], s));
	int rc = grid_build(gb, points, n, cell_target ? (double)cell_target : (double)DIST3_CELL_TARGET, s);
	if (rc) return rc;
	int* stat = gb.counters + 4;   // zeroed with the grid's counters
	if (stage_ms) GSR_TRY(hipEventRecord(ev[1], s));
	hipLaunchKernelGGL(dist3_query, dim3(blocks(n)), dim3(256), 0, s, gb.g, gb.keys, gb.start, gb.cnt, gb.spts, n, out_dist2, leftover, stat);
	GSR_TRY(hipGetLastError());
	if (stage_ms) GSR_TRY(hipEventRecord(ev[2], s));
	int st[2] = {0, 0};
	GSR_TRY(hipMemcpyAsync(st, stat, sizeof(st), hipMemcpyDeviceToHost, s));
	GSR_TRY(hipStreamSynchronize(s));
	const int m = st[1];
	if (m < 0 || m > n) return GSR_ERR_HIP;
	if (m > 0) {   // far outliers, sparse regions, n close to 4: the wave-per-query search, which scans every occupied cell
		float* q;
		double* d2;
		int64_t* nbr;
		auto carve2 = [&](Arena& w2) {
			q = w2.take<float>((size_t)m * 3);
			d2 = w2.take<double>((size_t)m * 4);
			nbr = w2.take<int64_t>((size_t)m * 4);
		};
		if (!ws_carve(workspace_alloc, workspace_ctx, carve2)) return GSR_ERR_ALLOC;
		hipLaunchKernelGGL(gather_points, dim3(blocks(m)), dim3(256), 0, s, points, leftover, m, q);
		rc = knn_answer(gb, q, m, 4, d2, nbr, false, s);
		if (rc) return rc;
		hipLaunchKernelGGL(dist3_fold, dim3(blocks(m)), dim3(256), 0, s, d2, leftover, m, out_dist2);
		GSR_TRY(hipGetLastError());
	}
	if (stage_ms) {
		GSR_TRY(hipEventRecord(ev[3], s));
		GSR_TRY(hipEventSynchronize(ev[3]));
		for (int j = 0; j < 3; j++) GSR_TRY(hipEventElapsedTime(&stage_ms[j], ev[j], ev[j + 1]));
	}
	if (stats) { stats[0] = gb.occupied; stats[1] = st[0]; stats[2] = m; }
	return GSR_OK;
}

int gsr_mean_dist3(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* points, int num_points, float* out_dist2,
                   int stats[3], void* stream)
{
	return gsr_mean_dist3_ex(workspace_alloc, workspace_ctx, points, num_points, out_dist2, 0, stats, nullptr, stream);
}

int gsr_fusion_records(const float* xyz, int num_gaussians, const int* ids, const float* normals, const float* confidences,
                       int num_records, const float w2c_translation[3], int* records, int* status, void* stream)
{
	if (num_records == 0) return GSR_OK;
	if (!xyz || num_gaussians <= 0 || !ids || !normals || !confidences || num_records < 0 || !w2c_translation || !records || !status)
		return GSR_ERR_ARG;
	hipLaunchKernelGGL(fusion_records, dim3(blocks(num_records)), dim3(256), 0, (hipStream_t)stream, xyz, num_gaussians, ids,
	                   normals, confidences, num_records, w2c_translation[0], w2c_translation[1], w2c_translation[2], records, status);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_fusion_group(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const int* records, int num_records, int num_gaussians,
                     float consistency, int* unique_ids, float* mean_normals, void* stream)
{
	if (num_records == 0) return 0;
	if (!records || num_records < 0 || num_gaussians <= 0 || !unique_ids || !mean_normals) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const int n = num_records;
	int *k0, *v0, *flags, *uidx, *seg;
	SortBufs<int> sb;   // sb.part serves the scan of the flags too
	auto carve = [&](Arena& ws) {
		k0 = ws.take<int>(n); v0 = ws.take<int>(n); sb = sort_take<int>(ws, n, (long long)n + 1);
		flags = ws.take<int>(n); uidx = ws.take<int>((size_t)n + 1); seg = ws.take<int>((size_t)n + 1);   // flags, their scan, segments
	};
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;

	hipLaunchKernelGGL(sort_init, dim3(blocks(n)), dim3(256), 0, s, records, n, k0, v0);
	int rc = radix_sort(k0, v0, n, bits_for(num_gaussians), sb, s);
	if (rc) return rc;
	hipLaunchKernelGGL(unique_flags, dim3(blocks(n)), dim3(256), 0, s, k0, n, flags);
	rc = exclusive_scan(flags, n, uidx, sb.part, s);
	if (rc) return rc;
	hipLaunchKernelGGL(unique_emit, dim3(blocks(n)), dim3(256), 0, s, k0, n, flags, uidx, seg, unique_ids);
	int U = 0;
	GSR_TRY(hipMemcpyAsync(&U, uidx + n, sizeof(int), hipMemcpyDeviceToHost, s));
	GSR_TRY(hipStreamSynchronize(s));
	hipLaunchKernelGGL(fusion_reduce, dim3(blocks(U)), dim3(256), 0, s, records, v0, seg, U, consistency, mean_normals);
	GSR_TRY(hipGetLastError());
	return U;
}

int gsr_fusion_smooth(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* xyz, const int* unique_ids,
                      const float* mean_normals, int num_unique, int k, float sigma, float* normals, void* stream)
{
	if (!xyz || !unique_ids || !mean_normals || !normals || k < 1 || k > GSR_KNN_MAX_K || num_unique < k || !(sigma > 0.f))
		return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const int U = num_unique;
	float* q;
	double* d2;
	int64_t* nbr;
	GridBufs gb;
	auto carve = [&](Arena& ws) {
		q = ws.take<float>((size_t)U * 3);
		d2 = ws.take<double>((size_t)U * k);
		nbr = ws.take<int64_t>((size_t)U * k);
		grid_take(ws, U, gb);
	};
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;
	hipLaunchKernelGGL(gather_points, dim3(blocks(U)), dim3(256), 0, s, xyz, unique_ids, U, q);
	const int rc = knn_run(gb, q, U, q, U, k, d2, nbr, s);
	if (rc) return rc;
	hipLaunchKernelGGL(fusion_smooth, dim3(blocks(U)), dim3(256), 0, s, mean_normals, d2, nbr, U, k, (double)sigma, normals);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_outlier_statistical(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* points, int num_points,
                            int nb_neighbors, double std_ratio, unsigned char* keep, double* mean_distance, void* stream)
{
	if (num_points == 0) return GSR_OK;
	if (!points || num_points < 0 || !keep || nb_neighbors < 1 || nb_neighbors > GSR_KNN_MAX_K) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const int n = num_points, k = nb_neighbors < n ? nb_neighbors : n;
	const int np = (n + 255) / 256;
	double *d2, *a, *psum, *stats;
	int64_t* nbr;
	int* pcnt;
	GridBufs gb;
	auto carve = [&](Arena& ws) {
		d2 = ws.take<double>((size_t)n * k);
		nbr = ws.take<int64_t>((size_t)n * k);
		a = ws.take<double>(n);
		psum = ws.take<double>(np);
		pcnt = ws.take<int>(np);
		stats = ws.take<double>(2);
		grid_take(ws, n, gb);
	};
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;
	int rc = knn_run(gb, points, n, points, n, k, d2, nbr, s);
	if (rc) return rc;
	hipLaunchKernelGGL(mean_knn_dist, dim3(np), dim3(256), 0, s, d2, n, k, a);
	hipLaunchKernelGGL(stat_partials, dim3(np), dim3(256), 0, s, a, n, stats, 1, psum, pcnt);
	hipLaunchKernelGGL(stat_final, dim3(1), dim3(256), 0, s, psum, pcnt, np, 1, std_ratio, stats);
	hipLaunchKernelGGL(stat_partials, dim3(np), dim3(256), 0, s, a, n, stats, 2, psum, pcnt);
	hipLaunchKernelGGL(stat_final, dim3(1), dim3(256), 0, s, psum, pcnt, np, 2, std_ratio, stats);
	hipLaunchKernelGGL(stat_mask, dim3(np), dim3(256), 0, s, a, n, stats, keep);
	if (mean_distance) GSR_TRY(hipMemcpyAsync(mean_distance, a, (size_t)n * 8, hipMemcpyDeviceToDevice, s));
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_outlier_normal(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* points, const double* normals,
                       int num_points, int nb_neighbors, double angle_threshold, unsigned char* keep, void* stream)
{
	if (num_points == 0) return GSR_OK;
	if (!points || !normals || num_points < 0 || !keep || nb_neighbors < 1 || nb_neighbors > GSR_KNN_MAX_K) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const int n = num_points, k = nb_neighbors < n ? nb_neighbors : n;
	double* d2;
	int64_t* nbr;
	GridBufs gb;
	auto carve = [&](Arena& ws) {
		d2 = ws.take<double>((size_t)n * k);
		nbr = ws.take<int64_t>((size_t)n * k);
		grid_take(ws, n, gb);
	};
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;
	const int rc = knn_run(gb, points, n, points, n, k, d2, nbr, s);
	if (rc) return rc;
	hipLaunchKernelGGL(normal_mask, dim3(blocks(n)), dim3(256), 0, s, normals, nbr, n, k, angle_threshold, keep);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

}  // extern "C"
