// gsr_anchor.hip -- Scaffold-GS anchor control: the per-offset and per-anchor statistics of a training view, anchor growing by
// voxel level and pruning, as one compaction that carries the Adam moments (its definition to the bit:
// tests/anchor_model.py; design: DESIGN.md s20b).
//
// A level:  cand_kernel (one lane per offset slot: the candidate test, the cell, the cell range by integer min / max) -> scan
// -> read-back {candidates, range, status} -> keys_kernel (cells rebased to the range's corner, packed x-major into as few
// bits as the range needs) -> radix_sort -> head_kernel -> scan -> unique_kernel (distinct cells with the start of their run)
// -> mark_kernel (one lane per EXISTING anchor: binary search of its cell among the distinct candidate cells, a plain store of
// 1 on a hit) -> new_kernel -> scan -> read-back {count} -> tile_max_kernel + cell_max_kernel (the per-cell maximum feature).
// The anchors are never sorted: only the candidates are, and the membership test runs from the anchors' side.
//
// The per-cell maximum walks a run of the sorted candidates that can be as long as the whole list.  tile_max_kernel gives every
// 64-candidate tile of the sorted list the maximum over its LEADING segment (from the tile's first candidate to the next run
// head); a run then is its candidates up to the first tile boundary plus one 128-byte row per further tile.  The maximum is
// taken on an order-preserving integer image of the floats (-0 < +0), so that it does not depend on how a run is cut.
//
// The emit: one lane per source WORD of every tensor for the survivors (gsr_optim.hip's walk), one lane per word of the new
// rows.  No float atomics; the only atomics are integer min / max / or on seven words of a level's header.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsrast.h"
#include "gsr_anchor_plan.h"
#include "gsr_common.h"
#include "gsr_sort.h"
#include "gsr_ws.h"

namespace {

using anchor_plan::KeyPlan;

constexpr unsigned MAX_GRID = 2048;   // 256 CUs x 8 workgroups: the rest is the grid-stride loop
constexpr int FEAT = GSR_ANCHOR_FEAT;
constexpr int TILE = 64;              // candidates per tile of tile_max_kernel: one wave

unsigned capped_grid(unsigned long long work)
{
	const unsigned long long b = (work + 255) / 256;
	return (unsigned)(b < MAX_GRID ? (b ? b : 1) : MAX_GRID);
}

__device__ __forceinline__ float clamp80(float p) { return p < -80.f ? -80.f : (p > 80.f ? 80.f : p); }

// the voxel cell of a coordinate: correctly rounded divide, half to even
__device__ __forceinline__ float cell_of(float p, float cur) { return rintf(p / cur); }
// false for a NaN or an infinity as well
__device__ __forceinline__ bool cell_fits(float c) { return c >= (float)anchor_plan::CELL_MIN && c <= (float)anchor_plan::CELL_MAX; }

// component c of the position an offset slot decodes to: one product, one sum (gsr_scaffold.hip emit), the scale as
// gsr_optim.hip forms it
__device__ __forceinline__ float slot_pos(const float* __restrict__ anchor, const float* __restrict__ offset,
                                          const float* __restrict__ scale_raw, unsigned a, unsigned slot, int c)
{
	const float s = gs_exp(clamp80(scale_raw[6 * (size_t)a + c]));
	return anchor[3 * (size_t)a + c] + offset[3 * (size_t)slot + c] * s;
}

// order-preserving image of a float in the unsigned integers (-0 below +0)
__device__ __forceinline__ uint32_t f2ord(float f)
{
	const uint32_t b = __float_as_uint(f);
	return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// ------------------------------------------------------------------------------------------------------ statistics
__global__ __launch_bounds__(256) void accumulate_kernel(int n, int k, int m, const int* __restrict__ aidx,
                                                         const int* __restrict__ oidx, const float* __restrict__ opacity,
                                                         const float* __restrict__ vg, const int* __restrict__ radii,
                                                         const unsigned char* __restrict__ visible, float* __restrict__ accum,
                                                         int* __restrict__ denom, float* __restrict__ op_accum,
                                                         int* __restrict__ a_denom)
{
	const unsigned total = (unsigned)m + (unsigned)n, stride = gridDim.x * 256u;
	for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += stride) {
		if (i >= (unsigned)m) {
			const unsigned a = i - (unsigned)m;
			if (visible[a]) a_denom[a] = a_denom[a] + 1;
			continue;
		}
		const int a = aidx[i], j = oidx[i];
		if ((unsigned)a >= (unsigned)n || (unsigned)j >= (unsigned)k) continue;
		if (radii[i] > 0) {
			const size_t slot = (size_t)a * k + j;
			const float gx = vg[3 * (size_t)i], gy = vg[3 * (size_t)i + 1];
			accum[slot] = accum[slot] + sqrtf(gx * gx + gy * gy);
			denom[slot] = denom[slot] + 1;
		}
		if (i == 0 || aidx[i - 1] != a) {   // the head of the anchor's run sums it, at most 16 values
			float s = opacity[i];
			for (unsigned e = i + 1; e < (unsigned)m && e < i + 16u && aidx[e] == a; e++) s = s + opacity[e];
			op_accum[a] = op_accum[a] + s;
		}
	}
}

// ------------------------------------------------------------------------------------------------------ a level
struct LevelArgs {
	int n, k;
	int mature_min;
	float grad_min, rand_min, cur;
};

// meta: {lo x y z, hi x y z, status}
__global__ void meta_init_kernel(int* __restrict__ meta)
{
	if (threadIdx.x < 3) meta[threadIdx.x] = INT_MAX;
	else if (threadIdx.x < 6) meta[threadIdx.x] = INT_MIN;
	else if (threadIdx.x == 6) meta[6] = 0;
}

__device__ __forceinline__ bool is_candidate(const LevelArgs& L, unsigned slot, const float* __restrict__ accum,
                                             const int* __restrict__ denom, const float* __restrict__ rnd)
{
	const int d = denom[slot];
	const float avg = d > 0 ? accum[slot] / (float)d : 0.f;
	return avg >= L.grad_min && d > L.mature_min && rnd[slot] > L.rand_min;   // avg: false for a NaN
}

__global__ __launch_bounds__(256) void cand_kernel(LevelArgs L, const float* __restrict__ anchor, const float* __restrict__ offset,
                                                   const float* __restrict__ scale_raw, const float* __restrict__ accum,
                                                   const int* __restrict__ denom, const float* __restrict__ rnd,
                                                   int* __restrict__ flag, int* __restrict__ meta)
{
	const unsigned total = (unsigned)L.n * (unsigned)L.k, stride = gridDim.x * 256u;
	int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
	int bad = 0;
	for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < total; s += stride) {
		const bool cand = is_candidate(L, s, accum, denom, rnd);
		flag[s] = cand ? 1 : 0;
		if (!cand) continue;
		const unsigned a = s / (unsigned)L.k;
		for (int c = 0; c < 3; c++) {
			const float cell = cell_of(slot_pos(anchor, offset, scale_raw, a, s, c), L.cur);
			if (!cell_fits(cell)) { bad = 1; continue; }
			const int ci = (int)cell;
			lo[c] = ci < lo[c] ? ci : lo[c];
			hi[c] = ci > hi[c] ? ci : hi[c];
		}
	}
	for (int o = 32; o > 0; o >>= 1) {
		for (int c = 0; c < 3; c++) {
			const int l = __shfl_xor(lo[c], o), h = __shfl_xor(hi[c], o);
			lo[c] = l < lo[c] ? l : lo[c];
			hi[c] = h > hi[c] ? h : hi[c];
		}
		bad |= __shfl_xor(bad, o);
	}
	if ((threadIdx.x & 63) == 0) {
		for (int c = 0; c < 3; c++) {
			if (lo[c] != INT_MAX) atomicMin(&meta[c], lo[c]);
			if (hi[c] != INT_MIN) atomicMax(&meta[3 + c], hi[c]);
		}
		if (bad) atomicOr(&meta[6], 1);
	}
}

__global__ __launch_bounds__(256) void keys_kernel(LevelArgs L, KeyPlan kp, const float* __restrict__ anchor,
                                                   const float* __restrict__ offset, const float* __restrict__ scale_raw,
                                                   const int* __restrict__ pos, uint64_t* __restrict__ keys, int* __restrict__ vals)
{
	const unsigned total = (unsigned)L.n * (unsigned)L.k, stride = gridDim.x * 256u;
	for (unsigned s = blockIdx.x * 256u + threadIdx.x; s < total; s += stride) {
		const int p = pos[s];
		if (pos[s + 1] == p) continue;
		const unsigned a = s / (unsigned)L.k;
		int cell[3];
		for (int c = 0; c < 3; c++) cell[c] = (int)cell_of(slot_pos(anchor, offset, scale_raw, a, s, c), L.cur);
		keys[p] = anchor_plan::pack_key(kp, cell[0], cell[1], cell[2]);
		vals[p] = (int)s;
	}
}

__global__ __launch_bounds__(256) void head_kernel(const uint64_t* __restrict__ keys, int n, int* __restrict__ head)
{
	const unsigned stride = gridDim.x * 256u;
	for (unsigned j = blockIdx.x * 256u + threadIdx.x; j < (unsigned)n; j += stride)
		head[j] = (j == 0 || keys[j] != keys[j - 1]) ? 1 : 0;
}

// ukey[u], ustart[u] for every distinct key; ustart[U] = n; occ = 0
__global__ __launch_bounds__(256) void unique_kernel(const uint64_t* __restrict__ keys, int n, const int* __restrict__ upos,
                                                     uint64_t* __restrict__ ukey, int* __restrict__ ustart, int* __restrict__ occ)
{
	const unsigned stride = gridDim.x * 256u;
	for (unsigned j = blockIdx.x * 256u + threadIdx.x; j < (unsigned)n; j += stride) {
		occ[j] = 0;
		const int u = upos[j];
		if (upos[j + 1] != u) { ukey[u] = keys[j]; ustart[u] = (int)j; }
		if (j == 0) ustart[upos[n]] = n;
	}
}

struct MarkArgs {
	const int* cells[GSR_ANCHOR_MAX_LEVELS];
	float cur[GSR_ANCHOR_MAX_LEVELS];
	int start[GSR_ANCHOR_MAX_LEVELS + 1];   // first lane of each earlier level behind the n anchors, total at [num]
	int num;
	int n;
};

// one lane per existing anchor: occ[u] = 1 when its cell is candidate cell u.  Several anchors of one cell store the same 1.
__global__ __launch_bounds__(256) void mark_kernel(MarkArgs M, KeyPlan kp, float cur, const float* __restrict__ anchor,
                                                   const uint64_t* __restrict__ ukey, const int* __restrict__ upos, int ncand,
                                                   int* __restrict__ occ)
{
	const unsigned total = (unsigned)M.n + (unsigned)M.start[M.num], stride = gridDim.x * 256u;
	const int nu = upos[ncand];
	for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < total; i += stride) {
		float p[3];
		if (i < (unsigned)M.n) {
			for (int c = 0; c < 3; c++) p[c] = anchor[3 * (size_t)i + c];
		} else {
			const int r = (int)(i - (unsigned)M.n);
			int l = 0;
			for (int q = 1; q < GSR_ANCHOR_MAX_LEVELS; q++) l += (q < M.num && r >= M.start[q]) ? 1 : 0;
			const int* cl = M.cells[l] + 3 * (size_t)(r - M.start[l]);
			for (int c = 0; c < 3; c++) p[c] = (float)cl[c] * M.cur[l];
		}
		int cell[3];
		bool in = true;
		for (int c = 0; c < 3; c++) {
			const float f = cell_of(p[c], cur);
			in = in && f >= (float)kp.lo[c] && f <= (float)kp.hi[c];   // outside the candidates' box: no candidate cell
			cell[c] = in ? (int)f : 0;
		}
		if (!in) continue;
		const uint64_t key = anchor_plan::pack_key(kp, cell[0], cell[1], cell[2]);
		int lo = 0, hi = nu;                  // first u with ukey[u] >= key
		while (lo < hi) {
			const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
			if (ukey[mid] < key) lo = mid + 1; else hi = mid;
		}
		if (lo < nu && ukey[lo] == key) occ[lo] = 1;
	}
}

__global__ __launch_bounds__(256) void new_kernel(const int* __restrict__ occ, const int* __restrict__ upos, int ncand,
                                                  int* __restrict__ nf)
{
	const unsigned stride = gridDim.x * 256u;
	const int nu = upos[ncand];
	for (unsigned u = blockIdx.x * 256u + threadIdx.x; u < (unsigned)ncand; u += stride) nf[u] = ((int)u < nu && !occ[u]) ? 1 : 0;
}

// part[t][c]: the maximum of feature c over the leading segment of tile t of the sorted candidates.  One wave per tile: lanes
// (h, c), h = lane / 32 taking every second candidate.
__global__ __launch_bounds__(256) void tile_max_kernel(const int* __restrict__ head, const int* __restrict__ vals, int ncand, int k,
                                                       const float* __restrict__ feat, uint32_t* __restrict__ part)
{
	const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
	const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
	const long long base = t * TILE;
	if (base >= ncand) return;
	const bool hd = base + lane >= ncand || head[base + lane] != 0;
	const uint64_t mask = __ballot(hd) & ~1ull;
	const int end = mask ? __ffsll((unsigned long long)mask) - 1 : TILE;
	uint32_t m = 0;
	for (int r = h; r < end; r += 2) {
		const unsigned src = (unsigned)vals[base + r] / (unsigned)k;
		const uint32_t v = f2ord(feat[(size_t)src * FEAT + c]);
		m = v > m ? v : m;
	}
	const uint32_t o = (uint32_t)__shfl_xor((int)m, 32);
	m = o > m ? o : m;
	if (h == 0) part[(size_t)t * FEAT + c] = m;
}

// one wave per distinct candidate cell that is new: its cell and the maximum of every feature over its run
__global__ __launch_bounds__(256) void cell_max_kernel(KeyPlan kp, const uint64_t* __restrict__ ukey, const int* __restrict__ ustart,
                                                       const int* __restrict__ upos, const int* __restrict__ npos,
                                                       const int* __restrict__ vals, int ncand, int k,
                                                       const float* __restrict__ feat, const uint32_t* __restrict__ part,
                                                       int* __restrict__ cells, float* __restrict__ out)
{
	const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
	const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
	if (u >= upos[ncand]) return;
	const int row = npos[u];
	if (npos[u + 1] == row) return;
	const int s = ustart[u], e = ustart[u + 1];
	const long long first_end = ((long long)s + TILE - 1) / TILE * TILE;   // s itself when the run starts a tile
	const int ind_end = first_end < e ? (int)first_end : e;
	uint32_t m = 0;
	for (int r = s + h; r < ind_end; r += 2) {
		const unsigned src = (unsigned)vals[r] / (unsigned)k;
		const uint32_t v = f2ord(feat[(size_t)src * FEAT + c]);
		m = v > m ? v : m;
	}
	for (long long t = first_end / TILE + h; t * TILE < e; t += 2) {
		const uint32_t v = part[(size_t)t * FEAT + c];
		m = v > m ? v : m;
	}
	const uint32_t o = (uint32_t)__shfl_xor((int)m, 32);
	m = o > m ? o : m;
	if (h == 0) out[(size_t)row * FEAT + c] = ord2f(m);
	if (lane < 3) {
		int cell[3];
		anchor_plan::unpack_key(kp, ukey[u], cell);
		cells[3 * (size_t)row + lane] = lane == 0 ? cell[0] : (lane == 1 ? cell[1] : cell[2]);
	}
}

// ------------------------------------------------------------------------------------------------------ prune and emit
__global__ __launch_bounds__(256) void prune_kernel(int n, const float* __restrict__ op_accum, const int* __restrict__ a_denom,
                                                    int settled_min, float min_opacity, int* __restrict__ flag)
{
	const unsigned stride = gridDim.x * 256u;
	for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < (unsigned)n; i += stride) {
		const int d = a_denom[i];
		const bool prune = d > settled_min && op_accum[i] < min_opacity * (float)d;
		flag[i] = prune ? 0 : 1;
	}
}

struct EmitTensor {
	const uint32_t* src;
	uint32_t* dst;
	unsigned w;
	int kind;
};
struct EmitArgs {
	EmitTensor t[GSR_ANCHOR_MAX_TENSORS];
	unsigned long long start[GSR_ANCHOR_MAX_TENSORS + 1];   // first word of each tensor in the walk, total at [num]
	int num;
	int n, k;
	int mature_min, settled_min;
};

__device__ __forceinline__ int tensor_of(const EmitArgs& a, unsigned long long T)
{
	int ti = 0;
#pragma unroll
	for (int q = 1; q < GSR_ANCHOR_MAX_TENSORS; q++) ti += (q < a.num && T >= a.start[q]) ? 1 : 0;
	return ti;
}

__global__ __launch_bounds__(256) void emit_old_kernel(EmitArgs a, const int* __restrict__ pos, const int* __restrict__ o_denom,
                                                       const int* __restrict__ a_denom)
{
	const unsigned long long total = a.start[a.num], stride = (unsigned long long)gridDim.x * 256u;
	for (unsigned long long T = (unsigned long long)blockIdx.x * 256u + threadIdx.x; T < total; T += stride) {
		const int ti = tensor_of(a, T);
		const EmitTensor& G = a.t[ti];
		const unsigned e = (unsigned)(T - a.start[ti]), w = G.w;
		const unsigned i = e / w, col = e - i * w;
		const int row = pos[i];
		if (pos[i + 1] == row) continue;
		uint32_t val = G.src[e];
		if (G.kind == GSR_ANCHOR_SLOT_STAT && o_denom[(size_t)i * a.k + col] > a.mature_min) val = 0u;
		if (G.kind == GSR_ANCHOR_ANCHOR_STAT && a_denom[i] > a.settled_min) val = 0u;
		G.dst[(size_t)row * w + col] = val;
	}
}

// the rows of one level's new anchors: tensors 0 .. 4 are anchor, anchor_feat, offset, scale_raw, rot_raw; the rest get 0
__global__ __launch_bounds__(256) void emit_new_kernel(EmitArgs a, const int* __restrict__ pos, int row0, const int* __restrict__ cells,
                                                       const float* __restrict__ feat, float cur, float log_cur)
{
	const unsigned long long total = a.start[a.num], stride = (unsigned long long)gridDim.x * 256u;
	const size_t base = (size_t)pos[a.n] + (size_t)row0;
	for (unsigned long long T = (unsigned long long)blockIdx.x * 256u + threadIdx.x; T < total; T += stride) {
		const int ti = tensor_of(a, T);
		const EmitTensor& G = a.t[ti];
		const unsigned e = (unsigned)(T - a.start[ti]), w = G.w;
		const unsigned r = e / w, col = e - r * w;
		uint32_t val = 0u;
		if (ti == 0) val = __float_as_uint((float)cells[3 * (size_t)r + col] * cur);
		else if (ti == 1) val = __float_as_uint(feat[(size_t)r * FEAT + col]);
		else if (ti == 3) val = __float_as_uint(log_cur);
		else if (ti == 4) val = col == 0 ? __float_as_uint(1.f) : 0u;
		G.dst[(base + r) * w + col] = val;
	}
}

int read_ints(int* host, const int* dev, int count, hipStream_t s)
{
	GSR_TRY(hipMemcpyAsync(host, dev, sizeof(int) * count, hipMemcpyDeviceToHost, s));
	GSR_TRY(hipStreamSynchronize(s));
	return GSR_OK;
}

}  // namespace

extern "C" {

int gsr_anchor_accumulate(int num_anchors, int k, int num_gaussians, const int* anchor_index, const int* offset_index,
                          const float* opacity, const float* viewspace_grad, const int* radii, const unsigned char* visible,
                          float* offset_grad_accum, int* offset_denom, float* opacity_accum, int* anchor_denom, void* stream)
{
	if (!anchor_plan::sizes_ok(num_anchors, k) || num_gaussians < 0 || (long long)num_gaussians > (long long)num_anchors * k)
		return GSR_ERR_ARG;
	if (num_anchors == 0) return GSR_OK;
	if (!visible || !offset_grad_accum || !offset_denom || !opacity_accum || !anchor_denom) return GSR_ERR_ARG;
	if (num_gaussians > 0 && (!anchor_index || !offset_index || !opacity || !viewspace_grad || !radii)) return GSR_ERR_ARG;
	hipLaunchKernelGGL(accumulate_kernel, dim3(capped_grid((unsigned long long)num_anchors + num_gaussians)), dim3(256), 0,
	                   (hipStream_t)stream, num_anchors, k, num_gaussians, anchor_index, offset_index, opacity, viewspace_grad, radii,
	                   visible, offset_grad_accum, offset_denom, opacity_accum, anchor_denom);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_anchor_level(gsr_alloc_fn workspace_alloc, void* workspace_ctx, int num_anchors, int k, const float* anchor,
                     const float* offset, const float* scale_raw, const float* anchor_feat, const float* offset_grad_accum,
                     const int* offset_denom, const float* rand, int mature_min, float grad_min, float rand_min, float cur,
                     const gsr_anchor_cells* prior, int num_prior, int** cells_out, float** feat_out, long long* info_host,
                     void* stream)
{
	if (!anchor_plan::sizes_ok(num_anchors, k) || !workspace_alloc || !cells_out || !feat_out || !info_host) return GSR_ERR_ARG;
	if (!(cur > 0.f) || !isfinite(cur) || grad_min != grad_min || num_prior < 0 || num_prior > GSR_ANCHOR_MAX_LEVELS ||
	    (num_prior > 0 && !prior))
		return GSR_ERR_ARG;
	*cells_out = nullptr;
	*feat_out = nullptr;
	info_host[0] = info_host[1] = 0;
	if (num_anchors == 0) return GSR_OK;
	if (!anchor || !offset || !scale_raw || !anchor_feat || !offset_grad_accum || !offset_denom || !rand) return GSR_ERR_ARG;
	MarkArgs M = {};
	M.n = num_anchors;
	M.num = num_prior;
	long long others = 0;
	for (int l = 0; l < num_prior; l++) {
		if (prior[l].count < 0 || (prior[l].count > 0 && !prior[l].cells) || !(prior[l].cur > 0.f)) return GSR_ERR_ARG;
		M.cells[l] = prior[l].cells;
		M.cur[l] = prior[l].cur;
		M.start[l] = (int)others;
		others += prior[l].count;
		if (num_anchors + others > anchor_plan::MAX_ANCHORS) return GSR_ERR_ARG;
	}
	for (int l = num_prior; l <= GSR_ANCHOR_MAX_LEVELS; l++) M.start[l] = (int)others;

	hipStream_t s = (hipStream_t)stream;
	const long long nk = (long long)num_anchors * k;
	const LevelArgs L = {num_anchors, k, mature_min, grad_min, rand_min, cur};
	int *flag = nullptr, *pos = nullptr, *part = nullptr, *meta = nullptr;
	if (!ws_carve(workspace_alloc, workspace_ctx, [&](Arena& ws) {
		    flag = ws.take<int>((size_t)nk);
		    pos = ws.take<int>((size_t)nk + 1);
		    part = ws.take<int>((size_t)scan_part_len(nk));
		    meta = ws.take<int>(8);
	    }))
		return GSR_ERR_ALLOC;
	hipLaunchKernelGGL(meta_init_kernel, dim3(1), dim3(64), 0, s, meta);
	hipLaunchKernelGGL(cand_kernel, dim3(capped_grid((unsigned long long)nk)), dim3(256), 0, s, L, anchor, offset, scale_raw,
	                   offset_grad_accum, offset_denom, rand, flag, meta);
	int rc = exclusive_scan<int>(flag, (int)nk, pos, part, s);
	if (rc != GSR_OK) return rc;
	int hm[7], ncand = 0;
	GSR_TRY(hipMemcpyAsync(hm, meta, sizeof(hm), hipMemcpyDeviceToHost, s));
	rc = read_ints(&ncand, pos + nk, 1, s);
	if (rc != GSR_OK) return rc;
	if (hm[6]) return GSR_ERR_CELL;
	info_host[0] = ncand;
	if (ncand <= 0) return ncand < 0 ? GSR_ERR_HIP : GSR_OK;
	KeyPlan kp;
	if (!anchor_plan::key_plan(hm, hm + 3, &kp)) return GSR_ERR_HIP;   // the kernel let a cell through that does not fit

	const long long ntiles = ((long long)ncand + TILE - 1) / TILE;
	uint64_t *keys = nullptr, *ukey = nullptr;
	int *vals = nullptr, *head = nullptr, *upos = nullptr, *ustart = nullptr, *occ = nullptr, *nf = nullptr, *npos = nullptr;
	uint32_t* tpart = nullptr;
	SortBufs<uint64_t> sb = {};
	if (!ws_carve(workspace_alloc, workspace_ctx, [&](Arena& ws) {
		    keys = ws.take<uint64_t>((size_t)ncand);
		    vals = ws.take<int>((size_t)ncand);
		    sb = sort_take<uint64_t>(ws, ncand, ncand);
		    ukey = ws.take<uint64_t>((size_t)ncand);
		    head = ws.take<int>((size_t)ncand);
		    upos = ws.take<int>((size_t)ncand + 1);
		    ustart = ws.take<int>((size_t)ncand + 1);
		    occ = ws.take<int>((size_t)ncand);
		    nf = ws.take<int>((size_t)ncand);
		    npos = ws.take<int>((size_t)ncand + 1);
		    tpart = ws.take<uint32_t>((size_t)ntiles * FEAT);
	    }))
		return GSR_ERR_ALLOC;
	const unsigned gc = capped_grid((unsigned long long)ncand);
	hipLaunchKernelGGL(keys_kernel, dim3(capped_grid((unsigned long long)nk)), dim3(256), 0, s, L, kp, anchor, offset, scale_raw, pos,
	                   keys, vals);
	rc = radix_sort<uint64_t>(keys, vals, ncand, kp.bits, sb, s);
	if (rc != GSR_OK) return rc;
	hipLaunchKernelGGL(head_kernel, dim3(gc), dim3(256), 0, s, keys, ncand, head);
	rc = exclusive_scan<int>(head, ncand, upos, sb.part, s);
	if (rc != GSR_OK) return rc;
	hipLaunchKernelGGL(unique_kernel, dim3(gc), dim3(256), 0, s, keys, ncand, upos, ukey, ustart, occ);
	hipLaunchKernelGGL(mark_kernel, dim3(capped_grid((unsigned long long)(num_anchors + others))), dim3(256), 0, s, M, kp, cur, anchor,
	                   ukey, upos, ncand, occ);
	hipLaunchKernelGGL(new_kernel, dim3(gc), dim3(256), 0, s, occ, upos, ncand, nf);
	rc = exclusive_scan<int>(nf, ncand, npos, sb.part, s);
	if (rc != GSR_OK) return rc;
	int count = 0;
	rc = read_ints(&count, npos + ncand, 1, s);
	if (rc != GSR_OK) return rc;
	if (count < 0 || count > ncand) return GSR_ERR_HIP;
	info_host[1] = count;
	if (count == 0) return GSR_OK;

	int* cells = nullptr;
	float* feat = nullptr;
	if (!ws_carve(workspace_alloc, workspace_ctx, [&](Arena& ws) {
		    cells = ws.take<int>(3 * (size_t)count);
		    feat = ws.take<float>((size_t)FEAT * count);
	    }))
		return GSR_ERR_ALLOC;
	hipLaunchKernelGGL(tile_max_kernel, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, s, head, vals, ncand, k, anchor_feat, tpart);
	hipLaunchKernelGGL(cell_max_kernel, dim3((unsigned)(((long long)ncand + 3) / 4)), dim3(256), 0, s, kp, ukey, ustart, upos, npos,
	                   vals, ncand, k, anchor_feat, tpart, cells, feat);
	*cells_out = cells;
	*feat_out = feat;
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_anchor_prune(gsr_alloc_fn workspace_alloc, void* workspace_ctx, int num_anchors, const float* opacity_accum,
                     const int* anchor_denom, int settled_min, float min_opacity, int* pos, int* survivors_host, void* stream)
{
	if (!anchor_plan::sizes_ok(num_anchors, 1) || !workspace_alloc || !pos || !survivors_host || min_opacity != min_opacity)
		return GSR_ERR_ARG;
	if (num_anchors > 0 && (!opacity_accum || !anchor_denom)) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	int *flag = nullptr, *part = nullptr;
	if (!ws_carve(workspace_alloc, workspace_ctx, [&](Arena& ws) {
		    flag = ws.take<int>((size_t)num_anchors + 1);
		    part = ws.take<int>((size_t)scan_part_len(num_anchors));
	    }))
		return GSR_ERR_ALLOC;
	if (num_anchors > 0)
		hipLaunchKernelGGL(prune_kernel, dim3(capped_grid((unsigned long long)num_anchors)), dim3(256), 0, s, num_anchors,
		                   opacity_accum, anchor_denom, settled_min, min_opacity, flag);
	const int rc = exclusive_scan<int>(flag, num_anchors, pos, part, s);
	if (rc != GSR_OK) return rc;
	return read_ints(survivors_host, pos + num_anchors, 1, s);
}

int gsr_anchor_emit(int num_anchors, int k, const gsr_anchor_tensor* tensors, int num_tensors, const int* pos,
                    const int* offset_denom, const int* anchor_denom, int mature_min, int settled_min,
                    const gsr_anchor_cells* levels, const float* const* feat, int num_levels, void* stream)
{
	if (!anchor_plan::sizes_ok(num_anchors, k) || !tensors || num_tensors < 5 || num_tensors > GSR_ANCHOR_MAX_TENSORS || !pos)
		return GSR_ERR_ARG;
	if (num_levels < 0 || num_levels > GSR_ANCHOR_MAX_LEVELS || (num_levels > 0 && (!levels || !feat))) return GSR_ERR_ARG;
	const int want[5] = {3, FEAT, 3 * k, 6, 4};
	long long fresh = 0;
	for (int l = 0; l < num_levels; l++) {
		if (levels[l].count < 0 || (levels[l].count > 0 && (!levels[l].cells || !feat[l])) || !(levels[l].cur > 0.f)) return GSR_ERR_ARG;
		fresh += levels[l].count;
	}
	if (num_anchors + fresh > anchor_plan::MAX_ANCHORS) return GSR_ERR_ARG;
	EmitArgs a = {};
	a.num = num_tensors;
	a.n = num_anchors;
	a.k = k;
	a.mature_min = mature_min;
	a.settled_min = settled_min;
	bool slot_stat = false, anchor_stat = false;
	for (int t = 0; t < num_tensors; t++) {
		const gsr_anchor_tensor& g = tensors[t];
		if (g.width < 1 || g.width > 3 * anchor_plan::MAX_OFFSETS || g.kind < GSR_ANCHOR_COPY || g.kind > GSR_ANCHOR_ANCHOR_STAT)
			return GSR_ERR_ARG;
		if (t < 5 && (g.width != want[t] || g.kind != GSR_ANCHOR_COPY)) return GSR_ERR_ARG;
		if ((g.kind == GSR_ANCHOR_SLOT_STAT && g.width != k) || (g.kind == GSR_ANCHOR_ANCHOR_STAT && g.width != 1)) return GSR_ERR_ARG;
		if (num_anchors > 0 && !g.src) return GSR_ERR_ARG;   // a destination may be NULL only when no row is written: the caller's check
		slot_stat |= g.kind == GSR_ANCHOR_SLOT_STAT;
		anchor_stat |= g.kind == GSR_ANCHOR_ANCHOR_STAT;
		a.t[t].src = static_cast<const uint32_t*>(g.src);
		a.t[t].dst = static_cast<uint32_t*>(g.dst);
		a.t[t].w = (unsigned)g.width;
		a.t[t].kind = g.kind;
	}
	if (num_anchors > 0 && ((slot_stat && !offset_denom) || (anchor_stat && !anchor_denom))) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	auto lay = [&](long long rows) {
		a.start[0] = 0;
		for (int t = 0; t < num_tensors; t++) a.start[t + 1] = a.start[t] + (unsigned long long)rows * a.t[t].w;
		for (int t = num_tensors; t < GSR_ANCHOR_MAX_TENSORS; t++) a.start[t + 1] = a.start[num_tensors];
	};
	if (num_anchors > 0) {
		lay(num_anchors);
		hipLaunchKernelGGL(emit_old_kernel, dim3(capped_grid(a.start[num_tensors])), dim3(256), 0, s, a, pos, offset_denom, anchor_denom);
	}
	long long row0 = 0;
	for (int l = 0; l < num_levels; l++) {
		if (levels[l].count == 0) continue;
		lay(levels[l].count);
		hipLaunchKernelGGL(emit_new_kernel, dim3(capped_grid(a.start[num_tensors])), dim3(256), 0, s, a, pos, (int)row0, levels[l].cells,
		                   feat[l], levels[l].cur, (float)log((double)levels[l].cur));
		row0 += levels[l].count;
	}
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

}  // extern "C"
