// gsr_mesh_clean.hip -- the --clean stage of gaustudio/scripts/extract_mesh.py:149-186 on the device: what the script takes
// from Open3D (TriangleMesh::ClusterConnectedTriangles, the per-cluster areas, RemoveTrianglesByMask and
// RemoveUnreferencedVertices), for the mesh that TSDFVolume.extract_triangle_mesh_device() leaves in HBM.
//
// Contract:
//   * two triangles are adjacent when they share an undirected edge {min(a, b), max(a, b)}; a shared vertex alone does not
//     connect, an edge with more than two triangles connects all of them, a triangle that repeats an index behaves as its
//     three literal edges say;
//   * clusters are numbered in ascending order of their lowest triangle index (the order in which Open3D's scan over the
//     triangles opens them): the result is a pure function of `faces`;
//   * a triangle's area is 0.5 |(v1 - v0) x (v2 - v0)| in fp64 from the f32 vertices; a cluster's area is the sum over its
//     triangles in a fixed order (below);
//   * compaction keeps faces and referenced vertices in their original order.
//
// MI355X design:
//   * edge_emit: one lane per face corner -> ((min << b) | max, triangle) pairs, b = bits_for(V); index check.
//   * a stable LSD radix sort (gsr_sort.h) over the 2 b significant key bits; equal-key neighbours of the sorted list are
//     the union edges (a chain through every edge's triangles), compacted into one (u, v) list by a flag scan.
//   * connected components of the triangle graph: synchronous FastSV (Zhang, Azad, Hu 2020: stochastic hooking, aggressive
//     hooking, shortcutting).  One round = two kernels: cc_hook (one lane per union edge, integer atomicMin into `next`,
//     reading only the parents f and grandparents gf that the round before left) and cc_jump (one lane per triangle:
//     f = next, gf = next[next], the following round's `next` = gf, a per-round "changed" word for f or gf).  Nothing a kernel reads
//     is written by the same launch except through atomicMin on `next`, which nobody reads in that launch: correctness
//     never depends on one workgroup seeing another's stores inside a launch, and no workgroup waits on another.  The host
//     reads the "changed" words back once per batch of CC_BATCH rounds and stops after the first round that changed
//     nothing; the rounds of a batch past that one are no-ops.  The number of rounds grows with log F, not the diameter.
//     The fixed point gives every triangle the lowest triangle index of its component, whatever the scheduling.
//   * renumbering: a flag scan over the roots (f[t] == t) -> cluster index; counts by integer atomicAdd, one per distinct
//     cluster of a wave (the lanes of a wave that hold the same cluster are counted with ballots first).
//   * areas: a stable radix sort of the triangle ids by cluster index; every cluster is cut into pieces of AREA_PIECE
//     consecutive triangles of that order; one wave per piece (lane l adds elements l, l + 64, ... in order, then a fixed
//     shuffle tree), then one lane per cluster adds its pieces in order.  A fixed order: bit-identical from run to run.
//   * compaction: byte / int flag stores of the value 1, two int scans, gather.
// Plain HIP C++.  No float atomics and no inline assembly; the only atomics are integer vector atomics (atomicMin on the
// labels, atomicAdd on the counts, atomicOr on a status word, the LDS histogram of the radix sort).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsrast.h"
#include "gsr_sort.h"

namespace {

constexpr int CC_BATCH = 4;          // rounds enqueued between two reads of the "changed" words
constexpr int CC_MAX_ROUNDS = 4096;  // never reached (FastSV needs O(log F) rounds); a bound on the host loop
constexpr int AREA_PIECE = 1024;     // triangles per partial sum

// ------------------------------------------------------------------------------------------------------ union edges
// corner i = 3 t + k holds the edge (faces[t, k], faces[t, (k + 1) % 3]) of triangle t
__global__ void __launch_bounds__(256) edge_emit(const int* __restrict__ faces, int n, int V, int vbits, uint64_t* __restrict__ keys,
                                                 int* __restrict__ vals, int* status)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int t = i / 3, k = i - 3 * t;
	int a = faces[i], b = faces[3 * t + (k == 2 ? 0 : k + 1)];
	if (a < 0 || a >= V || b < 0 || b >= V) {
		atomicOr(status, 1);
		a = b = 0;
	}
	keys[i] = ((uint64_t)(uint32_t)min(a, b) << vbits) | (uint64_t)(uint32_t)max(a, b);
	vals[i] = t;
}
__global__ void __launch_bounds__(256) edge_flag(const uint64_t* __restrict__ keys, const int* __restrict__ vals, int n, int* __restrict__ flag)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	flag[i] = (i + 1 < n && keys[i] == keys[i + 1] && vals[i] != vals[i + 1]) ? 1 : 0;
}
__global__ void __launch_bounds__(256) edge_compact(const int* __restrict__ vals, const int* __restrict__ flag, const int* __restrict__ off,
                                                    int n, int2* __restrict__ edges)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n || !flag[i]) return;
	edges[off[i]] = make_int2(vals[i], vals[i + 1]);
}

// ------------------------------------------------------------------------------------------------------ connected components
__global__ void __launch_bounds__(256) cc_init(int F, int* __restrict__ f, int* __restrict__ gf, int* __restrict__ next)
{
	const int t = blockIdx.x * 256 + threadIdx.x;
	if (t >= F) return;
	f[t] = t; gf[t] = t; next[t] = t;
}
// `next` enters the round holding gf (the shortcut); both directions of every union edge hook into it.  f and gf are not
// written in this launch and `next` is not read in it.  f[x] <= x and gf[x] <= f[x] always: a hook with gf[u] == gf[v] is a no-op.
__global__ void __launch_bounds__(256) cc_hook(const int2* __restrict__ edges, int E, const int* __restrict__ f, const int* __restrict__ gf,
                                               int* __restrict__ next)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= E) return;
	const int2 e = edges[i];
	const int gu = gf[e.x], gv = gf[e.y];
	if (gu == gv) return;
	if (gv < gu) {
		atomicMin(&next[f[e.x]], gv);
		atomicMin(&next[e.x], gv);
	} else {
		atomicMin(&next[f[e.y]], gu);
		atomicMin(&next[e.y], gu);
	}
}
// f = next, gf = f[f]; next2 (the other buffer: `next` is read here at other lanes' indices) = gf for the following round
__global__ void __launch_bounds__(256) cc_jump(int F, const int* __restrict__ next, int* __restrict__ f, int* __restrict__ gf,
                                               int* __restrict__ next2, int* changed)
{
	const int t = blockIdx.x * 256 + threadIdx.x;
	if (t >= F) return;
	const int p = next[t];
	const int g = next[p];
	const bool ch = g != gf[t] || p != f[t];
	f[t] = p; gf[t] = g; next2[t] = g;
	const uint64_t m = __ballot(ch);
	if (ch && (m & ((1ull << (threadIdx.x & 63)) - 1)) == 0) atomicOr(changed, 1);   // the first such lane of the wave
}

// ------------------------------------------------------------------------------------------------------ renumbering and counts
__global__ void __launch_bounds__(256) root_flag(const int* __restrict__ f, int F, int* __restrict__ flag)
{
	const int t = blockIdx.x * 256 + threadIdx.x;
	if (t < F) flag[t] = f[t] == t ? 1 : 0;
}
__global__ void __launch_bounds__(256) cluster_assign(const int* __restrict__ f, const int* __restrict__ rank, int F,
                                                      int* __restrict__ clusters, int* __restrict__ counts)
{
	const int t = blockIdx.x * 256 + threadIdx.x;
	const bool valid = t < F;
	const int c = valid ? rank[f[t]] : -1;
	if (valid) clusters[t] = c;
	// one atomicAdd per distinct cluster of the wave
	const int lane = threadIdx.x & 63;
	bool pending = valid;
	while (true) {
		const uint64_t todo = __ballot(pending);
		if (todo == 0) break;
		const int leader = __ffsll((unsigned long long)todo) - 1;
		const int lc = __shfl(c, leader);
		const uint64_t same = __ballot(pending && c == lc);
		if (lane == leader) atomicAdd(&counts[lc], __popcll(same));
		if (c == lc) pending = false;
	}
}

// ------------------------------------------------------------------------------------------------------ areas
__global__ void __launch_bounds__(256) area_emit(const int* __restrict__ clusters, int F, int C, uint64_t* __restrict__ keys,
                                                 int* __restrict__ vals, int* status)
{
	const int t = blockIdx.x * 256 + threadIdx.x;
	if (t >= F) return;
	int c = clusters[t];
	if (c < 0 || c >= C) {
		atomicOr(status, 1);
		c = 0;
	}
	keys[t] = (uint64_t)(uint32_t)c;
	vals[t] = t;
}
// area[j] of the j-th triangle in (cluster, triangle) order; the range of every cluster
__global__ void __launch_bounds__(256) area_tri(const float* __restrict__ verts, int V, const int* __restrict__ faces,
                                                const uint64_t* __restrict__ keys, const int* __restrict__ tris, int F,
                                                double* __restrict__ area, int2* __restrict__ ranges, int* status)
{
	const int j = blockIdx.x * 256 + threadIdx.x;
	if (j >= F) return;
	const int c = (int)keys[j];
	if (j == 0 || (int)keys[j - 1] != c) ranges[c].x = j;
	if (j == F - 1 || (int)keys[j + 1] != c) ranges[c].y = j + 1;
	const int t = tris[j];
	const int i0 = faces[3 * (size_t)t], i1 = faces[3 * (size_t)t + 1], i2 = faces[3 * (size_t)t + 2];
	if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) {
		atomicOr(status, 1);
		area[j] = 0.0;
		return;
	}
	const double x0 = verts[3 * (size_t)i0], y0 = verts[3 * (size_t)i0 + 1], z0 = verts[3 * (size_t)i0 + 2];
	const double ax = (double)verts[3 * (size_t)i1] - x0, ay = (double)verts[3 * (size_t)i1 + 1] - y0, az = (double)verts[3 * (size_t)i1 + 2] - z0;
	const double bx = (double)verts[3 * (size_t)i2] - x0, by = (double)verts[3 * (size_t)i2 + 1] - y0, bz = (double)verts[3 * (size_t)i2 + 2] - z0;
	const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
	area[j] = 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}
__global__ void __launch_bounds__(256) piece_count(const int2* __restrict__ ranges, int C, int* __restrict__ npieces)
{
	const int c = blockIdx.x * 256 + threadIdx.x;
	if (c < C) npieces[c] = (ranges[c].y - ranges[c].x + AREA_PIECE - 1) / AREA_PIECE;
}
// one wave per piece: the piece's cluster by a binary search in the piece offsets (poff[C] = number of pieces)
__global__ void __launch_bounds__(256) piece_sum(const double* __restrict__ area, const int2* __restrict__ ranges,
                                                 const int* __restrict__ poff, int C, int P, double* __restrict__ partial)
{
	const int piece = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (piece >= P) return;
	int lo = 0, hi = C - 1;   // the last cluster with poff[c] <= piece: the one with poff[c] <= piece < poff[c + 1]
	while (lo < hi) {
		const int mid = (lo + hi + 1) >> 1;
		if (poff[mid] <= piece) lo = mid;
		else hi = mid - 1;
	}
	const int2 r = ranges[lo];
	const int b = r.x + (piece - poff[lo]) * AREA_PIECE, e = min(b + AREA_PIECE, r.y);
	double s = 0.0;
	for (int j = b + lane; j < e; j += 64) s += area[j];
	for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);   // a + b == b + a: every lane holds the same bits
	if (lane == 0) partial[piece] = s;
}
__global__ void __launch_bounds__(256) cluster_sum(const double* __restrict__ partial, const int* __restrict__ poff, int C,
                                                   double* __restrict__ out)
{
	const int c = blockIdx.x * 256 + threadIdx.x;
	if (c >= C) return;
	double s = 0.0;
	for (int p = poff[c]; p < poff[c + 1]; p++) s += partial[p];
	out[c] = s;
}

// ------------------------------------------------------------------------------------------------------ compaction
__global__ void __launch_bounds__(256) keep_mark(const int* __restrict__ faces, const unsigned char* __restrict__ keep, int F, int V,
                                                 int* __restrict__ fflag, int* __restrict__ vflag, int* status)
{
	const int t = blockIdx.x * 256 + threadIdx.x;
	if (t >= F) return;
	const int i0 = faces[3 * (size_t)t], i1 = faces[3 * (size_t)t + 1], i2 = faces[3 * (size_t)t + 2];
	const bool k = keep[t] != 0;
	fflag[t] = k ? 1 : 0;
	if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) {
		atomicOr(status, 1);
		return;
	}
	if (k) { vflag[i0] = 1; vflag[i1] = 1; vflag[i2] = 1; }
}
__global__ void __launch_bounds__(256) compact_faces(const int* __restrict__ faces, const int* __restrict__ fflag, const int* __restrict__ foff,
                                                     const int* __restrict__ voff, int F, int* __restrict__ out_faces,
                                                     int* __restrict__ face_index)
{
	const int t = blockIdx.x * 256 + threadIdx.x;
	if (t >= F || !fflag[t]) return;
	const int o = foff[t];
	out_faces[3 * (size_t)o] = voff[faces[3 * (size_t)t]];
	out_faces[3 * (size_t)o + 1] = voff[faces[3 * (size_t)t + 1]];
	out_faces[3 * (size_t)o + 2] = voff[faces[3 * (size_t)t + 2]];
	face_index[o] = t;
}
__global__ void __launch_bounds__(256) compact_verts(const float* __restrict__ verts, const int* __restrict__ vflag, const int* __restrict__ voff,
                                                     int V, float* __restrict__ out_verts, int* __restrict__ vertex_index)
{
	const int v = blockIdx.x * 256 + threadIdx.x;
	if (v >= V || !vflag[v]) return;
	const int o = voff[v];
	vertex_index[o] = v;
	if (verts) {
		out_verts[3 * (size_t)o] = verts[3 * (size_t)v];
		out_verts[3 * (size_t)o + 1] = verts[3 * (size_t)v + 1];
		out_verts[3 * (size_t)o + 2] = verts[3 * (size_t)v + 2];
	}
}

}  // namespace

extern "C" {

int gsr_mesh_cluster_triangles(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const int* faces, int num_faces, int num_verts,
                               int* triangle_clusters, int* cluster_n_triangles, int* rounds, void* stream)
{
	if (rounds) *rounds = 0;
	if (num_faces < 0 || num_verts < 0 || num_faces > 0x7fffffff / 3) return GSR_ERR_ARG;
	if (num_faces == 0) return 0;
	if (!faces || !triangle_clusters || !cluster_n_triangles || num_verts == 0) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const int F = num_faces, n = 3 * F;
	const int vbits = bits_for(num_verts);

	int *status, *v0, *flag, *off, *part, *f, *gf, *next, *next2;
	uint64_t* k0;
	SortBufs<uint64_t> sb;
	auto carve = [&](Arena& ws) {
		status = ws.take<int>(1 + CC_BATCH);   // [0] = a bad index, [1 ..] = the "changed" words of a batch of rounds
		k0 = ws.take<uint64_t>(n);
		v0 = ws.take<int>(n);
		sb = sort_take<uint64_t>(ws, n);
		flag = ws.take<int>(n);
		off = ws.take<int>((size_t)n + 1);
		part = ws.take<int>(scan_part_len(n));
		f = ws.take<int>(F);
		gf = ws.take<int>(F);
		next = ws.take<int>(F);
		next2 = ws.take<int>(F);
	};
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;
	int* changed = status + 1;

	// the (edge, triangle) pairs, sorted by edge; the index check before anything is written
	GSR_TRY(hipMemsetAsync(status, 0, sizeof(int) * (1 + CC_BATCH), s));
	hipLaunchKernelGGL(edge_emit, dim3(blocks(n)), dim3(256), 0, s, faces, n, num_verts, vbits, k0, v0, status);
	int rc = read_status(status, s);
	if (rc) return rc;
	rc = radix_sort(k0, v0, n, 2 * vbits, sb, s);
	if (rc) return rc;
	hipLaunchKernelGGL(edge_flag, dim3(blocks(n)), dim3(256), 0, s, k0, v0, n, flag);
	rc = exclusive_scan<int>(flag, n, off, part, s);
	if (rc) return rc;
	int E = 0;
	GSR_TRY(hipMemcpyAsync(&E, off + n, sizeof(int), hipMemcpyDeviceToHost, s));
	hipLaunchKernelGGL(cc_init, dim3(blocks(F)), dim3(256), 0, s, F, f, gf, next);
	GSR_TRY(hipStreamSynchronize(s));
	// the sorted keys are dead from here: their first buffer holds the compacted union edges (E <= n - 1 pairs of 8 bytes)
	// (radix_sort leaves the buffer that does not hold the result in sb.k1)
	int2* edges = reinterpret_cast<int2*>(sb.k1);
	if (E > 0) {
		hipLaunchKernelGGL(edge_compact, dim3(blocks(n)), dim3(256), 0, s, v0, flag, off, n, edges);
	}

	// FastSV rounds in batches of CC_BATCH, until one round changes nothing
	int nrounds = 0;
	bool done = E == 0;
	while (!done) {
		if (nrounds >= CC_MAX_ROUNDS) return GSR_ERR_HIP;
		GSR_TRY(hipMemsetAsync(changed, 0, sizeof(int) * CC_BATCH, s));
		for (int r = 0; r < CC_BATCH; r++) {
			hipLaunchKernelGGL(cc_hook, dim3(blocks(E)), dim3(256), 0, s, edges, E, f, gf, next);
			hipLaunchKernelGGL(cc_jump, dim3(blocks(F)), dim3(256), 0, s, F, next, f, gf, next2, changed + r);
			int* t = next; next = next2; next2 = t;
		}
		int ch[CC_BATCH];
		GSR_TRY(hipMemcpyAsync(ch, changed, sizeof(int) * CC_BATCH, hipMemcpyDeviceToHost, s));
		GSR_TRY(hipStreamSynchronize(s));
		for (int r = 0; r < CC_BATCH && !done; r++) {
			nrounds++;
			done = ch[r] == 0;
		}
	}
	if (rounds) *rounds = nrounds;

	// roots -> cluster indices in ascending root order; counts
	hipLaunchKernelGGL(root_flag, dim3(blocks(F)), dim3(256), 0, s, f, F, flag);
	rc = exclusive_scan<int>(flag, F, off, part, s);
	if (rc) return rc;
	int C = 0;
	GSR_TRY(hipMemcpyAsync(&C, off + F, sizeof(int), hipMemcpyDeviceToHost, s));
	GSR_TRY(hipStreamSynchronize(s));
	GSR_TRY(hipMemsetAsync(cluster_n_triangles, 0, sizeof(int) * (size_t)C, s));
	hipLaunchKernelGGL(cluster_assign, dim3(blocks(F)), dim3(256), 0, s, f, off, F, triangle_clusters, cluster_n_triangles);
	GSR_TRY(hipGetLastError());
	return C;
}

int gsr_mesh_cluster_area(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* verts, int num_verts, const int* faces,
                          int num_faces, const int* triangle_clusters, int num_clusters, double* cluster_area, void* stream)
{
	if (num_faces < 0 || num_verts < 0 || num_clusters < 0 || num_clusters > num_faces) return GSR_ERR_ARG;
	if (num_clusters == 0) return num_faces == 0 ? GSR_OK : GSR_ERR_ARG;
	if (!verts || !faces || !triangle_clusters || !cluster_area) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const int F = num_faces, C = num_clusters;
	const long long max_pieces = (long long)F / AREA_PIECE + C;

	int *status, *v0, *npieces, *poff, *part;
	uint64_t* k0;
	SortBufs<uint64_t> sb;
	double *area, *partial;
	int2* ranges;
	auto carve = [&](Arena& ws) {
		status = ws.take<int>(1);
		k0 = ws.take<uint64_t>(F);
		v0 = ws.take<int>(F);
		sb = sort_take<uint64_t>(ws, F);
		area = ws.take<double>(F);
		ranges = ws.take<int2>(C);
		npieces = ws.take<int>(C);
		poff = ws.take<int>((size_t)C + 1);
		part = ws.take<int>(scan_part_len(C));
		partial = ws.take<double>(max_pieces);
	};
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;

	GSR_TRY(hipMemsetAsync(status, 0, sizeof(int), s));
	GSR_TRY(hipMemsetAsync(ranges, 0, sizeof(int2) * (size_t)C, s));
	hipLaunchKernelGGL(area_emit, dim3(blocks(F)), dim3(256), 0, s, triangle_clusters, F, C, k0, v0, status);
	int rc = radix_sort(k0, v0, F, bits_for(C), sb, s);
	if (rc) return rc;
	hipLaunchKernelGGL(area_tri, dim3(blocks(F)), dim3(256), 0, s, verts, num_verts, faces, k0, v0, F, area, ranges, status);
	hipLaunchKernelGGL(piece_count, dim3(blocks(C)), dim3(256), 0, s, ranges, C, npieces);
	rc = exclusive_scan<int>(npieces, C, poff, part, s);
	if (rc) return rc;
	int P = 0;
	GSR_TRY(hipMemcpyAsync(&P, poff + C, sizeof(int), hipMemcpyDeviceToHost, s));
	rc = read_status(status, s);   // a cluster index outside [0, num_clusters) or a face index outside [0, num_verts)
	if (rc) return rc;
	if (P > max_pieces) return GSR_ERR_ARG;
	if (P > 0) hipLaunchKernelGGL(piece_sum, dim3((P + 3) / 4), dim3(256), 0, s, area, ranges, poff, C, P, partial);
	hipLaunchKernelGGL(cluster_sum, dim3(blocks(C)), dim3(256), 0, s, partial, poff, C, cluster_area);
	GSR_TRY(hipGetLastError());
	return GSR_OK;
}

int gsr_mesh_compact(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* verts, int num_verts, const int* faces,
                     int num_faces, const unsigned char* keep, float* out_verts, int* out_faces, int* vertex_index, int* face_index,
                     int* num_verts_out, void* stream)
{
	if (num_verts_out) *num_verts_out = 0;
	if (num_faces < 0 || num_verts < 0 || num_faces > 0x7fffffff / 3) return GSR_ERR_ARG;
	if (num_faces == 0) return 0;
	if (!faces || !keep || !out_faces || !face_index || num_verts == 0 || !vertex_index || (verts && !out_verts)) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const int F = num_faces, V = num_verts;
	const int m = F > V ? F : V;

	int *status, *fflag, *foff, *vflag, *voff, *part;
	auto carve = [&](Arena& ws) {
		status = ws.take<int>(1);
		fflag = ws.take<int>(F);
		foff = ws.take<int>((size_t)F + 1);
		vflag = ws.take<int>(V);
		voff = ws.take<int>((size_t)V + 1);
		part = ws.take<int>(scan_part_len(m));
	};
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;

	GSR_TRY(hipMemsetAsync(status, 0, sizeof(int), s));
	GSR_TRY(hipMemsetAsync(vflag, 0, sizeof(int) * (size_t)V, s));
	hipLaunchKernelGGL(keep_mark, dim3(blocks(F)), dim3(256), 0, s, faces, keep, F, V, fflag, vflag, status);
	int rc = exclusive_scan<int>(fflag, F, foff, part, s);
	if (rc) return rc;
	rc = exclusive_scan<int>(vflag, V, voff, part, s);
	if (rc) return rc;
	int nf = 0, nv = 0;
	GSR_TRY(hipMemcpyAsync(&nf, foff + F, sizeof(int), hipMemcpyDeviceToHost, s));
	GSR_TRY(hipMemcpyAsync(&nv, voff + V, sizeof(int), hipMemcpyDeviceToHost, s));
	rc = read_status(status, s);   // a face index outside [0, num_verts): nothing is written
	if (rc) return rc;
	hipLaunchKernelGGL(compact_faces, dim3(blocks(F)), dim3(256), 0, s, faces, fflag, foff, voff, F, out_faces, face_index);
	hipLaunchKernelGGL(compact_verts, dim3(blocks(V)), dim3(256), 0, s, verts, vflag, voff, V, out_verts, vertex_index);
	GSR_TRY(hipGetLastError());
	if (num_verts_out) *num_verts_out = nv;
	return nf;
}

}  // extern "C"
