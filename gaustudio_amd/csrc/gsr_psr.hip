// gsr_psr.hip -- Shape-as-Points meshing (gs-extract-pcd --meshing sap) on the device: the differentiable Poisson solver DPSR
// of gaustudio/utils/graphics_utils.py:19-333, forward and backward, and a dense indexed marching cubes with vertex normals
// in place of the reference's CPU round trip through skimage.  The two FFTs between the stages stay with torch.fft, which
// differentiates them itself (gaustudio_amd/sap.py).
//
// Contract:
//   * index and weight arithmetic of a point is the reference's fp32 chain, operation for operation (axis_of below);
//   * point_rasterize: per grid node the terms w * val (fp32) of every (point, corner) pair that lands on it are added in
//     fp64 in a fixed order and rounded to fp32 once; weighted = divide (fp32) by the number of pairs, 0 counted as 1;
//   * spectral solve: the reference's fp32 chain per element, the Gaussian filter evaluated in fp64 and cast;
//   * grid_interp: the 8 corner terms lat * w (fp32) added in fp64 in the reference's corner order, rounded once; the mean of
//     the samples is a fixed-order fp64 reduction;
//   * marching cubes: inside iff value < level, tables and cube geometry of gsr_mc_tables.h (constants of the code object, the
//     ones the block volumes read), one vertex per crossing edge owned by the edge's
//     lower node, vertices ordered by (owner node linear index, axis), triangles by (cube linear index, table order).
//
// MI355X design:
//   * rasterize: psr_keys (cell of each point, integer histogram) -> scan -> stable radix sort by cell (gsr_sort.h, only the
//     significant digits) -> psr_permute (points and values in sorted order) -> psr_node_gather: one lane per grid node walks
//     the points of its 8 adjacent cells (wrapped).  A gather: no float atomics, bit-identical from run to run.
//   * spectral, normalize: pure HBM streams, grid-stride loops, 8 / 16 bytes per lane, no LDS.
//   * interp: one lane per point (8 scattered loads), block partial sums in a fixed LDS tree, one block adds the partials.
//   * marching cubes: classify (case + owned-edge flags per node, computed from the node's own neighbours: no atomics) ->
//     two int scans -> emit vertices, emit triangles, emit vertex normals (the same walk as the vertices).
//   * backward: the backward of a scatter is a gather and that of a gather a scatter.
//     rasterize_bwd and interp_bwd are gathers, one lane per point over its 8 corners; the grid gradient of interp IS the
//     forward scatter (gsr_psr_rasterize with one channel), so there is no second scatter.  spectral_bwd and normalize_bwd
//     are streams like their forwards; normalize_bwd also leaves block partials that one block adds into grad_mean.
// Plain HIP C++.  No float atomics, no inline assembly; the only atomics are integer vector atomics (cell histogram, status
// word, the LDS histogram of the radix sort).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/gsrast.h"
#include "gsr_mc_tables.h"
#include "gsr_sort.h"

namespace {

unsigned stream_blocks(long long n) { long long b = (n + 255) / 256; return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b)); }
bool good_res(int r0, int r1, int r2) { return r0 >= 2 && r1 >= 2 && r2 >= 2 && (long long)r0 * r1 * r2 < (1LL << 30); }

struct Res { int r[3]; float cs[3]; float rf[3]; };
Res make_res(int r0, int r1, int r2)
{
	Res R;
	R.r[0] = r0; R.r[1] = r1; R.r[2] = r2;
	for (int d = 0; d < 3; d++) { R.rf[d] = (float)R.r[d]; R.cs[d] = 1.0f / R.rf[d]; }   // cubesize = 1.0 / size (fp32)
	return R;
}

// One axis of graphics_utils.point_rasterize / grid_interp (:175-194, :83-106), in its fp32 arithmetic:
//   ind0 = floor(p / cubesize), ind1 = fmod(ceil(p / cubesize), size)
//   weight of node ind0 = |p - (ind0 + 1) * cubesize| / cubesize, of node ind1 = |p - ind0 * cubesize| / cubesize
struct Axis { int i0, i1; float w0, w1; };
__device__ __forceinline__ Axis axis_of(float p, float cs, float rf)
{
	Axis a;
	const float q = p / cs;
	const float f0 = floorf(q);
	a.i0 = (int)f0;
	a.i1 = (int)fmodf(ceilf(q), rf);
	const float x0 = f0 * cs, x1 = (f0 + 1.0f) * cs;
	a.w0 = fabsf(p - x1) / cs;
	a.w1 = fabsf(p - x0) / cs;
	return a;
}
// a coordinate the reference can index with: finite, in [0, 1), and floor(p / cubesize) < size after the fp32 division
__device__ __forceinline__ bool axis_ok(float p, float cs, int r) { return p >= 0.0f && p < 1.0f && (int)floorf(p / cs) < r; }

// ------------------------------------------------------------------------------------------------------ rasterize
__global__ void __launch_bounds__(256) psr_keys(const float* __restrict__ pts, int n, Res R, int* __restrict__ keys,
                                                int* __restrict__ vals, int* __restrict__ cell_count, int* status)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
	int key = 0;
	if (axis_ok(x, R.cs[0], R.r[0]) && axis_ok(y, R.cs[1], R.r[1]) && axis_ok(z, R.cs[2], R.r[2])) {
		key = ((int)floorf(x / R.cs[0]) * R.r[1] + (int)floorf(y / R.cs[1])) * R.r[2] + (int)floorf(z / R.cs[2]);
		atomicAdd(&cell_count[key], 1);
	} else {
		atomicOr(status, 1);   // the point is left out of every cell; the call fails
	}
	keys[i] = key;
	vals[i] = i;
}

__global__ void __launch_bounds__(256) psr_permute(const float* __restrict__ pts, const float* __restrict__ vals, int n, int C,
                                                   const int* __restrict__ order, float* __restrict__ spts, float* __restrict__ svals)
{
	const int j = blockIdx.x * 256 + threadIdx.x;
	if (j >= n) return;
	const size_t i = (size_t)order[j];
	for (int d = 0; d < 3; d++) spts[3 * (size_t)j + d] = pts[3 * i + d];
	for (int c = 0; c < C; c++) svals[(size_t)C * j + c] = vals[(size_t)C * i + c];
}

// One lane per grid node: the (point, corner) pairs that land on node (n0, n1, n2) come from the cells {n - 1, n} per axis
// (wrapped).  Cells in the order (-1,-1,-1) ... (0,0,0), a cell's points in ascending original index (stable sort), a
// point's corners in ascending corner index: a fixed order.  A point that lies in an invalid cell never got a cell count,
// so it is not visited.
__global__ void __launch_bounds__(256) psr_node_gather(const float* __restrict__ spts, const float* __restrict__ svals, int C,
                                                       const int* __restrict__ cell_start, Res R, int weighted,
                                                       float* __restrict__ out, int* __restrict__ counts)
{
	const long long nn = (long long)R.r[0] * R.r[1] * R.r[2];
	const long long lin = (long long)blockIdx.x * 256 + threadIdx.x;
	if (lin >= nn) return;
	const int n2 = (int)(lin % R.r[2]), n1 = (int)((lin / R.r[2]) % R.r[1]), n0 = (int)(lin / ((long long)R.r[2] * R.r[1]));
	double acc[GSR_PSR_MAX_CHANNELS] = {0.0, 0.0, 0.0, 0.0};
	int cnt = 0;
	for (int d0 = -1; d0 <= 0; d0++) {
		const int c0 = n0 + d0 < 0 ? R.r[0] - 1 : n0 + d0;
		for (int d1 = -1; d1 <= 0; d1++) {
			const int c1 = n1 + d1 < 0 ? R.r[1] - 1 : n1 + d1;
			for (int d2 = -1; d2 <= 0; d2++) {
				const int c2 = n2 + d2 < 0 ? R.r[2] - 1 : n2 + d2;
				const int cell = (c0 * R.r[1] + c1) * R.r[2] + c2;
				const int b = cell_start[cell], e = cell_start[cell + 1];
				for (int j = b; j < e; j++) {
					const Axis ax = axis_of(spts[3 * (size_t)j], R.cs[0], R.rf[0]);
					const Axis ay = axis_of(spts[3 * (size_t)j + 1], R.cs[1], R.rf[1]);
					const Axis az = axis_of(spts[3 * (size_t)j + 2], R.cs[2], R.rf[2]);
					const int m0 = (ax.i0 == n0 ? 1 : 0) | (ax.i1 == n0 ? 2 : 0);
					const int m1 = (ay.i0 == n1 ? 1 : 0) | (ay.i1 == n1 ? 2 : 0);
					const int m2 = (az.i0 == n2 ? 1 : 0) | (az.i1 == n2 ? 2 : 0);
					if (!m0 || !m1 || !m2) continue;
					float v[GSR_PSR_MAX_CHANNELS] = {0.f, 0.f, 0.f, 0.f};
					for (int c = 0; c < GSR_PSR_MAX_CHANNELS; c++)
						if (c < C) v[c] = svals[(size_t)C * j + c];
					for (int k0 = 0; k0 < 2; k0++) {
						if (!((m0 >> k0) & 1)) continue;
						for (int k1 = 0; k1 < 2; k1++) {
							if (!((m1 >> k1) & 1)) continue;
							for (int k2 = 0; k2 < 2; k2++) {
								if (!((m2 >> k2) & 1)) continue;
								const float w = ((k0 ? ax.w1 : ax.w0) * (k1 ? ay.w1 : ay.w0)) * (k2 ? az.w1 : az.w0);
								cnt++;
								for (int c = 0; c < GSR_PSR_MAX_CHANNELS; c++) acc[c] += (double)(w * v[c]);
							}
						}
					}
				}
			}
		}
	}
	const float div = (float)(cnt == 0 ? 1 : cnt);
	for (int c = 0; c < GSR_PSR_MAX_CHANNELS; c++) {
		if (c >= C) break;
		const float s = (float)acc[c];
		out[(size_t)c * nn + lin] = weighted ? s / div : s;
	}
	if (counts) counts[lin] = cnt;
}

// ------------------------------------------------------------------------------------------------------ spectral solve
// np.fft.fftfreq(n, d = 1 / n): 0 .. ceil(n / 2) - 1, then -floor(n / 2) .. -1
__device__ __forceinline__ int fft_freq(int i, int n) { return i < (n + 1) / 2 ? i : i - n; }

// DPSR.forward :305-316 per element of the half spectrum [R0, R1, R2 / 2 + 1]; spec holds the three planes of rfftn(N).
__global__ void __launch_bounds__(256) psr_spectral(const float2* __restrict__ spec, int r0, int r1, int r2h, double sig,
                                                    float2* __restrict__ phi)
{
	const long long ne = (long long)r0 * r1 * r2h;
	const float pi = (float)M_PI;
	for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < ne; e += (long long)gridDim.x * 256) {
		const int k = (int)(e % r2h), j = (int)((e / r2h) % r1), i = (int)(e / ((long long)r2h * r1));
		const int f[3] = {fft_freq(i, r0), fft_freq(j, r1), k};
		// spec_gaussian_filter :44-50, fp64 from the integer frequencies, cast to fp32
		const double dis = sqrt((double)f[0] * f[0] + (double)f[1] * f[1] + (double)f[2] * f[2]);
		const double t = (sig * 2.0) * dis / (double)r0;
		const float g = (float)exp(-0.5 * (t * t));
		float dr = 0.f, di = 0.f, lap = 0.f;
		for (int d = 0; d < 3; d++) {
			const float2 n = spec[(size_t)d * ne + e];
			const float om = ((float)f[d] * 2.0f) * pi;
			const float nr = n.x * g, ni = n.y * g;
			const float tr = ni * om, ti = (-nr) * om;
			const float o2 = om * om;
			if (d == 0) { dr = tr; di = ti; lap = o2; }
			else { dr = dr + tr; di = di + ti; lap = lap + o2; }
		}
		const float den = (-lap) + 1e-6f;
		float2 o;
		o.x = dr / den;
		o.y = di / den;
		if (e == 0) { o.x = 0.f; o.y = 0.f; }
		phi[e] = o;
	}
}

// ------------------------------------------------------------------------------------------------------ interp + normalize
__device__ __forceinline__ double block_sum_256(double v, double* red)
{
	red[threadIdx.x] = v;
	__syncthreads();
	for (int w = 128; w > 0; w >>= 1) {
		if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
		__syncthreads();
	}
	const double r = red[0];
	__syncthreads();
	return r;
}

__global__ void __launch_bounds__(256) psr_interp(const float* __restrict__ grid, Res R, const float* __restrict__ pts, int n,
                                                  float* __restrict__ out, double* __restrict__ partial, int* status)
{
	__shared__ double red[256];
	const int i = blockIdx.x * 256 + threadIdx.x;
	float fv = 0.f;
	if (i < n) {
		const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
		if (axis_ok(x, R.cs[0], R.r[0]) && axis_ok(y, R.cs[1], R.r[1]) && axis_ok(z, R.cs[2], R.r[2])) {
			const Axis ax = axis_of(x, R.cs[0], R.rf[0]), ay = axis_of(y, R.cs[1], R.rf[1]), az = axis_of(z, R.cs[2], R.rf[2]);
			double acc = 0.0;
			for (int c = 0; c < 8; c++) {   // corner c = (k0, k1, k2), k0 slowest: torch.meshgrid order of the reference
				const int k0 = c >> 2, k1 = (c >> 1) & 1, k2 = c & 1;
				const int node = ((k0 ? ax.i1 : ax.i0) * R.r[1] + (k1 ? ay.i1 : ay.i0)) * R.r[2] + (k2 ? az.i1 : az.i0);
				const float w = ((k0 ? ax.w1 : ax.w0) * (k1 ? ay.w1 : ay.w0)) * (k2 ? az.w1 : az.w0);
				acc += (double)(grid[node] * w);
			}
			fv = (float)acc;
		} else {
			atomicOr(status, 1);
		}
		out[i] = fv;
	}
	const double s = block_sum_256((double)fv, red);
	if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// mean[0] = (sum of the block partials in a fixed order) / n
__global__ void __launch_bounds__(256) psr_mean(const double* __restrict__ partial, int np, int n, double* __restrict__ mean)
{
	__shared__ double red[256];
	double s = 0.0;
	for (int b = threadIdx.x; b < np; b += 256) s += partial[b];
	const double t = block_sum_256(s, red);
	if (threadIdx.x == 0) mean[0] = t / (double)n;
}

// params = {offset, |phi[0,0,0] - offset|}: read before the stream below may overwrite grid[0] in place
__global__ void psr_norm_params(const float* __restrict__ in, const double* __restrict__ mean, float* __restrict__ params)
{
	const float off = mean ? (float)mean[0] : 0.0f;
	params[0] = off;
	params[1] = fabsf(mean ? in[0] - off : in[0]);
}

__device__ __forceinline__ float psr_norm_one(float v, float off, float a, int shift, int scale, int do_tanh)
{
	if (shift) v = v - off;
	if (scale) v = (-v) / a * 0.5f;
	if (do_tanh) v = tanhf(v);
	return v;
}
// DPSR.forward :323-332 and the tanh of ShapeAsPoints.generate_mesh in one stream; nvec float4 then the scalar tail
__global__ void __launch_bounds__(256) psr_normalize(const float* in, float* out, long long n, long long nvec,
                                                     const float* __restrict__ params, int shift, int scale, int do_tanh)
{
	const float off = params[0], a = params[1];
	const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
	const float4* in4 = reinterpret_cast<const float4*>(in);
	float4* out4 = reinterpret_cast<float4*>(out);
	for (long long i = t0; i < nvec; i += step) {
		float4 v = in4[i];
		v.x = psr_norm_one(v.x, off, a, shift, scale, do_tanh);
		v.y = psr_norm_one(v.y, off, a, shift, scale, do_tanh);
		v.z = psr_norm_one(v.z, off, a, shift, scale, do_tanh);
		v.w = psr_norm_one(v.w, off, a, shift, scale, do_tanh);
		out4[i] = v;
	}
	for (long long i = 4 * nvec + t0; i < n; i += step) out[i] = psr_norm_one(in[i], off, a, shift, scale, do_tanh);
}

// ------------------------------------------------------------------------------------------------------ marching cubes
// tables and cube geometry (corner offsets along axis 0, 1, 2; per cube edge the corner that owns it -- its lower end -- and its
// axis): gsr_mc_tables.h, the ones the block volumes use.  The kernels are this file's own: one lane per node of a dense grid.
// per node: info = cube case (cube with this node as its lower corner; 0 on the upper faces of the grid) | edge flags << 8
// (bit a: the edge from this node along axis a crosses the level), and the two counts the scans run over
__global__ void __launch_bounds__(256) psr_mc_classify(const float* __restrict__ g, int r0, int r1, int r2, float level,
                                                       uint32_t* __restrict__ info, int* __restrict__ nvc, int* __restrict__ ntc)
{
	const long long nn = (long long)r0 * r1 * r2;
	const long long lin = (long long)blockIdx.x * 256 + threadIdx.x;
	if (lin >= nn) return;
	const int k = (int)(lin % r2), j = (int)((lin / r2) % r1), i = (int)(lin / ((long long)r2 * r1));
	const long long st[3] = {(long long)r1 * r2, r2, 1};
	const bool in0 = g[lin] < level;
	const bool has[3] = {i + 1 < r0, j + 1 < r1, k + 1 < r2};
	uint32_t fl = 0;
	for (int a = 0; a < 3; a++)
		if (has[a] && ((g[lin + st[a]] < level) != in0)) fl |= 1u << a;
	uint32_t cs = 0;
	if (has[0] && has[1] && has[2]) {
		for (int c = 0; c < 8; c++)
			if (g[lin + gsr_mc_corner[c][0] * st[0] + gsr_mc_corner[c][1] * st[1] + gsr_mc_corner[c][2] * st[2]] < level) cs |= 1u << c;
	}
	info[lin] = cs | (fl << 8);
	nvc[lin] = __popc(fl);
	ntc[lin] = gsr_mc_ntris[cs];
}

__global__ void __launch_bounds__(256) psr_mc_vertices(const float* __restrict__ g, int r0, int r1, int r2, float level,
                                                       const uint32_t* __restrict__ info, const int* __restrict__ voff,
                                                       float* __restrict__ verts)
{
	const long long nn = (long long)r0 * r1 * r2;
	const long long lin = (long long)blockIdx.x * 256 + threadIdx.x;
	if (lin >= nn) return;
	const uint32_t fl = info[lin] >> 8;
	if (!fl) return;
	const int k = (int)(lin % r2), j = (int)((lin / r2) % r1), i = (int)(lin / ((long long)r2 * r1));
	const long long st[3] = {(long long)r1 * r2, r2, 1};
	const float a0 = g[lin];
	size_t v = (size_t)voff[lin];
	for (int a = 0; a < 3; a++) {
		if (!((fl >> a) & 1)) continue;
		const float b0 = g[lin + st[a]];
		float p[3] = {(float)i, (float)j, (float)k};
		p[a] = p[a] + (level - a0) / (b0 - a0);
		verts[3 * v] = p[0]; verts[3 * v + 1] = p[1]; verts[3 * v + 2] = p[2];
		v++;
	}
}

__global__ void __launch_bounds__(256) psr_mc_triangles(int r0, int r1, int r2, const uint32_t* __restrict__ info,
                                                        const int* __restrict__ voff, const int* __restrict__ toff,
                                                        int* __restrict__ faces)
{
	const long long nn = (long long)r0 * r1 * r2;
	const long long lin = (long long)blockIdx.x * 256 + threadIdx.x;
	if (lin >= nn) return;
	const uint32_t cs = info[lin] & 255u;
	const int nt = gsr_mc_ntris[cs];
	if (!nt) return;
	const long long st[3] = {(long long)r1 * r2, r2, 1};
	size_t t = (size_t)toff[lin];
	for (int q = 0; q < nt; q++, t++) {
		for (int c = 0; c < 3; c++) {
			const int e = gsr_mc_tris[cs][3 * q + c];
			const int o = gsr_mc_edge_owner[e], ax = gsr_mc_edge_axis[e];
			const long long ol = lin + gsr_mc_corner[o][0] * st[0] + gsr_mc_corner[o][1] * st[1] + gsr_mc_corner[o][2] * st[2];
			const uint32_t fl = info[ol] >> 8;
			faces[3 * t + c] = voff[ol] + __popc(fl & ((1u << ax) - 1u));
		}
	}
}

// The edge end's central difference along one axis (spacing 1, index units); one-sided on the two faces of the grid
__device__ __forceinline__ float psr_node_diff(const float* __restrict__ g, long long lin, int idx, int r, long long st)
{
	if (idx == 0) return g[lin + st] - g[lin];
	if (idx == r - 1) return g[lin] - g[lin - st];
	return (g[lin + st] - g[lin - st]) * 0.5f;
}

// Vertex normals in the order of psr_mc_vertices: the grid's gradient at the two ends of the crossing edge, interpolated with
// the vertex's own t (fp32, ga + t * (gb - ga)), divided by max(|n|, 1e-6).
__global__ void __launch_bounds__(256) psr_mc_normals(const float* __restrict__ g, int r0, int r1, int r2, float level,
                                                      const uint32_t* __restrict__ info, const int* __restrict__ voff,
                                                      float* __restrict__ normals)
{
	const long long nn = (long long)r0 * r1 * r2;
	const long long lin = (long long)blockIdx.x * 256 + threadIdx.x;
	if (lin >= nn) return;
	const uint32_t fl = info[lin] >> 8;
	if (!fl) return;
	const int idx[3] = {(int)(lin / ((long long)r2 * r1)), (int)((lin / r2) % r1), (int)(lin % r2)};
	const int r[3] = {r0, r1, r2};
	const long long st[3] = {(long long)r1 * r2, r2, 1};
	const float a0 = g[lin];
	float ga[3];
	for (int d = 0; d < 3; d++) ga[d] = psr_node_diff(g, lin, idx[d], r[d], st[d]);
	size_t v = (size_t)voff[lin];
	for (int a = 0; a < 3; a++) {
		if (!((fl >> a) & 1)) continue;
		const long long lb = lin + st[a];      // the edge flag says idx[a] + 1 < r[a]
		const float t = (level - a0) / (g[lb] - a0);
		float n[3];
		for (int d = 0; d < 3; d++) {
			const float gb = psr_node_diff(g, lb, idx[d] + (d == a ? 1 : 0), r[d], st[d]);
			n[d] = ga[d] + t * (gb - ga[d]);
		}
		const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
		const float den = len > 1e-6f ? len : 1e-6f;
		normals[3 * v] = n[0] / den; normals[3 * v + 1] = n[1] / den; normals[3 * v + 2] = n[2] / den;
		v++;
	}
}

// ------------------------------------------------------------------------------------------------------ backward
// What torch autograd gives the reference for one axis: a factor |p - pos| / cs differentiates to sign(p - pos) / cs with
// sign(0) = 0; floor and ceil contribute nothing.  d0 goes with node i0 (pos = x1), d1 with node i1 (pos = x0).
struct AxisD { float d0, d1; };
__device__ __forceinline__ float psr_sign(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }
__device__ __forceinline__ AxisD axis_deriv(float p, float cs)
{
	AxisD a;
	const float f0 = floorf(p / cs);
	const float x0 = f0 * cs, x1 = (f0 + 1.0f) * cs;
	a.d0 = psr_sign(p - x1) / cs;
	a.d1 = psr_sign(p - x0) / cs;
	return a;
}

// One lane per point, the 8 corners in the order of psr_interp (k0 slowest).  g' = g[c, node] (/ (float)max(cnt, 1) when
// weighted), all fp32: grad_values[n, c] = sum_k (double)(w_k g'), grad_points[n, d] = sum_c sum_k (double)((dw_kd g') v_c),
// dw_kd the corner weight with the factor of axis d replaced by its derivative.  Each sum in fp64, rounded once.
__global__ void __launch_bounds__(256) psr_rasterize_bwd(const float* __restrict__ gg, const float* __restrict__ pts,
                                                         const float* __restrict__ vals, int n, int C, Res R, int weighted,
                                                         const int* __restrict__ counts, float* __restrict__ gvals,
                                                         float* __restrict__ gpts, int* status)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
	if (!(axis_ok(x, R.cs[0], R.r[0]) && axis_ok(y, R.cs[1], R.r[1]) && axis_ok(z, R.cs[2], R.r[2]))) {
		atomicOr(status, 1);
		return;
	}
	const size_t nn = (size_t)R.r[0] * R.r[1] * R.r[2];
	const Axis ax = axis_of(x, R.cs[0], R.rf[0]), ay = axis_of(y, R.cs[1], R.rf[1]), az = axis_of(z, R.cs[2], R.rf[2]);
	const AxisD dx = axis_deriv(x, R.cs[0]), dy = axis_deriv(y, R.cs[1]), dz = axis_deriv(z, R.cs[2]);
	float v[GSR_PSR_MAX_CHANNELS] = {0.f, 0.f, 0.f, 0.f};
	for (int c = 0; c < GSR_PSR_MAX_CHANNELS; c++)
		if (c < C) v[c] = vals[(size_t)C * i + c];
	double av[GSR_PSR_MAX_CHANNELS] = {0.0, 0.0, 0.0, 0.0};
	double ap[3] = {0.0, 0.0, 0.0};
	for (int c = 0; c < GSR_PSR_MAX_CHANNELS; c++) {
		if (c >= C) break;
		for (int k = 0; k < 8; k++) {
			const int k0 = k >> 2, k1 = (k >> 1) & 1, k2 = k & 1;
			const size_t node = ((size_t)(k0 ? ax.i1 : ax.i0) * R.r[1] + (k1 ? ay.i1 : ay.i0)) * R.r[2] + (k2 ? az.i1 : az.i0);
			float g = gg[c * nn + node];
			if (weighted) {
				const int cnt = counts[node];
				g = g / (float)(cnt == 0 ? 1 : cnt);
			}
			const float wx = k0 ? ax.w1 : ax.w0, wy = k1 ? ay.w1 : ay.w0, wz = k2 ? az.w1 : az.w0;
			const float sx = k0 ? dx.d1 : dx.d0, sy = k1 ? dy.d1 : dy.d0, sz = k2 ? dz.d1 : dz.d0;
			av[c] += (double)(((wx * wy) * wz) * g);
			ap[0] += (double)((((sx * wy) * wz) * g) * v[c]);
			ap[1] += (double)((((wx * sy) * wz) * g) * v[c]);
			ap[2] += (double)((((wx * wy) * sz) * g) * v[c]);
		}
	}
	if (gvals)
		for (int c = 0; c < GSR_PSR_MAX_CHANNELS; c++)
			if (c < C) gvals[(size_t)C * i + c] = (float)av[c];
	if (gpts)
		for (int d = 0; d < 3; d++) gpts[3 * (size_t)i + d] = (float)ap[d];
}

// grad_points[n, d] = sum_k (double)((grid[node_k] dw_kd) grad_out[n]), fp64, rounded once
__global__ void __launch_bounds__(256) psr_interp_bwd(const float* __restrict__ grid, Res R, const float* __restrict__ pts, int n,
                                                      const float* __restrict__ gout, float* __restrict__ gpts, int* status)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
	if (!(axis_ok(x, R.cs[0], R.r[0]) && axis_ok(y, R.cs[1], R.r[1]) && axis_ok(z, R.cs[2], R.r[2]))) {
		atomicOr(status, 1);
		return;
	}
	const Axis ax = axis_of(x, R.cs[0], R.rf[0]), ay = axis_of(y, R.cs[1], R.rf[1]), az = axis_of(z, R.cs[2], R.rf[2]);
	const AxisD dx = axis_deriv(x, R.cs[0]), dy = axis_deriv(y, R.cs[1]), dz = axis_deriv(z, R.cs[2]);
	const float go = gout[i];
	double ap[3] = {0.0, 0.0, 0.0};
	for (int k = 0; k < 8; k++) {
		const int k0 = k >> 2, k1 = (k >> 1) & 1, k2 = k & 1;
		const size_t node = ((size_t)(k0 ? ax.i1 : ax.i0) * R.r[1] + (k1 ? ay.i1 : ay.i0)) * R.r[2] + (k2 ? az.i1 : az.i0);
		const float lat = grid[node];
		const float wx = k0 ? ax.w1 : ax.w0, wy = k1 ? ay.w1 : ay.w0, wz = k2 ? az.w1 : az.w0;
		const float sx = k0 ? dx.d1 : dx.d0, sy = k1 ? dy.d1 : dy.d0, sz = k2 ? dz.d1 : dz.d0;
		ap[0] += (double)((lat * ((sx * wy) * wz)) * go);
		ap[1] += (double)((lat * ((wx * sy) * wz)) * go);
		ap[2] += (double)((lat * ((wx * wy) * sz)) * go);
	}
	for (int d = 0; d < 3; d++) gpts[3 * (size_t)i + d] = (float)ap[d];
}

// The adjoint of psr_spectral in PyTorch's convention for complex gradients: grad_N_d = conj(c_d) grad_Phi with
// c_d = -i w_d G / (Lap + 1e-6), i.e. (w_d G / den) (-Im, Re) of grad_Phi; element 0 (Phi[0,0,0] = 0) gets nothing.
// fp32 chain: a = grad_Phi / den, then (-a.y w_d, a.x w_d), then times G (fp64 filter, cast, as in the forward).
__global__ void __launch_bounds__(256) psr_spectral_bwd(const float2* __restrict__ gphi, int r0, int r1, int r2h, double sig,
                                                        float2* __restrict__ gspec)
{
	const long long ne = (long long)r0 * r1 * r2h;
	const float pi = (float)M_PI;
	for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < ne; e += (long long)gridDim.x * 256) {
		const int k = (int)(e % r2h), j = (int)((e / r2h) % r1), i = (int)(e / ((long long)r2h * r1));
		const int f[3] = {fft_freq(i, r0), fft_freq(j, r1), k};
		const double dis = sqrt((double)f[0] * f[0] + (double)f[1] * f[1] + (double)f[2] * f[2]);
		const double t = (sig * 2.0) * dis / (double)r0;
		const float g = (float)exp(-0.5 * (t * t));
		float om[3], lap = 0.f;
		for (int d = 0; d < 3; d++) {
			om[d] = ((float)f[d] * 2.0f) * pi;
			const float o2 = om[d] * om[d];
			lap = d == 0 ? o2 : lap + o2;
		}
		const float den = (-lap) + 1e-6f;
		const float2 gp = gphi[e];
		const float ar = gp.x / den, ai = gp.y / den;
		for (int d = 0; d < 3; d++) {
			float2 o;
			o.x = ((-ai) * om[d]) * g;
			o.y = (ar * om[d]) * g;
			if (e == 0) { o.x = 0.f; o.y = 0.f; }
			gspec[(size_t)d * ne + e] = o;
		}
	}
}

__device__ __forceinline__ float psr_norm_bwd_one(float go, float o, float a, int scale, int do_tanh)
{
	if (do_tanh) go = go * (1.0f - o * o);
	if (scale) go = (-go) / a * 0.5f;
	return go;
}
// grad_in = grad_out (1 - out^2) [tanh] (-0.5 / |v0|) [scale], |v0| = params[1] a constant; every lane adds its own values
// in fp64 in loop order, a block its lanes in the fixed tree: partial[blockIdx.x]
__global__ void __launch_bounds__(256) psr_normalize_bwd(const float* gout, const float* out, float* gin, long long n, long long nvec,
                                                         const float* __restrict__ params, int scale, int do_tanh,
                                                         double* __restrict__ partial)
{
	__shared__ double red[256];
	const float a = params[1];
	const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
	const float4* go4 = reinterpret_cast<const float4*>(gout);
	const float4* o4 = reinterpret_cast<const float4*>(out);
	float4* gi4 = reinterpret_cast<float4*>(gin);
	double acc = 0.0;
	for (long long i = t0; i < nvec; i += step) {
		float4 v = go4[i];
		const float4 o = do_tanh ? o4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
		v.x = psr_norm_bwd_one(v.x, o.x, a, scale, do_tanh);
		v.y = psr_norm_bwd_one(v.y, o.y, a, scale, do_tanh);
		v.z = psr_norm_bwd_one(v.z, o.z, a, scale, do_tanh);
		v.w = psr_norm_bwd_one(v.w, o.w, a, scale, do_tanh);
		gi4[i] = v;
		acc += (double)v.x; acc += (double)v.y; acc += (double)v.z; acc += (double)v.w;
	}
	for (long long i = 4 * nvec + t0; i < n; i += step) {
		const float v = psr_norm_bwd_one(gout[i], do_tanh ? out[i] : 0.f, a, scale, do_tanh);
		gin[i] = v;
		acc += (double)v;
	}
	const double s = block_sum_256(acc, red);
	if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// grad_mean[0] = -(sum of the block partials in a fixed order): the shift subtracts the mean from every value
__global__ void __launch_bounds__(256) psr_neg_sum(const double* __restrict__ partial, int np, double* __restrict__ gmean)
{
	__shared__ double red[256];
	double s = 0.0;
	for (int b = threadIdx.x; b < np; b += 256) s += partial[b];
	const double t = block_sum_256(s, red);
	if (threadIdx.x == 0) gmean[0] = -t;
}

}  // namespace

extern "C" {

int gsr_psr_rasterize(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* points, int num_points, const float* values,
                      int channels, int r0, int r1, int r2, int weighted, float* grid, int* counts, void* stream)
{
	if (!grid || !good_res(r0, r1, r2) || channels < 1 || channels > GSR_PSR_MAX_CHANNELS || num_points < 0 ||
	    num_points > (1 << 28) || (num_points > 0 && (!points || !values)))
		return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const int n = num_points, C = channels;
	const long long nn = (long long)r0 * r1 * r2;
	const Res R = make_res(r0, r1, r2);
	int *k0, *v0, *cell_count, *cell_start, *status;
	SortBufs<int> sb;   // sb.part serves the scan of the cell counts too
	float *spts, *svals;
	auto carve = [&](Arena& ws) {
		k0 = ws.take<int>(n); v0 = ws.take<int>(n); sb = sort_take<int>(ws, n, nn);
		cell_count = ws.take<int>(nn); cell_start = ws.take<int>(nn + 1);
		spts = ws.take<float>((size_t)n * 3); svals = ws.take<float>((size_t)n * C);
		status = ws.take<int>(1);
	};
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;

	GSR_TRY(hipMemsetAsync(cell_count, 0, (size_t)nn * 4, s));
	GSR_TRY(hipMemsetAsync(status, 0, 4, s));
	if (n > 0) hipLaunchKernelGGL(psr_keys, dim3(blocks(n)), dim3(256), 0, s, points, n, R, k0, v0, cell_count, status);
	int rc = exclusive_scan(cell_count, (int)nn, cell_start, sb.part, s);
	if (rc) return rc;
	if (n > 0) {
		rc = radix_sort(k0, v0, n, bits_for(nn), sb, s);
		if (rc) return rc;
		hipLaunchKernelGGL(psr_permute, dim3(blocks(n)), dim3(256), 0, s, points, values, n, C, v0, spts, svals);
	}
	rc = read_status(status, s);
	if (rc) return rc;
	// a valid cloud: every point has a cell count, cell_start[nn] == n, every sorted slot below it holds a valid point
	hipLaunchKernelGGL(psr_node_gather, dim3(blocks(nn)), dim3(256), 0, s, spts, svals, C, cell_start, R, weighted, grid, counts);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_psr_spectral(const float* spectrum, int r0, int r1, int r2, double sig, float* phi, void* stream)
{
	if (!spectrum || !phi || !good_res(r0, r1, r2)) return GSR_ERR_ARG;
	const long long ne = (long long)r0 * r1 * (r2 / 2 + 1);
	hipLaunchKernelGGL(psr_spectral, dim3(stream_blocks(ne)), dim3(256), 0, (hipStream_t)stream,
	                   reinterpret_cast<const float2*>(spectrum), r0, r1, r2 / 2 + 1, sig, reinterpret_cast<float2*>(phi));
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_psr_interp(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* grid, int r0, int r1, int r2, const float* points,
                   int num_points, float* samples, double* mean, void* stream)
{
	if (!grid || !good_res(r0, r1, r2) || !points || num_points < 1 || !samples) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const int n = num_points, np = (int)blocks(n);
	double *partial, *m;
	int* status;
	auto carve = [&](Arena& ws) {
		partial = ws.take<double>(np);
		m = ws.take<double>(1);
		status = ws.take<int>(1);
	};
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;
	GSR_TRY(hipMemsetAsync(status, 0, 4, s));
	hipLaunchKernelGGL(psr_interp, dim3(np), dim3(256), 0, s, grid, make_res(r0, r1, r2), points, n, samples, partial, status);
	hipLaunchKernelGGL(psr_mean, dim3(1), dim3(256), 0, s, partial, np, n, mean ? mean : m);
	const int rc = read_status(status, s);
	if (rc) return rc;
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_psr_normalize(const float* grid_in, float* grid_out, long long count, const double* mean, int scale, int apply_tanh,
                      float* params, void* stream)
{
	if (!grid_in || !grid_out || count < 1 || !params) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	hipLaunchKernelGGL(psr_norm_params, dim3(1), dim3(1), 0, s, grid_in, mean, params);
	const bool aligned = (((uintptr_t)grid_in | (uintptr_t)grid_out) & 15) == 0;
	const long long nvec = aligned ? count / 4 : 0;
	hipLaunchKernelGGL(psr_normalize, dim3(stream_blocks(count / 4 + 1)), dim3(256), 0, s, grid_in, grid_out, count, nvec, params,
	                   mean ? 1 : 0, scale, apply_tanh);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_psr_mc_classify(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* grid, int r0, int r1, int r2, float level,
                        uint32_t* node_info, int* vertex_offset, int* triangle_offset, int* num_vertices, int* num_triangles,
                        void* stream)
{
	if (!grid || !good_res(r0, r1, r2) || !node_info || !vertex_offset || !triangle_offset || !num_vertices || !num_triangles)
		return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const long long nn = (long long)r0 * r1 * r2;
	int *nvc, *ntc, *part;
	auto carve = [&](Arena& ws) { nvc = ws.take<int>(nn); ntc = ws.take<int>(nn); part = ws.take<int>(scan_part_len(nn)); };
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;
	hipLaunchKernelGGL(psr_mc_classify, dim3(blocks(nn)), dim3(256), 0, s, grid, r0, r1, r2, level, node_info, nvc, ntc);
	int rc = exclusive_scan(nvc, (int)nn, vertex_offset, part, s);
	if (rc) return rc;
	rc = exclusive_scan(ntc, (int)nn, triangle_offset, part, s);
	if (rc) return rc;
	GSR_TRY(hipMemcpyAsync(num_vertices, vertex_offset + nn, sizeof(int), hipMemcpyDeviceToHost, s));
	GSR_TRY(hipMemcpyAsync(num_triangles, triangle_offset + nn, sizeof(int), hipMemcpyDeviceToHost, s));
	GSR_TRY(hipStreamSynchronize(s));
	return GSR_OK;
}

int gsr_psr_mc_emit(const float* grid, int r0, int r1, int r2, float level, const uint32_t* node_info, const int* vertex_offset,
                    const int* triangle_offset, float* vertices, int* faces, void* stream)
{
	if (!grid || !good_res(r0, r1, r2) || !node_info || !vertex_offset || !triangle_offset) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const long long nn = (long long)r0 * r1 * r2;
	if (vertices) hipLaunchKernelGGL(psr_mc_vertices, dim3(blocks(nn)), dim3(256), 0, s, grid, r0, r1, r2, level, node_info, vertex_offset, vertices);
	if (faces) hipLaunchKernelGGL(psr_mc_triangles, dim3(blocks(nn)), dim3(256), 0, s, r0, r1, r2, node_info, vertex_offset, triangle_offset, faces);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_psr_mc_normals(const float* grid, int r0, int r1, int r2, float level, const uint32_t* node_info, const int* vertex_offset,
                       float* normals, void* stream)
{
	if (!grid || !good_res(r0, r1, r2) || !node_info || !vertex_offset || !normals) return GSR_ERR_ARG;
	const long long nn = (long long)r0 * r1 * r2;
	hipLaunchKernelGGL(psr_mc_normals, dim3(blocks(nn)), dim3(256), 0, (hipStream_t)stream, grid, r0, r1, r2, level, node_info,
	                   vertex_offset, normals);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_psr_rasterize_bwd(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* grad_grid, const float* points,
                          int num_points, const float* values, int channels, int r0, int r1, int r2, int weighted,
                          const int* counts, float* grad_values, float* grad_points, void* stream)
{
	if (!grad_grid || !good_res(r0, r1, r2) || channels < 1 || channels > GSR_PSR_MAX_CHANNELS || num_points < 0 ||
	    num_points > (1 << 28) || (num_points > 0 && (!points || !values)) || (weighted && !counts))
		return GSR_ERR_ARG;
	if (num_points == 0 || (!grad_values && !grad_points)) return GSR_OK;
	hipStream_t s = (hipStream_t)stream;
	int* status;
	auto carve = [&](Arena& ws) { status = ws.take<int>(1); };
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;
	GSR_TRY(hipMemsetAsync(status, 0, 4, s));
	hipLaunchKernelGGL(psr_rasterize_bwd, dim3(blocks(num_points)), dim3(256), 0, s, grad_grid, points, values, num_points, channels,
	                   make_res(r0, r1, r2), weighted, counts, grad_values, grad_points, status);
	const int rc = read_status(status, s);
	if (rc) return rc;
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_psr_interp_bwd(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* grid, int r0, int r1, int r2,
                       const float* points, int num_points, const float* grad_samples, float* grad_points, void* stream)
{
	if (!grid || !good_res(r0, r1, r2) || !points || num_points < 1 || !grad_samples || !grad_points) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	int* status;
	auto carve = [&](Arena& ws) { status = ws.take<int>(1); };
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;
	GSR_TRY(hipMemsetAsync(status, 0, 4, s));
	hipLaunchKernelGGL(psr_interp_bwd, dim3(blocks(num_points)), dim3(256), 0, s, grid, make_res(r0, r1, r2), points, num_points,
	                   grad_samples, grad_points, status);
	const int rc = read_status(status, s);
	if (rc) return rc;
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_psr_spectral_bwd(const float* grad_phi, int r0, int r1, int r2, double sig, float* grad_spectrum, void* stream)
{
	if (!grad_phi || !grad_spectrum || !good_res(r0, r1, r2)) return GSR_ERR_ARG;
	const long long ne = (long long)r0 * r1 * (r2 / 2 + 1);
	hipLaunchKernelGGL(psr_spectral_bwd, dim3(stream_blocks(ne)), dim3(256), 0, (hipStream_t)stream,
	                   reinterpret_cast<const float2*>(grad_phi), r0, r1, r2 / 2 + 1, sig, reinterpret_cast<float2*>(grad_spectrum));
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_psr_normalize_bwd(gsr_alloc_fn workspace_alloc, void* workspace_ctx, const float* grad_out, const float* grid_out,
                          long long count, const float* params, int scale, int apply_tanh, float* grad_in, double* grad_mean,
                          void* stream)
{
	if (!grad_out || !grad_in || count < 1 || !params || (apply_tanh && !grid_out)) return GSR_ERR_ARG;
	hipStream_t s = (hipStream_t)stream;
	const unsigned nb = stream_blocks(count / 4 + 1);
	double *partial, *m;
	auto carve = [&](Arena& ws) { partial = ws.take<double>(nb); m = ws.take<double>(1); };
	if (!ws_carve(workspace_alloc, workspace_ctx, carve)) return GSR_ERR_ALLOC;
	const bool aligned = (((uintptr_t)grad_out | (uintptr_t)grad_in | (uintptr_t)grid_out) & 15) == 0;
	const long long nvec = aligned ? count / 4 : 0;
	hipLaunchKernelGGL(psr_normalize_bwd, dim3(nb), dim3(256), 0, s, grad_out, grid_out, grad_in, count, nvec, params, scale,
	                   apply_tanh, partial);
	hipLaunchKernelGGL(psr_neg_sum, dim3(1), dim3(256), 0, s, partial, (int)nb, grad_mean ? grad_mean : m);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

}  // extern "C"
