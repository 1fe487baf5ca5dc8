// gsr_optim.hip -- the optimiser half of 3DGS training: the Adam step over the six parameter groups of a Gaussian model
// (dense, or sparse in the rows a view saw), the statistics of adaptive density control, and clone / split / prune as one
// classify -> scan -> emit compaction that carries the Adam moments (its definition to the bit:
// tests/optim_model.py; design: DESIGN.md s22).
//
// adam_kernel: ONE launch for all groups.  A group of n floats is cut into 16-byte units counted from the 16-byte boundary at
// or below its first float (`shift` floats before it): a unit that lies inside the tensor is read and written as float4 per
// tensor, the first and the last unit element by element.  That needs parameter, gradient and both moments to sit at one
// offset within 16 bytes; a group where they do not takes the element path for every unit.  The units of all groups form one
// index space walked by a capped grid-stride loop.  Arithmetic per element, plain IEEE, nothing contracted:
//     m' = m + (g - m) c1;  v' = v + (g g - v) c2;  p' = p - s (m' / (sqrt(v') / b + eps))
// accumulate_kernel, classify_kernel: one lane per row.  emit_kernel: one lane per source WORD of every group; it writes the
// word to each output row of its source.  No atomics anywhere.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/gsrast.h"
#include "gsr_common.h"
#include "gsr_optim_plan.h"
#include "gsr_sort.h"
#include "gsr_ws.h"

namespace {

constexpr unsigned MAX_GRID = 2048;   // 256 CUs x 8 workgroups: the rest is the grid-stride loop

unsigned capped_grid(unsigned long long work)
{
	const unsigned long long b = (work + 255) / 256;
	return (unsigned)(b < MAX_GRID ? (b ? b : 1) : MAX_GRID);
}

// ------------------------------------------------------------------------------------------------------ Adam
struct AdamGroup {
	float* p;
	const float* g;
	float* m;
	float* v;
	unsigned n;       // floats
	unsigned w;       // floats per row
	unsigned shift;   // floats between the 16-byte boundary below p and p (0 on the element path)
	unsigned vec;     // 1: all four tensors share that offset
	float c1, c2, sqrt_bc2, step_size;
};
struct AdamArgs {
	AdamGroup g[6];
	unsigned ustart[7];   // first unit of each group, total at [ngroups]
	int ngroups;
	float eps;
};

__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float c1, float c2, float b, float s, float eps)
{
	m = m + (g - m) * c1;
	v = v + (g * g - v) * c2;
	const float den = sqrtf(v) / b + eps;
	p = p - s * (m / den);
}

__global__ __launch_bounds__(256) void adam_kernel(AdamArgs a, const int* __restrict__ radii)
{
	const unsigned total = a.ustart[a.ngroups], stride = gridDim.x * 256u;
	for (unsigned U = blockIdx.x * 256u + threadIdx.x; U < total; U += stride) {
		int gi = 0;
#pragma unroll
		for (int k = 1; k < 6; k++) gi += (k < a.ngroups && U >= a.ustart[k]) ? 1 : 0;
		const AdamGroup& G = a.g[gi];
		const unsigned u = U - a.ustart[gi];
		const int e0 = (int)(4u * u) - (int)G.shift;                    // -3 .. n - 1
		const unsigned n = G.n, w = G.w;
		const unsigned first = e0 < 0 ? 0u : (unsigned)e0;
		unsigned row = first / w, rem = first - row * w;
		bool vis[4];
		bool any = false;
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const int e = e0 + k;
			const bool valid = e >= 0 && (unsigned)e < n;
			bool s = valid;
			if (valid) {
				if (radii) s = radii[row] > 0;
				if (++rem == w) { rem = 0; row++; }
			}
			vis[k] = s;
			any |= s;
		}
		if (!any) continue;
		const bool full = G.vec && e0 >= 0 && (unsigned)e0 + 4u <= n;
		float P[4], Gr[4], M[4], V[4];
		if (full) {
			const float4 p4 = *reinterpret_cast<const float4*>(G.p + e0), g4 = *reinterpret_cast<const float4*>(G.g + e0);
			const float4 m4 = *reinterpret_cast<const float4*>(G.m + e0), v4 = *reinterpret_cast<const float4*>(G.v + e0);
			P[0] = p4.x; P[1] = p4.y; P[2] = p4.z; P[3] = p4.w;
			Gr[0] = g4.x; Gr[1] = g4.y; Gr[2] = g4.z; Gr[3] = g4.w;
			M[0] = m4.x; M[1] = m4.y; M[2] = m4.z; M[3] = m4.w;
			V[0] = v4.x; V[1] = v4.y; V[2] = v4.z; V[3] = v4.w;
		} else {
#pragma unroll
			for (int k = 0; k < 4; k++) {
				P[k] = Gr[k] = M[k] = V[k] = 0.f;
				if (vis[k]) { P[k] = G.p[e0 + k]; Gr[k] = G.g[e0 + k]; M[k] = G.m[e0 + k]; V[k] = G.v[e0 + k]; }
			}
		}
#pragma unroll
		for (int k = 0; k < 4; k++) {
			float p = P[k], m = M[k], v = V[k];
			adam_update(p, Gr[k], m, v, G.c1, G.c2, G.sqrt_bc2, G.step_size, a.eps);
			if (vis[k]) { P[k] = p; M[k] = m; V[k] = v; }          // an unseen element keeps the bits it was read with
		}
		if (full) {
			*reinterpret_cast<float4*>(G.p + e0) = make_float4(P[0], P[1], P[2], P[3]);
			*reinterpret_cast<float4*>(G.m + e0) = make_float4(M[0], M[1], M[2], M[3]);
			*reinterpret_cast<float4*>(G.v + e0) = make_float4(V[0], V[1], V[2], V[3]);
		} else {
#pragma unroll
			for (int k = 0; k < 4; k++)
				if (vis[k]) { G.p[e0 + k] = P[k]; G.m[e0 + k] = M[k]; G.v[e0 + k] = V[k]; }
		}
	}
}

// ------------------------------------------------------------------------------------------------------ statistics
__global__ __launch_bounds__(256) void accumulate_kernel(int n, const float* __restrict__ mg, const int* __restrict__ radii,
                                                         float* __restrict__ grad_accum, int* __restrict__ denom,
                                                         int* __restrict__ max_radii)
{
	const unsigned stride = gridDim.x * 256u;
	for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < (unsigned)n; i += stride) {
		const int r = radii[i];
		if (r <= 0) continue;
		const float gx = mg[3 * (size_t)i], gy = mg[3 * (size_t)i + 1];
		grad_accum[i] = grad_accum[i] + sqrtf(gx * gx + gy * gy);
		denom[i] = denom[i] + 1;
		const int mr = max_radii[i];
		max_radii[i] = mr > r ? mr : r;
	}
}

// ------------------------------------------------------------------------------------------------------ classify
struct ClassifyArgs {
	float max_grad, t_big, t_world, t_op, d_split;
	int max_screen_size;   // < 0: no screen- and world-size tests
};

// flag[i], flag[n + i], flag[2 n + i]: the source survives, its clone is emitted, its children are emitted
__global__ __launch_bounds__(256) void classify_kernel(int n, const float* __restrict__ scaling, const float* __restrict__ opacity,
                                                       const float* __restrict__ grad_accum, const int* __restrict__ denom,
                                                       const int* __restrict__ max_radii, const unsigned char* __restrict__ mask,
                                                       ClassifyArgs c, int* __restrict__ flag)
{
	const unsigned stride = gridDim.x * 256u;
	for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < (unsigned)n; i += stride) {
		int fa, fb = 0, fc = 0;
		if (mask) {
			fa = mask[i] ? 0 : 1;
		} else {
			const int d = denom[i];
			const float avg = d > 0 ? grad_accum[i] / (float)d : 0.f;
			const bool hot = avg >= c.max_grad;                        // false for a NaN
			float smax = scaling[3 * (size_t)i];
			const float s1 = scaling[3 * (size_t)i + 1], s2 = scaling[3 * (size_t)i + 2];
			if (s1 > smax) smax = s1;
			if (s2 > smax) smax = s2;
			const bool big = smax > c.t_big;
			const bool clone = hot && !big, split = hot && big;
			const bool tests = c.max_screen_size >= 0;
			const bool low = opacity[i] < c.t_op;
			const bool fail_self = low || (tests && (max_radii[i] > c.max_screen_size || smax > c.t_world));
			const bool fail_child = low || (tests && (smax - c.d_split) > c.t_world);
			fa = (!split && !fail_self) ? 1 : 0;
			fb = (clone && !fail_self) ? 1 : 0;
			fc = (split && !fail_child) ? 1 : 0;
		}
		flag[i] = fa;
		flag[(size_t)n + i] = fb;
		flag[2 * (size_t)n + i] = fc;
	}
}

__global__ void totals_kernel(const int* __restrict__ pos, int n, int* __restrict__ out3)
{
	if (threadIdx.x == 0 && blockIdx.x == 0) {
		out3[0] = pos[n];
		out3[1] = pos[2 * (size_t)n] - pos[n];
		out3[2] = pos[3 * (size_t)n] - pos[2 * (size_t)n];
	}
}

// ------------------------------------------------------------------------------------------------------ emit
struct EmitGroup {
	const uint32_t* src[3];
	uint32_t* dst[3];
	unsigned w;
	int kind;
};
struct EmitArgs {
	EmitGroup g[8];
	unsigned long long start[9];   // first word of each group in the walk, total at [ngroups]
	int ngroups;
	int n;
	int n_split;
	float d_split;
};

__device__ __forceinline__ float clamp80(float p) { return p < -80.f ? -80.f : (p > 80.f ? 80.f : p); }

// component `col` of R(q / |q|) (exp(scaling) * noise), plain IEEE in this order (the rotation of the published build_rotation)
__device__ __forceinline__ float child_offset(const float* __restrict__ q4, const float* __restrict__ s3, const float* __restrict__ z3,
                                              unsigned col)
{
	const float qw = q4[0], qx = q4[1], qy = q4[2], qz = q4[3];
	const float nn = ((qw * qw + qx * qx) + qy * qy) + qz * qz;
	const float nrm = sqrtf(nn);
	const float r = qw / nrm, x = qx / nrm, y = qy / nrm, z = qz / nrm;
	const float a0 = gs_exp(clamp80(s3[0])) * z3[0], a1 = gs_exp(clamp80(s3[1])) * z3[1], a2 = gs_exp(clamp80(s3[2])) * z3[2];
	float r0, r1, r2;
	if (col == 0) {
		r0 = 1.f - 2.f * (y * y + z * z); r1 = 2.f * (x * y - r * z); r2 = 2.f * (x * z + r * y);
	} else if (col == 1) {
		r0 = 2.f * (x * y + r * z); r1 = 1.f - 2.f * (x * x + z * z); r2 = 2.f * (y * z - r * x);
	} else {
		r0 = 2.f * (x * z - r * y); r1 = 2.f * (y * z + r * x); r2 = 1.f - 2.f * (x * x + y * y);
	}
	return (r0 * a0 + r1 * a1) + r2 * a2;
}

__global__ __launch_bounds__(256) void emit_kernel(EmitArgs a, const int* __restrict__ pos, const float* __restrict__ noise,
                                                   const float* __restrict__ scaling, const float* __restrict__ rotation)
{
	const unsigned long long total = a.start[a.ngroups], stride = (unsigned long long)gridDim.x * 256u;
	const size_t n = (size_t)a.n;
	const int n_c = pos[3 * n] - pos[2 * n];
	for (unsigned long long T = (unsigned long long)blockIdx.x * 256u + threadIdx.x; T < total; T += stride) {
		int gi = 0;
#pragma unroll
		for (int k = 1; k < 8; k++) gi += (k < a.ngroups && T >= a.start[k]) ? 1 : 0;
		const EmitGroup& G = a.g[gi];
		const unsigned e = (unsigned)(T - a.start[gi]), w = G.w;
		const unsigned i = e / w, col = e - i * w;
		const int a0 = pos[i], b0 = pos[n + i], c0 = pos[2 * n + i];
		const bool fa = pos[i + 1] != a0, fb = pos[n + i + 1] != b0, fc = pos[2 * n + i + 1] != c0;
		const bool stats = G.kind == GSR_COMPACT_STATS;
		if (!(fa || ((fb || fc) && !stats))) continue;
		const uint32_t val = G.src[0][e];
		if (fa) {
			const size_t d = (size_t)a0 * w + col;
			G.dst[0][d] = val;
			G.dst[1][d] = G.src[1][e];
			G.dst[2][d] = G.src[2][e];
		}
		if (stats) continue;
		if (fb) {
			const size_t d = (size_t)b0 * w + col;
			G.dst[0][d] = val;
			G.dst[1][d] = 0u;
			G.dst[2][d] = 0u;
		}
		if (fc) {
			for (int c = 0; c < a.n_split; c++) {
				uint32_t out = val;
				if (G.kind == GSR_COMPACT_XYZ)
					out = __float_as_uint(__uint_as_float(val) + child_offset(rotation + 4 * (size_t)i, scaling + 3 * (size_t)i,
					                                                          noise + ((size_t)i * a.n_split + c) * 3, col));
				else if (G.kind == GSR_COMPACT_SCALING)
					out = __float_as_uint(__uint_as_float(val) - a.d_split);
				const size_t d = ((size_t)c0 + (size_t)c * n_c) * w + col;
				G.dst[0][d] = out;
				G.dst[1][d] = 0u;
				G.dst[2][d] = 0u;
			}
		}
	}
}

bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

}  // namespace

extern "C" {

int gsr_adam_step(const gsr_adam_group* groups, int num_groups, int num_rows, double beta1, double beta2, double eps,
                  long long step, const int* visible, void* stream)
{
	if (!groups || num_groups < 1 || num_groups > 6 || !optim_plan::rows_ok(num_rows) || !(eps >= 0.0)) return GSR_ERR_ARG;
	AdamArgs a;
	a.ngroups = 0;
	a.eps = (float)eps;
	a.ustart[0] = 0;
	for (int k = 0; k < num_groups; k++) {
		const gsr_adam_group& s = groups[k];
		if (s.width < 0 || s.width > optim_plan::MAX_WIDTH) return GSR_ERR_ARG;
		if (!s.grad || s.width == 0 || num_rows == 0) continue;
		if (!s.param || !s.exp_avg || !s.exp_avg_sq) return GSR_ERR_ARG;
		if (!aligned4(s.param) || !aligned4(s.grad) || !aligned4(s.exp_avg) || !aligned4(s.exp_avg_sq)) return GSR_ERR_ARG;
		optim_plan::AdamConsts c;
		if (!optim_plan::adam_consts(s.lr, beta1, beta2, step, &c)) return GSR_ERR_ARG;
		AdamGroup& g = a.g[a.ngroups];
		g.p = s.param; g.g = s.grad; g.m = s.exp_avg; g.v = s.exp_avg_sq;
		g.n = (unsigned)num_rows * (unsigned)s.width;
		g.w = (unsigned)s.width;
		const unsigned off = (unsigned)((uintptr_t)s.param & 15u);
		g.vec = ((uintptr_t)s.grad & 15u) == off && ((uintptr_t)s.exp_avg & 15u) == off && ((uintptr_t)s.exp_avg_sq & 15u) == off;
		g.shift = g.vec ? off / 4u : 0u;
		g.c1 = c.c1; g.c2 = c.c2; g.sqrt_bc2 = c.sqrt_bc2; g.step_size = c.step_size;
		a.ustart[a.ngroups + 1] = a.ustart[a.ngroups] + optim_plan::units_of(g.n, g.shift);
		a.ngroups++;
	}
	if (a.ngroups == 0) return GSR_OK;
	for (int k = a.ngroups; k < 6; k++) { a.g[k] = a.g[0]; a.ustart[k + 1] = a.ustart[a.ngroups]; }
	hipLaunchKernelGGL(adam_kernel, dim3(capped_grid(a.ustart[a.ngroups])), dim3(256), 0, (hipStream_t)stream, a, visible);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_density_accumulate(int num_rows, const float* means2d_grad, const int* radii, float* grad_accum, int* denom,
                           int* max_radii, void* stream)
{
	if (!optim_plan::rows_ok(num_rows)) return GSR_ERR_ARG;
	if (num_rows == 0) return GSR_OK;
	if (!means2d_grad || !radii || !grad_accum || !denom || !max_radii) return GSR_ERR_ARG;
	hipLaunchKernelGGL(accumulate_kernel, dim3(capped_grid((unsigned long long)num_rows)), dim3(256), 0, (hipStream_t)stream,
	                   num_rows, means2d_grad, radii, grad_accum, denom, max_radii);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

int gsr_densify_classify(gsr_alloc_fn workspace_alloc, void* workspace_ctx, int num_rows, const float* scaling,
                         const float* opacity, const float* grad_accum, const int* denom, const int* max_radii,
                         const unsigned char* prune_mask, float max_grad, double percent_dense, double extent,
                         double min_opacity, int max_screen_size, int n_split, int* pos, long long* totals_host, void* stream)
{
	if (!optim_plan::rows_ok(num_rows) || !pos || !totals_host || !workspace_alloc) return GSR_ERR_ARG;
	ClassifyArgs c = {};
	if (!prune_mask) {
		optim_plan::Thresholds t;
		if (!optim_plan::thresholds(percent_dense, extent, min_opacity, n_split, &t)) return GSR_ERR_ARG;
		if (num_rows > 0 && (!scaling || !opacity || !grad_accum || !denom || !max_radii)) return GSR_ERR_ARG;
		c.max_grad = max_grad; c.t_big = t.t_big; c.t_world = t.t_world; c.t_op = t.t_op; c.d_split = t.d_split;
		c.max_screen_size = max_screen_size;
	} else {
		n_split = 1;
	}
	hipStream_t s = (hipStream_t)stream;
	const long long n3 = 3LL * num_rows;
	int *flag = nullptr, *part = nullptr, *tot = nullptr;
	if (!ws_carve(workspace_alloc, workspace_ctx, [&](Arena& ws) {
		    flag = ws.take<int>((size_t)n3 + 1);
		    part = ws.take<int>((size_t)scan_part_len(n3));
		    tot = ws.take<int>(4);
	    }))
		return GSR_ERR_ALLOC;
	if (num_rows > 0)
		hipLaunchKernelGGL(classify_kernel, dim3(capped_grid((unsigned long long)num_rows)), dim3(256), 0, s, num_rows, scaling,
		                   opacity, grad_accum, denom, max_radii, prune_mask, c, flag);
	const int rc = exclusive_scan<int>(flag, (int)n3, pos, part, s);
	if (rc != GSR_OK) return rc;
	hipLaunchKernelGGL(totals_kernel, dim3(1), dim3(64), 0, s, pos, num_rows, tot);
	int h[3] = {0, 0, 0};
	GSR_TRY(hipMemcpyAsync(h, tot, sizeof(h), hipMemcpyDeviceToHost, s));
	GSR_TRY(hipStreamSynchronize(s));
	const long long after = optim_plan::rows_after(h, n_split);
	totals_host[0] = h[0]; totals_host[1] = h[1]; totals_host[2] = h[2]; totals_host[3] = after;
	return after < 0 ? GSR_ERR_ARG : GSR_OK;
}

int gsr_densify_emit(int num_rows, int n_split, const gsr_compact_group* groups, int num_groups, const int* pos,
                     const float* noise, const float* scaling, const float* rotation, void* stream)
{
	if (!optim_plan::rows_ok(num_rows) || !groups || num_groups < 1 || num_groups > 8 || !pos) return GSR_ERR_ARG;
	if (n_split < 1 || n_split > optim_plan::MAX_SPLIT) return GSR_ERR_ARG;
	if (num_rows == 0) return GSR_OK;
	EmitArgs a;
	a.ngroups = 0;
	a.n = num_rows;
	a.n_split = n_split;
	a.d_split = (float)log(0.8 * (double)n_split);
	a.start[0] = 0;
	for (int k = 0; k < num_groups; k++) {
		const gsr_compact_group& s = groups[k];
		if (s.width < 0 || s.width > optim_plan::MAX_WIDTH || s.kind < GSR_COMPACT_COPY || s.kind > GSR_COMPACT_STATS) return GSR_ERR_ARG;
		if (s.width == 0) continue;
		if ((s.kind == GSR_COMPACT_XYZ || s.kind == GSR_COMPACT_SCALING) && s.width != 3) return GSR_ERR_ARG;
		if (s.kind == GSR_COMPACT_XYZ && (!scaling || !rotation || !noise)) return GSR_ERR_ARG;
		EmitGroup& g = a.g[a.ngroups];
		for (int j = 0; j < 3; j++) {
			if (!s.src[j]) return GSR_ERR_ARG;       // a destination may be NULL only when nothing survives: checked by the caller
			g.src[j] = static_cast<const uint32_t*>(s.src[j]);
			g.dst[j] = static_cast<uint32_t*>(s.dst[j]);
		}
		g.w = (unsigned)s.width;
		g.kind = s.kind;
		a.start[a.ngroups + 1] = a.start[a.ngroups] + (unsigned long long)num_rows * (unsigned)s.width;
		a.ngroups++;
	}
	if (a.ngroups == 0) return GSR_OK;
	for (int k = a.ngroups; k < 8; k++) { a.g[k] = a.g[0]; a.start[k + 1] = a.start[a.ngroups]; }
	hipLaunchKernelGGL(emit_kernel, dim3(capped_grid(a.start[a.ngroups])), dim3(256), 0, (hipStream_t)stream, a, pos, noise,
	                   scaling, rotation);
	return hipGetLastError() == hipSuccess ? GSR_OK : GSR_ERR_HIP;
}

}  // extern "C"
